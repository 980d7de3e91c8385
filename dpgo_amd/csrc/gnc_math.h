// The weight and the surrogate of graduated non-convexity (gnc.h), as one function the device kernel (gnc.hip) and the host's
// debug hook (gnc_weight_host, gnc.cpp; no GPU needed) both compile.  Plain fp64 in the operation order of gnc.h; no FMA
// contraction, so that every operation rounds once, as the restated bound (tests/gnc_restatement.py) assumes.
#pragma once
#include "edge_math.h"

namespace dpgo {

// kind 0: TLS, otherwise GM.  mu > 0, c2 > 0, s >= 0.
__host__ __device__ inline void gnc_weight_rho(int kind, double mu, double c2, double s, double &w, double &rho) {
#pragma clang fp contract(off)
  if (kind == 0) {
    const double m1 = mu + 1.0;
    const double lo = mu / m1 * c2, hi = m1 / mu * c2;
    if (s <= lo) {
      w = 1.0;
      rho = s;
      return;
    }
    if (s >= hi) {
      w = 0.0;
      rho = c2;
      return;
    }
    const double a = c2 * (mu * m1);
    w = fmin(fmax(sqrt(a / s) - mu, 0.0), 1.0);
    rho = 2.0 * sqrt(a * s) - mu * (c2 + s);
  } else {
    edge_loss(2, mu * c2, s, w, rho);
  }
}

}  // namespace dpgo
