// The per-edge computation of k_edge_eval (edges.hip), as one function the device kernel and the host's debug restatement
// (edge_eval_host, edges.cpp; no GPU needed) both compile: record unpacking, residuals, loss.  edges.h has the definitions.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "edges.h"

namespace dpgo {

// DPGOProblem.cpp:651-670 with delta = dl (the formulas of k_inter's loss_weight, kernels.hip)
__host__ __device__ inline void edge_loss(int loss, double dl, double s, double &w, double &rho) {
  if (loss == 1) {          // Huber
    const double rs = sqrt(fmax(s, dl)), sd = sqrt(dl);
    w = sd / rs;
    rho = fmin(2.0 * sd * rs - dl, s);
  } else if (loss == 2) {   // Geman-McClure
    const double q = s + dl;
    w = dl * dl / (q * q);
    rho = dl * (s / q);
  } else if (loss == 3) {   // Welsch: rho = delta - delta w, written -delta expm1(-s / delta) -- the same number without the
    const double x = -s / dl;   // cancellation that costs delta u / rho of relative accuracy where s << delta
    w = exp(x);
    rho = -dl * expm1(x);
  } else {
    w = 1.0;
    rho = s;
  }
}

// the ints of a record's unit 0: i, j, inter
__host__ __device__ inline void edge_head(const double *q, int &i, int &j, bool &inter) {
  unsigned long long h0, h1;
  memcpy(&h0, q, 8);
  memcpy(&h1, q + 1, 8);
  i = (int)(unsigned)(h0 & 0xffffffffull);
  j = (int)(unsigned)(h0 >> 32);
  inter = (h1 & 0xffffffffull) != 0;
}

// q: the edge record; a, b: the pose records [t | rows of Y] of its poses i and j.  v = {s_rot, s_trans, rho, w}.
template <int D>
__host__ __device__ inline void edge_lane(const double *q, const double *a, const double *b, bool inter, int loss, double dl,
                                          double (&v)[4]) {
  const double *R = q + 2, *t = q + 2 + D * D;
  const double kappa = q[2 + D * D + D], tau = q[2 + D * D + D + 1];
  const double *Yi = a + D, *Yj = b + D;
  double er = 0, et = 0;
#pragma unroll
  for (int c = 0; c < D; c++) {
    // (t_e^T Y_i)_c
    double p = 0;
#pragma unroll
    for (int k = 0; k < D; k++) p += t[k] * Yi[k * D + c];
    const double dt = (b[c] - a[c]) - p;
    et += dt * dt;
#pragma unroll
    for (int r = 0; r < D; r++) {
      // (R_e^T Y_i)_{r c}
      double g = 0;
#pragma unroll
      for (int k = 0; k < D; k++) g += R[k * D + r] * Yi[k * D + c];
      const double dr = Yj[r * D + c] - g;
      er += dr * dr;
    }
  }
  // s is the sum of the two ROUNDED parts the caller gets back (rho and w are functions of that s, and rho = s exactly on an
  // intra edge): no contraction of kappa * er into the sum
  double s;
  {
#pragma clang fp contract(off)
    v[0] = kappa * er;
    v[1] = tau * et;
    s = v[0] + v[1];
  }
  v[2] = s;
  v[3] = 1.0;
  if (inter) edge_loss(loss, dl, s, v[3], v[2]);
}

}  // namespace dpgo
