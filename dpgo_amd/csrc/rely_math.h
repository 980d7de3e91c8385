// The arithmetic of one edge's reliability record (rely.h) from the covariance of its relative pose, its residual and its own
// weights: the residual covariance C = Omega^-1 - rel, its Cholesky factor, the leave-one-out statistic, residual and
// influence, the redundancy numbers.  Plain fp64 in a fixed order, explicit fma, no memory but the caller's arrays:
// k_rely_edge (rely.hip) runs it with one lane per edge, dpgo_debug_rely_edge_host (capi_debug.cpp) on the host.
//
// rel (DOF x DOF row-major) and r (DOF) are pairs_math.h's, with the edge's own (R~, t~, kappa, tau) taken as the candidate;
// Omega = blkdiag(tau I_D, 2 kappa I_{DOF - D}).
#pragma once
#include <cmath>

#include "pairs_math.h"

namespace dpgo {

enum { RELY_FLAG_OK = 0, RELY_FLAG_NOT_PD = 1, RELY_FLAG_UNWEIGHTED = 2 };

template <int D>
struct RelyDims {
  static constexpr int DOF = PairsDims<D>::DOF, WIDTH = 6 + 2 * DOF;
  // the record: d2_loo, flag, redundancy, redundancy_trans, d2_own, influence, r[DOF], r_loo[DOF]
  static constexpr int D2_LOO = 0, FLAG = 1, RED = 2, RED_TRANS = 3, D2_OWN = 4, INFLUENCE = 5, R = 6, R_LOO = 6 + DOF;
};

// out (WIDTH doubles).  flag 2 (kappa or tau not > 0): zeros but the flag.  flag 1 (a pivot of C not > 0): d2_loo, influence
// and r_loo exact zeros, the rest filled.  The Cholesky of C's lower triangle runs in pairs_mahalanobis' loop order, with the
// forward substitution y = L^-1 r folded into it: d2_loo = |y|^2; then z = L^-T y = C^-1 r, r_loo = Omega^-1 z,
// influence = z^T rel z.
template <int D>
PAIRS_HD void rely_one(const double *rel, const double *r, double kappa, double tau, double *out) {
  typedef RelyDims<D> Q;
  constexpr int DOF = Q::DOF;
#pragma unroll
  for (int i = 0; i < Q::WIDTH; i++) out[i] = 0.0;
  if (!(kappa > 0.0) || !(tau > 0.0)) {
    out[Q::FLAG] = (double)RELY_FLAG_UNWEIGHTED;
    return;
  }
  const double wt = tau, wr = 2.0 * kappa, it = 1.0 / tau, ir = 1.0 / (2.0 * kappa);
  double tr = 0.0, trt = 0.0, own = 0.0;
#pragma unroll
  for (int i = 0; i < DOF; i++) {
    const double w = i < D ? wt : wr;
    tr = fma(w, rel[i * DOF + i], tr);
    if (i < D) trt += rel[i * DOF + i];
    own = fma(w * r[i], r[i], own);
    out[Q::R + i] = r[i];
  }
  out[Q::RED] = (double)DOF - tr;
  out[Q::RED_TRANS] = (double)D - tau * trt;
  out[Q::D2_OWN] = own;
  double L[DOF * DOF], z[DOF];
#pragma unroll
  for (int i = 0; i < DOF; i++)
#pragma unroll
    for (int j = 0; j < DOF; j++) L[i * DOF + j] = (i == j ? (i < D ? it : ir) : 0.0) - rel[i * DOF + j];
  double acc = 0.0;
  bool pd = true;
#pragma unroll
  for (int j = 0; j < DOF; j++) {
    double dj = L[j * DOF + j];
#pragma unroll
    for (int k = 0; k < DOF; k++)
      if (k < j) dj = fma(-L[j * DOF + k], L[j * DOF + k], dj);
    if (!(dj > 0.0)) {
      pd = false;
      break;
    }
    const double lj = sqrt(dj);
    L[j * DOF + j] = lj;
#pragma unroll
    for (int i = 0; i < DOF; i++)
      if (i > j) {
        double s = L[i * DOF + j];
#pragma unroll
        for (int k = 0; k < DOF; k++)
          if (k < j) s = fma(-L[i * DOF + k], L[j * DOF + k], s);
        L[i * DOF + j] = s / lj;
      }
    double zj = r[j];
#pragma unroll
    for (int k = 0; k < DOF; k++)
      if (k < j) zj = fma(-L[j * DOF + k], z[k], zj);
    z[j] = zj / lj;
    acc = fma(z[j], z[j], acc);
  }
  if (!pd) {
    out[Q::FLAG] = (double)RELY_FLAG_NOT_PD;
    return;
  }
  out[Q::D2_LOO] = acc;
  // z <- L^-T y, last row first
#pragma unroll
  for (int jj = 0; jj < DOF; jj++) {
    const int j = DOF - 1 - jj;
    double zj = z[j];
#pragma unroll
    for (int k = 0; k < DOF; k++)
      if (k > j) zj = fma(-L[k * DOF + j], z[k], zj);
    z[j] = zj / L[j * DOF + j];
  }
  double infl = 0.0;
#pragma unroll
  for (int i = 0; i < DOF; i++) {
    out[Q::R_LOO + i] = (i < D ? it : ir) * z[i];
    double t = 0.0;
#pragma unroll
    for (int j = 0; j < DOF; j++) t = fma(rel[i * DOF + j], z[j], t);
    infl = fma(z[i], t, infl);
  }
  out[Q::INFLUENCE] = infl;
}

}  // namespace dpgo
