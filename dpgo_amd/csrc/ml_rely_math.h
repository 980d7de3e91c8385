// The arithmetic of one edge's reliability record and of one candidate's gate on the FULL information matrix (ml_rely.h): the
// covariance of the predicted residual rel = J Sigma_joint J^T entry by entry, and, on rel, Omega and r, the whitened form
//     Omega = L L^T (Cholesky, lower),   A = L^T rel L,   rho = L^T r,
// on which everything else is stated -- Omega^-1 is never formed:
//     d2_own = rho^T rho,   redundancy = dof - tr A,   redundancy_trans = d - sum_{a < d} (Omega rel)_aa,
//     SIGN -1 (reliability):  Q = I - A = K K^T,  y = K^-1 rho,  d2_loo = |y|^2,  zeta = K^-T y,  r_loo = L^-T zeta,
//                             influence = zeta^T A zeta        (C = Omega^-1 - rel = L^-T Q L^-1 of rely.h)
//     SIGN +1 (gate):         Q = I + A = K K^T,  y = K^-1 rho,  d2 = |y|^2        (= r^T (rel + Omega^-1)^-1 r of pairs.h)
// A's eigenvalues lie in [0, 1] where the Gauss-Newton model holds, whatever the scale of Omega.  Plain fp64 in a fixed order,
// explicit fma, no memory but the caller's arrays: k_ml_rel and k_ml_rely_edge (ml_rely.hip) run it on the device,
// ml_rely_edge_host (ml_rely.cpp) on the host, with the same bits.
//
// J = [J_p | J_q], two DOF x DOF row-major blocks as k_ml_edge<FULL> stores them (ml_math.h); joint = [S_pp | S_pq | S_qq],
// pairs.h's layout (S_pq: rows of p, columns of q); Omega, rel: DOF x DOF row-major; only the lower triangle of rel is read.
#pragma once
#include <cmath>

#include "cov.h"
#include "rely_math.h"

namespace dpgo {

template <int D>
struct MlGateDims {
  static constexpr int DOF = cov_dof(D), WIDTH = 2 + DOF;
  // the record (pairs.h's): d2, not_pd, residual[DOF]
  static constexpr int D2 = 0, NOT_PD = 1, R = 2;
};

// Entry (a, b) of rel = J_p S_pp J_p^T + J_p S_pq J_q^T + J_q S_pq^T J_p^T + J_q S_qq J_q^T: one sum over the four terms in
// that order, each over k ascending of J[a][k] (sum over l ascending of S[k][l] J'[b][l]).  The caller evaluates a >= b and
// writes both places.
template <int D>
__host__ __device__ inline double ml_rel_entry(const double *Jp, const double *Jq, const double *joint, int a, int b) {
  constexpr int DOF = cov_dof(D), DD = DOF * DOF;
  const double *Spp = joint, *Spq = joint + DD, *Sqq = joint + 2 * DD;
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < DOF; k++) {   // pp
    double t = 0.0;
#pragma unroll
    for (int l = 0; l < DOF; l++) t = fma(Spp[k * DOF + l], Jp[b * DOF + l], t);
    s = fma(Jp[a * DOF + k], t, s);
  }
#pragma unroll
  for (int k = 0; k < DOF; k++) {   // pq
    double t = 0.0;
#pragma unroll
    for (int l = 0; l < DOF; l++) t = fma(Spq[k * DOF + l], Jq[b * DOF + l], t);
    s = fma(Jp[a * DOF + k], t, s);
  }
#pragma unroll
  for (int k = 0; k < DOF; k++) {   // qp: S_qp = S_pq^T
    double t = 0.0;
#pragma unroll
    for (int l = 0; l < DOF; l++) t = fma(Spq[l * DOF + k], Jp[b * DOF + l], t);
    s = fma(Jq[a * DOF + k], t, s);
  }
#pragma unroll
  for (int k = 0; k < DOF; k++) {   // qq
    double t = 0.0;
#pragma unroll
    for (int l = 0; l < DOF; l++) t = fma(Sqq[k * DOF + l], Jq[b * DOF + l], t);
    s = fma(Jq[a * DOF + k], t, s);
  }
  return s;
}

// out: SIGN -1: RelyDims<D>::WIDTH doubles, d2_loo, flag, redundancy, redundancy_trans, d2_own, influence, r[DOF], r_loo[DOF];
// flag 1 (a pivot of Q not > 0): d2_loo, influence and r_loo exact zeros, the rest filled.  SIGN +1: MlGateDims<D>::WIDTH
// doubles, d2, not_pd, r[DOF]; not_pd 1: d2 an exact zero.  Omega is symmetric positive definite (ml_check_information
// refuses anything else before a plan exists), so L's pivots are taken as they come.  The Cholesky of Q runs in rely_one's loop
// order with the forward substitution y = K^-1 rho folded into it; behind a pivot that is not > 0 the loop runs on with a
// unit pivot -- no branch, and nothing of it is handed out.
template <int D, int SIGN>
__host__ __device__ inline void ml_rely_one(const double *rel, const double *Om, const double *r, double *out) {
  typedef RelyDims<D> Q;
  typedef MlGateDims<D> G;
  constexpr int DOF = Q::DOF;
  static_assert(SIGN == 1 || SIGN == -1, "SIGN is +1 (the gate) or -1 (the reliability)");
  // (Omega rel)_aa of the translation rows, from the lower triangle of rel
  double trt = 0.0;
#pragma unroll
  for (int a = 0; a < D; a++)
#pragma unroll
    for (int k = 0; k < DOF; k++) trt = fma(Om[a * DOF + k], k >= a ? rel[k * DOF + a] : rel[a * DOF + k], trt);
  // Omega = L L^T, row by row
  double L[DOF * DOF];
#pragma unroll
  for (int j = 0; j < DOF; j++) {
    double dj = Om[j * DOF + j];
#pragma unroll
    for (int k = 0; k < DOF; k++)
      if (k < j) dj = fma(-L[j * DOF + k], L[j * DOF + k], dj);
    const double lj = sqrt(dj);
    L[j * DOF + j] = lj;
#pragma unroll
    for (int i = 0; i < DOF; i++)
      if (i > j) {
        double s = Om[i * DOF + j];
#pragma unroll
        for (int k = 0; k < DOF; k++)
          if (k < j) s = fma(-L[i * DOF + k], L[j * DOF + k], s);
        L[i * DOF + j] = s / lj;
      }
  }
  // T = rel L (rel's lower triangle mirrored), then the lower triangle of A = L^T T; rho = L^T r
  double A[DOF * DOF], rho[DOF];
  {
    double T[DOF * DOF];
#pragma unroll
    for (int i = 0; i < DOF; i++)
#pragma unroll
      for (int j = 0; j < DOF; j++) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < DOF; k++)
          if (k >= j) s = fma(k <= i ? rel[i * DOF + k] : rel[k * DOF + i], L[k * DOF + j], s);
        T[i * DOF + j] = s;
      }
#pragma unroll
    for (int i = 0; i < DOF; i++)
#pragma unroll
      for (int j = 0; j < DOF; j++)
        if (j <= i) {
          double s = 0.0;
#pragma unroll
          for (int k = 0; k < DOF; k++)
            if (k >= i) s = fma(L[k * DOF + i], T[k * DOF + j], s);
          A[i * DOF + j] = s;
        }
  }
  double tr = 0.0, own = 0.0;
#pragma unroll
  for (int i = 0; i < DOF; i++) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < DOF; k++)
      if (k >= i) s = fma(L[k * DOF + i], r[k], s);
    rho[i] = s;
    own = fma(s, s, own);
    tr += A[i * DOF + i];
  }
  // Q = I + SIGN A = K K^T with y = K^-1 rho folded in
  double K[DOF * DOF], y[DOF];
#pragma unroll
  for (int i = 0; i < DOF; i++)
#pragma unroll
    for (int j = 0; j < DOF; j++)
      if (j <= i) K[i * DOF + j] = SIGN > 0 ? (i == j ? 1.0 : 0.0) + A[i * DOF + j] : (i == j ? 1.0 : 0.0) - A[i * DOF + j];
  double acc = 0.0;
  bool pd = true;
#pragma unroll
  for (int j = 0; j < DOF; j++) {
    double dj = K[j * DOF + j];
#pragma unroll
    for (int k = 0; k < DOF; k++)
      if (k < j) dj = fma(-K[j * DOF + k], K[j * DOF + k], dj);
    const bool ok = dj > 0.0;
    pd = pd && ok;
    const double kj = ok ? sqrt(dj) : 1.0;
    K[j * DOF + j] = kj;
#pragma unroll
    for (int i = 0; i < DOF; i++)
      if (i > j) {
        double s = K[i * DOF + j];
#pragma unroll
        for (int k = 0; k < DOF; k++)
          if (k < j) s = fma(-K[i * DOF + k], K[j * DOF + k], s);
        K[i * DOF + j] = s / kj;
      }
    double yj = rho[j];
#pragma unroll
    for (int k = 0; k < DOF; k++)
      if (k < j) yj = fma(-K[j * DOF + k], y[k], yj);
    y[j] = yj / kj;
    acc = fma(y[j], y[j], acc);
  }
  if constexpr (SIGN > 0) {
    out[G::D2] = pd ? acc : 0.0;
    out[G::NOT_PD] = pd ? 0.0 : 1.0;
#pragma unroll
    for (int i = 0; i < DOF; i++) out[G::R + i] = r[i];
  } else {
    out[Q::FLAG] = pd ? (double)RELY_FLAG_OK : (double)RELY_FLAG_NOT_PD;
    out[Q::RED] = (double)DOF - tr;
    out[Q::RED_TRANS] = (double)D - trt;
    out[Q::D2_OWN] = own;
#pragma unroll
    for (int i = 0; i < DOF; i++) out[Q::R + i] = r[i];
    // zeta = K^-T y, last row first; x = L^-T zeta the same way
    double x[DOF];
#pragma unroll
    for (int jj = 0; jj < DOF; jj++) {
      const int j = DOF - 1 - jj;
      double zj = y[j];
#pragma unroll
      for (int k = 0; k < DOF; k++)
        if (k > j) zj = fma(-K[k * DOF + j], y[k], zj);
      y[j] = zj / K[j * DOF + j];
    }
    double infl = 0.0;
#pragma unroll
    for (int i = 0; i < DOF; i++) {
      double t = 0.0;
#pragma unroll
      for (int j = 0; j < DOF; j++) t = fma(j <= i ? A[i * DOF + j] : A[j * DOF + i], y[j], t);
      infl = fma(y[i], t, infl);
    }
#pragma unroll
    for (int jj = 0; jj < DOF; jj++) {
      const int j = DOF - 1 - jj;
      double xj = y[j];
#pragma unroll
      for (int k = 0; k < DOF; k++)
        if (k > j) xj = fma(-L[k * DOF + j], x[k], xj);
      x[j] = xj / L[j * DOF + j];
    }
    out[Q::D2_LOO] = pd ? acc : 0.0;
    out[Q::INFLUENCE] = pd ? infl : 0.0;
#pragma unroll
    for (int i = 0; i < DOF; i++) out[Q::R_LOO + i] = pd ? x[i] : 0.0;
  }
}

}  // namespace dpgo
