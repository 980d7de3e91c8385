// The arithmetic of a set of loop-closure candidates (cand.h), shared by the kernels (cand.hip) and the host hooks (cand.cpp):
//
//  * one block of the joint innovation covariance.  With A_i = J_p(p_i, q_i), B_i = J_q(p_i, q_i) of pairs_math.h,
//        cov_ij = A_i S[p_i,p_j] A_j^T + B_i S[q_i,p_j] A_j^T + A_i S[p_i,q_j] B_j^T + B_i S[q_i,q_j] B_j^T,
//    computed with marg_math.h's marg_jac / marg_left_row / marg_right exactly as marg_rel_block computes a block of the
//    relative joint marginal -- for a star set (every p_i the same pose) the two give the same bits.  Every product is an
//    explicit fma, the reciprocals of the weights are IEEE divisions and S = cov + blkdiag(Omega_i^-1) is one add per entry:
//    host and device agree bit for bit;
//  * a candidate's residual (pairs_relative, pairs_residual);
//  * the score of one candidate in the greedy selection: the Cholesky of its conditional innovation covariance C_i in registers
//    (pairs_mahalanobis' loop), gain_i = 1/2 (log det C_i - log det Omega_i^-1) and d2_i = rho_i^T C_i^-1 rho_i;
//  * the pivot of a selection step (L_ss and z_s = L_ss^-1 rho_s) and one row of its panel.
#pragma once
#include "marg_math.h"

namespace dpgo {

// 1 / tau on the translation part, 1 / (2 kappa) on the rotation part: the diagonal of Omega^-1
PAIRS_HD void cand_omega_inv(double kappa, double tau, double *w) {
  w[0] = 1.0 / tau;
  w[1] = 1.0 / (2.0 * kappa);
}

// Block (i, j), i >= j, of cov = J Sigma_KK J^T and of S = cov + blkdiag(Omega^-1), n their order.  sig: Sigma_KK (ld its order)
// in the order of the list K; kpi, kqi, kpj, kqj: the positions of the four end poses in K; rec*: their records; wi: Omega_i^-1's
// two values (read where i == j).  Block (j, i) is written as the transpose; of a diagonal block the lower triangle is
// computed and mirrored.  cov, S2 are optional.
template <int D>
PAIRS_HD void cand_innov_block(const double *recpi, const double *recqi, const double *recpj, const double *recqj, const double *sig,
                               long long ld, int kpi, int kqi, int kpj, int kqj, int i, int j, const double *wi, double *cov, double *S,
                               double *S2, long long n) {
  constexpr int DOF = PairsDims<D>::DOF;
  MargJac<D> ji, jj;
  marg_jac<D>(recpi, recqi, ji);
  marg_jac<D>(recpj, recqj, jj);
  const double *Spp = sig + (long long)DOF * kpi * ld + (long long)DOF * kpj, *Sqp = sig + (long long)DOF * kqi * ld + (long long)DOF * kpj;
  const double *Spq = sig + (long long)DOF * kpi * ld + (long long)DOF * kqj, *Sqq = sig + (long long)DOF * kqi * ld + (long long)DOF * kqj;
  const long long r0 = (long long)DOF * i, c0 = (long long)DOF * j;
#pragma unroll
  for (int a = 0; a < DOF; a++) {
    double p[DOF], q[DOF];
    marg_left_row<D>(ji, a, Spp, Sqp, ld, p);
    marg_left_row<D>(ji, a, Spq, Sqq, ld, q);
#pragma unroll
    for (int b = 0; b < DOF; b++) {
      if (i == j && b > a) continue;
      const double v = marg_right<D>(jj, b, p, q);
      const long long lo = (r0 + a) * n + c0 + b, up = (c0 + b) * n + r0 + a;
      if (cov) {
        cov[lo] = v;
        cov[up] = v;
      }
      const double s = (i == j && a == b) ? v + wi[a < D ? 0 : 1] : v;
      S[lo] = s;
      S[up] = s;
      if (S2) {
        S2[lo] = s;
        S2[up] = s;
      }
    }
  }
}

// r (DOF) of a candidate between the poses with these records
template <int D>
PAIRS_HD void cand_residual(const double *recp, const double *recq, const double *cand, double *r) {
  double Rpq[D * D], tpq[D];
  pairs_relative<D>(recp, recq, Rpq, tpq);
  pairs_residual<D>(Rpq, tpq, cand, r);
}

// The Cholesky C = L L^T (lower triangle of C read; L's lower triangle written, the rest untouched) and z = L^-1 rho;
// *logdet <- log det C, *d2 <- z^T z.  false where a pivot is not positive.
template <int D>
PAIRS_HD bool cand_chol(const double *C, const double *rho, double *L, double *z, double *logdet, double *d2) {
  constexpr int DOF = PairsDims<D>::DOF;
  double acc = 0.0, lg = 0.0;
  *logdet = 0.0;
  *d2 = 0.0;
#pragma unroll
  for (int j = 0; j < DOF; j++) {
    double dj = C[j * DOF + j];
#pragma unroll
    for (int k = 0; k < DOF; k++)
      if (k < j) dj = fma(-L[j * DOF + k], L[j * DOF + k], dj);
    if (!(dj > 0.0)) return false;
    const double lj = sqrt(dj);
    L[j * DOF + j] = lj;
    lg += log(lj);
#pragma unroll
    for (int i = 0; i < DOF; i++)
      if (i > j) {
        double s = C[i * DOF + j];
#pragma unroll
        for (int k = 0; k < DOF; k++)
          if (k < j) s = fma(-L[i * DOF + k], L[j * DOF + k], s);
        L[i * DOF + j] = s / lj;
      }
    double zj = rho[j];
#pragma unroll
    for (int k = 0; k < DOF; k++)
      if (k < j) zj = fma(-L[j * DOF + k], z[k], zj);
    z[j] = zj / lj;
    acc = fma(z[j], z[j], acc);
  }
  *logdet = 2.0 * lg;
  *d2 = acc;
  return true;
}

// log det Omega^-1 from its two values
template <int D>
PAIRS_HD double cand_logdet_omega_inv(const double *w) {
  return D * log(w[0]) + (PairsDims<D>::DOF - D) * log(w[1]);
}

// One candidate's score: gain = 1/2 (log det C - log det Omega^-1), d2 = rho^T C^-1 rho.  false (gain = d2 = 0): C is not
// positive definite.
template <int D>
PAIRS_HD bool cand_score_one(const double *C, const double *rho, const double *w, double *gain, double *d2) {
  constexpr int DOF = PairsDims<D>::DOF;
  double L[DOF * DOF], z[DOF], lg;
  *gain = 0.0;
  if (!cand_chol<D>(C, rho, L, z, &lg, d2)) {
    *d2 = 0.0;
    return false;
  }
  *gain = 0.5 * (lg - cand_logdet_omega_inv<D>(w));
  return true;
}

// The order of the argmax: a beats b iff its gain is larger, or equal with the lower index -- associative and commutative, so
// every reduction order gives the same winner.
PAIRS_HD bool cand_better(double ga, int ia, double gb, int ib) {
  if (ia < 0) return false;
  if (ib < 0) return true;
  return ga > gb || (ga == gb && ia < ib);
}

// Row `a` of the panel of step t with pivot candidate s: v = S[a, s's columns] - sum_{u < t} P_u[a] P_u[s's rows]^T (u and the
// inner index ascending), x = v L_ss^-T.  P: entry (row a, column c) at P[c n + a], column c = DOF u + k; piv: L_ss (DOF x DOF).
template <int D>
PAIRS_HD void cand_panel_row(const double *S, const double *P, long long n, int t, int s, long long a, const double *piv, double *x) {
  constexpr int DOF = PairsDims<D>::DOF;
  double v[DOF];
#pragma unroll
  for (int c = 0; c < DOF; c++) v[c] = S[a * n + (long long)DOF * s + c];
  for (int u = 0; u < t; u++)
#pragma unroll
    for (int k = 0; k < DOF; k++) {
      const double pa = P[((long long)DOF * u + k) * n + a];
#pragma unroll
      for (int c = 0; c < DOF; c++) v[c] = fma(-pa, P[((long long)DOF * u + k) * n + (long long)DOF * s + c], v[c]);
    }
#pragma unroll
  for (int c = 0; c < DOF; c++) {
    double xc = v[c];
#pragma unroll
    for (int k = 0; k < DOF; k++)
      if (k < c) xc = fma(-x[k], piv[c * DOF + k], xc);
    x[c] = xc / piv[c * DOF + c];
  }
}

}  // namespace dpgo
