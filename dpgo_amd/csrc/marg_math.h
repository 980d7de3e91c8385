// The arithmetic of one block of the relative joint marginal (marg.h): with b the base pose and k, l two other kept poses,
//     C_kl = A_k S_bb A_l^T + A_k S_bl B_l^T + B_k S_kb A_l^T + B_k S_kl B_l^T,
// A_k = J_p(b, k), B_k = J_q(b, k) of pairs_math.h.  J is never formed dense: J_q = blkdiag(Y_b, I), and J_p has the blocks
// -Y_b, hat(t_bk) and the rotation block -R_bk^T (D = 2: -1), its lower-left block zero.  Row i of the output block is
//     p_i = row i of (A_k S_bb + B_k S_kb),   q_i = row i of (A_k S_bl + B_k S_kl),   C_kl[i][j] = p_i . A_l[j] + q_i . B_l[j]
// -- the four terms, summed in this fixed order.  Every product is an explicit fma and every other operation a single add or
// negation, so no compiler may contract or reorder anything: k_marg_rel (marg.hip) with one lane per block and
// dpgo_debug_marg_rel_host (capi_debug.cpp) on the host give the same bits.
#pragma once
#include "pairs_math.h"

namespace dpgo {

// the blocks of J_p(b, k) and J_q(b, k) that are neither zero nor the identity, read out of pairs_jacobian's J
template <int D>
struct MargJac {
  static constexpr int DOF = PairsDims<D>::DOF, R = DOF - D;
  double Y[D * D];   // J_q's translation block Y_b = R_b^T; J_p's is -Y
  double H[D * R];   // hat(t_bk), D x R
  double G[R * R];   // J_p's rotation block
};

template <int D>
PAIRS_HD void marg_jac(const double *recb, const double *reck, MargJac<D> &jac) {
  constexpr int DOF = PairsDims<D>::DOF, R = DOF - D, LD = 2 * DOF;
  double Rbk[D * D], tbk[D], J[DOF * LD];
  pairs_relative<D>(recb, reck, Rbk, tbk);
  pairs_jacobian<D>(recb, Rbk, tbk, J);
#pragma unroll
  for (int i = 0; i < D; i++) {
#pragma unroll
    for (int j = 0; j < D; j++) jac.Y[i * D + j] = J[i * LD + DOF + j];
#pragma unroll
    for (int j = 0; j < R; j++) jac.H[i * R + j] = J[i * LD + D + j];
  }
#pragma unroll
  for (int i = 0; i < R; i++)
#pragma unroll
    for (int j = 0; j < R; j++) jac.G[i * R + j] = J[(D + i) * LD + D + j];
}

// out (DOF) <- row i of A_k S1 + B_k S2: S1 the block on the base's rows, S2 the block on k's rows, leading dimension ld
template <int D>
PAIRS_HD void marg_left_row(const MargJac<D> &k, int i, const double *S1, const double *S2, long long ld, double *out) {
  constexpr int DOF = PairsDims<D>::DOF, R = DOF - D;
#pragma unroll
  for (int c = 0; c < DOF; c++) {
    double s = 0.0;
    if (i < D) {
#pragma unroll
      for (int j = 0; j < D; j++) s = fma(-k.Y[i * D + j], S1[j * ld + c], s);
#pragma unroll
      for (int j = 0; j < R; j++) s = fma(k.H[i * R + j], S1[(D + j) * ld + c], s);
#pragma unroll
      for (int j = 0; j < D; j++) s = fma(k.Y[i * D + j], S2[j * ld + c], s);
    } else {
#pragma unroll
      for (int j = 0; j < R; j++) s = fma(k.G[(i - D) * R + j], S1[(D + j) * ld + c], s);
      s = s + S2[i * ld + c];
    }
    out[c] = s;
  }
}

// p . A_l[j] + q . B_l[j]
template <int D>
PAIRS_HD double marg_right(const MargJac<D> &l, int j, const double *p, const double *q) {
  constexpr int DOF = PairsDims<D>::DOF, R = DOF - D;
  double s = 0.0;
  if (j < D) {
#pragma unroll
    for (int c = 0; c < D; c++) s = fma(p[c], -l.Y[j * D + c], s);
#pragma unroll
    for (int c = 0; c < R; c++) s = fma(p[D + c], l.H[j * R + c], s);
#pragma unroll
    for (int c = 0; c < D; c++) s = fma(q[c], l.Y[j * D + c], s);
  } else {
#pragma unroll
    for (int c = 0; c < R; c++) s = fma(p[D + c], l.G[(j - D) * R + c], s);
    s = s + q[j];
  }
  return s;
}

// Block (ko, lo), ko >= lo, of the relative covariance, ko / lo counting the kept poses without the base: written at
// C[(DOF ko + i) ldc + DOF lo + j] and, transposed, as block (lo, ko); of a diagonal block the lower triangle is computed and
// mirrored.  sig: Sigma_KK (ld its order) in list order, b / k / l the positions of the base and the two poses in that list;
// rec*: their pose records.  C2 (optional): a second copy, same layout.
template <int D>
PAIRS_HD void marg_rel_block(const double *recb, const double *reck, const double *recl, const double *sig, long long ld, int b, int k,
                             int l, int ko, int lo, double *C, double *C2, long long ldc) {
  constexpr int DOF = PairsDims<D>::DOF;
  MargJac<D> jk, jl;
  marg_jac<D>(recb, reck, jk);
  marg_jac<D>(recb, recl, jl);
  const double *Sbb = sig + (long long)DOF * b * ld + (long long)DOF * b, *Skb = sig + (long long)DOF * k * ld + (long long)DOF * b;
  const double *Sbl = sig + (long long)DOF * b * ld + (long long)DOF * l, *Skl = sig + (long long)DOF * k * ld + (long long)DOF * l;
  const long long r0 = (long long)DOF * ko, c0 = (long long)DOF * lo;
#pragma unroll
  for (int i = 0; i < DOF; i++) {
    double p[DOF], q[DOF];
    marg_left_row<D>(jk, i, Sbb, Skb, ld, p);
    marg_left_row<D>(jk, i, Sbl, Skl, ld, q);
#pragma unroll
    for (int j = 0; j < DOF; j++) {
      if (ko == lo && j > i) continue;
      const double v = marg_right<D>(jl, j, p, q);
      C[(r0 + i) * ldc + c0 + j] = v;
      C[(c0 + j) * ldc + r0 + i] = v;
      if (C2) {
        C2[(r0 + i) * ldc + c0 + j] = v;
        C2[(c0 + j) * ldc + r0 + i] = v;
      }
    }
  }
}

}  // namespace dpgo
