// The weighted per-edge arithmetic of graduated non-convexity on the maximum-likelihood objective (ml_gnc.h), as functions the
// device kernel (ml_gnc.hip) and the host's debug hook (ml_gnc_edge_host, ml_gnc.cpp; no GPU needed) both compile.  It takes
// what ml_math.h computed for the edge -- J_i, J_j, Omega r -- and a weight w in [0, 1], and writes what the gather and the
// Hessian kernel of ml.hip read: wr = w (Omega r), the gradient terms J' wr, and the record [J_i | J_j | w Omega J_i | w Omega J_j].
//
// One rounding per scaled value (no FMA contraction of the scaling), explicit FMAs only inside ml_math.h's own functions.
//
// The zero selection.  An outlier's rotation residual may sit at theta > pi - 1e-3, where ml_residual's values are not
// specified further -- they may not even be finite.  An edge of weight exactly 0 therefore contributes exact zeros BY
// SELECTION, never by multiplication (0 * NaN = NaN): wr, both gradient terms and the whole record are +0.0.  The J halves
// of the record are zeroed with the Omega J halves: ml_block_entry multiplies the one by the other, and 0 * J is a NaN again
// where J is not finite.  With w == 1 every value has the bits of k_ml_edge<D, true> (1 * x == x).
#pragma once
#include "ml_math.h"

namespace dpgo {

// w v in one rounding, +0.0 where w == 0 whatever v holds
__host__ __device__ inline double ml_gnc_scale(double w, double v) {
#pragma clang fp contract(off)
  return w == 0.0 ? 0.0 : w * v;
}

// the edge's term of sum_R w chi2, by the same selection
__host__ __device__ inline double ml_gnc_wchi2(double w, double chi2) { return ml_gnc_scale(w, chi2); }

// or: Omega r as ml_weigh left it.  Written: wr (dof), gi, gj (dof: the edge's gradient terms of pose i, of pose j) and jw
// (ml_jw_doubles).  The outputs may be global memory: every entry is written once and none is read back.
template <int D>
__host__ __device__ inline void ml_gnc_edge_out(double w, const double *Om, const double *Ji, const double *Jj, const double *orr,
                                                double *wr, double *gi, double *gj, double *jw) {
  constexpr int DOF = cov_dof(D), DD = DOF * DOF;
  if (w == 0.0) {
#pragma unroll
    for (int k = 0; k < DOF; k++) wr[k] = gi[k] = gj[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 4 * DD; k++) jw[k] = 0.0;
    return;
  }
  double s[DOF];
#pragma unroll
  for (int k = 0; k < DOF; k++) wr[k] = s[k] = ml_gnc_scale(w, orr[k]);
#pragma unroll
  for (int k = 0; k < DOF; k++) {
    gi[k] = ml_grad_entry<D>(Ji, s, k);
    gj[k] = ml_grad_entry<D>(Jj, s, k);
  }
#pragma unroll
  for (int k = 0; k < DD; k++) {
    jw[k] = Ji[k];
    jw[DD + k] = Jj[k];
  }
#pragma unroll
  for (int k = 0; k < DOF; k++)
#pragma unroll
    for (int c = 0; c < DOF; c++) {
      jw[2 * DD + k * DOF + c] = ml_gnc_scale(w, ml_w_entry<D>(Om, Ji, k, c));
      jw[3 * DD + k * DOF + c] = ml_gnc_scale(w, ml_w_entry<D>(Om, Jj, k, c));
    }
}

}  // namespace dpgo
