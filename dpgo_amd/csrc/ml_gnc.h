// Graduated non-convexity on the maximum-likelihood objective: GNC-TLS and GNC-GM outlier rejection on chi2_e = r_e' Omega_e r_e.
//
// gnc.h thresholds the isotropic chordal s_e = kappa |.|^2 + tau |.|^2: it ignores Omega_e, and its barc2 has no statistical
// meaning across edges of different noise.  chi2_e against a chi2_dof quantile is the test Yang et al.'s GNC, GTSAM's
// GncOptimizer and g2o's robust kernels apply.  ml_polish (ml.h) trusts every edge; this is its robust counterpart.
//
// Definitions.  r_e, J_i, J_j, Omega_e, near_pi, the anchor and Omega_iso exactly as ml.h has them.
//     s_e := chi2_e = r_e' Omega_e r_e
// c2 = barc2 > 0 is the caller's threshold on chi2_e: a chi2_dof quantile, dof = 3 (d = 2) or 6 (d = 3) -- 16.266 / 22.458 at
// 0.999.  (The library has no quantile function; the threshold stays the caller's.)  The robust set R: robust_set[e] != 0, or
// the inter-node rule of edges.h when robust_set is NULL.  w_e = 1 outside R.
//
//     F_w(X)  = 1/2 sum_e w_e chi2_e
//     F_mu(X) = 1/2 sum_{e not in R} chi2_e + 1/2 sum_{e in R} rho_mu(chi2_e)
//     g_w = sum_e w_e J_e' Omega_e r_e
//     H_w = sum_e w_e J_e' Omega_e J_e                   (Gauss-Newton, as ml.h's H)
//
// weight_mu and rho_mu are gnc_math.h's gnc_weight_rho, unchanged, applied to s = chi2 (gnc.h writes the formulas out).
//
// The levels, the mu schedule, the outcomes and the invariant (within a level F_mu never increases while the inner solve does
// not increase F_w) are gnc.h's with s = chi2: the same loop runs them (Group::gnc_loop, gnc.cpp).  inner is polish_loop
// (polish.h) on (F_w, g_w, H_w) with fixed weights.
//
// Four differences from gnc.h; the last two are named fields of the objective's description (GncObjective, group.h).
//  1. An inner MAX_STEPS is normal and is not a failure.  H_w is Gauss-Newton: at the early levels the weighted residuals at
//     the minimum are large, and the inner loop converges linearly (ml_polish needs 92 steps on tinyGrid3D).  The level's point
//     is then the last accepted one -- F_w has not increased, which is all the invariant needs.  Only an inner STALLED is
//     INNER_FAILED.  inner_outcome reports the last level's inner outcome; the log has the columns of GNC_LOG_COLS.
//  2. near_pi and weights of exactly zero.  An outlier's rotation residual can sit at theta > pi - 1e-3, where ml_residual's
//     values are not specified further.  An edge whose weight is exactly 0 contributes exact zeros by selection, not by
//     multiplication (ml_gnc_math.h): its two gradient terms, its record and its term of sum_R w chi2 -- 0 * NaN would poison
//     g, H and F_w.  The result's near_pi counts the edges with w_e > 0 at the final point; near_pi_all, every edge.
//     What the selection does NOT cover: rho_mu(chi2_e) and, in a WEIGH pass, w_e itself are still computed from the chi2 of
//     such an edge.  Where that chi2 is finite -- it is at every theta the tests reach, pi - 5e-4 included -- both are what the
//     formulas give for it; were it not, sum_R rho_mu (F_mu: F_surrogate_final and the log's columns 1 and 4) and that edge's
//     weight would not be finite either, while g_w, H_w and F_w of the edges with w > 0 stay untouched.  max_R chi2 drops a
//     NaN (fmax).  near_pi > 0 in the result is the caller's flag for this.
//  3. The pass at a failure writes per-edge output.  chi2 per edge is written by a FULL pass only, and num_outliers is read
//     from it: after an inner STALLED the point handed back (X_{k-1}, or X at level 0) gets a FULL pass.  gnc.h's pass writes
//     s_rot and s_trans whatever its flags, so its failure pass leaves the rows off.
//  4. A level-0 stall is evaluated.  INNER_FAILED at level 0 comes back with F_weighted_final, F_surrogate_final, the counts,
//     num_outliers and near_pi of (X, w = 1) at mu = 1; gnc.h returns without a pass and leaves them zero.
//
// Connectivity: as gnc.h.  A level whose zero weights disconnect the graph makes H_w singular; the Levenberg-Marquardt shift
// either copes or stalls; a stall is INNER_FAILED, an outcome, not an error.
//
// One kernel (ml_gnc.hip), fp64, fixed-order sums (wave_reduce.h), no floating-point atomics, no LDS: the same bits run to run.
//   k_ml_gnc_edge<D, FULL>  one lane per edge in graph order, EDGE_BLOCK per workgroup, records and poses read as 16-byte units
//                as in k_ml_edge; ml_residual<D> and ml_weigh<D> give chi2.  WEIGH: w = weight_mu(chi2) written for e in R (the
//                array is not touched elsewhere); FIXED: w read for e in R; 1 outside R in both.  R-membership is an array of
//                its own, one int per edge (the cached records' inter word is not overwritten: ml_begin compares them).
//                FULL writes r, chi2 (unweighted) and, through ml_gnc_edge_out, wr = w (Omega r), the gradient terms and the
//                record [J_i | J_j | w Omega J_i | w Omega J_j] in ml_jw_doubles layout, so that launch_ml_gather and
//                launch_ml_hessian serve unchanged and H_w inherits k_ml_hessian's bitwise symmetry.  FULL off is the trial
//                point: sums only.  Per workgroup, by wave shuffle (gnc_partials.h, shared with k_gnc_edge), one partial each:
//                sum_{not R} chi2, sum_R w chi2, sum_R rho_mu(chi2), max_R chi2, min_R w; the counts of w == 0, w == 1,
//                0 < w < 1 over R; near_pi over w > 0, and over all edges.
// The final wave is gnc.hip's k_gnc_final<5> (launch_gnc_final): the summary, and optionally F_w into a slot of the
// certificate's partial sums with the rest of the slot zeroed, as k_ml_final does.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "gnc.h"
#include "ml.h"

namespace dpgo {

// GncResult with the ML objective's extras: near_pi over the edges with w > 0 at the final point, near_pi_all over every edge.
// s_max_initial: max_R chi2 at X0; num_outliers: e in R with chi2_e > c2 at the final point.
struct MlGncResult : GncResult {
  long long near_pi = 0, near_pi_all = 0;
};

// What the final pass leaves on the device: GncSummaryDev on chi2, then the two near_pi counts, where k_gnc_final<5> writes its
// counts past the third.
struct MlGncSummaryDev {
  GncSummaryDev gnc;
  long long near_pi, near_pi_all;
};
static_assert(sizeof(MlGncSummaryDev) == 80 && offsetof(MlGncSummaryDev, gnc) == 0 && offsetof(MlGncSummaryDev, near_pi) == 64 &&
                  offsetof(MlGncSummaryDev, near_pi_all) == 72,
              "the two counts follow GncSummaryDev directly");

// device (ml_gnc.hip); enqueued on st.  in_R: m ints; w: m doubles (weigh: written on R, read nowhere; else read on R); out as
// launch_ml_edge (out.r == nullptr: the trial point, nothing per edge is written); partials: 5 nb doubles, counts: 5 nb,
// nb = ceil(m / EDGE_BLOCK); fslot[0] = F_w with fslot[1 .. nslot) zeroed (null: neither)
void launch_ml_gnc_edge(int d, hipStream_t st, int m, const double *rec, const double *omega, const double *X, const int *in_R,
                        int kind, double mu, double c2, bool weigh, double *w, const MlEdgeOut &out, double *partials,
                        long long *counts, MlGncSummaryDev *sum, double *fslot, int nslot);

// Host, debug (no GPU): per edge of g in graph order, given w (num_edges), what a FULL pass writes, through ml_math.h and
// ml_gnc_math.h: r, wr = w (Omega r) (dof), chi2 (unweighted), grad (2 dof: of pose i, of pose j), jw (ml_jw_doubles);
// near_pi over w > 0 and near_pi_all.  Output pointers may be null.  -1: as ml_edge_host, or a w outside [0, 1].
int ml_gnc_edge_host(const Graph &g, const double *X, int ld, const double *w, double *r, double *wr, double *chi2, double *grad,
                     double *jw, long long *near_pi, long long *near_pi_all);

}  // namespace dpgo
