// Maximum-likelihood refinement on the measurements' full information matrices, with its covariances.
//
// The optimiser, the polish and the covariances live in the isotropic chordal model: the loader reduces every Omega_e to
// kappa_e, tau_e.  g2o, GTSAM and Ceres minimise 1/2 sum r' Omega r with the file's Omega and hand out (J' Omega J)^-1.  Here,
// for an edge e = (i -> j) with measurement (R~, t~) and information Omega_e (dof x dof, dof = d + d (d - 1) / 2, translation
// first, then rotation, as the file orders them):
//
//     r_t = R~^T (R_i^T (t_j - t_i) - t~)
//     r_R = Log(R~^T R_i^T R_j)                 (rotation vector; d = 2: the angle, wrapped to (-pi, pi])
//     F_ml(X) = 1/2 sum_e r_e' Omega_e r_e,     chi2_e = r_e' Omega_e r_e
//
// The unknowns are cov.h's -- t_p + dt in the world frame, R_p <- R_p Exp(hat(omega)) in the body frame -- with the same anchor
// convention: identity block, zero off-diagonal blocks, zeros returned.  g = sum_e J_e' Omega_e r_e with the exact Jacobians of
// r (ml_math.h).  The Hessian is the GAUSS-NEWTON one, H = sum_e J_e' Omega_e J_e: the Fisher information, the matrix g2o and
// GTSAM factor and invert.  The second-order term is left out on purpose.  H is positive semidefinite by construction, so
// NOT_PD here means a rank-deficient graph (or rounding at the edge of one), never a saddle.
//
// A graph without Omega (graph.h) uses Omega_iso = diag(tau I_d, 2 kappa I), for which F_ml and the project's F agree to second
// order in the residual.  Edges with theta > pi - 1e-3 are counted (near_pi); their values are not specified further.
//
// Three kernels and a final pass (ml.hip), fp64, fixed-order sums, no floating-point atomics: the same bits run to run.
//   k_ml_edge     one lane per edge in graph order, 64 per workgroup: F_ml by wave shuffle, one partial per workgroup, one
//                 final wave in strided order (k_ml_final), near_pi beside it; behind a flag r, Omega r, chi2, the edge's
//                 gradient terms J_i' Omega r, J_j' Omega r and its record [J_i | J_j | Omega J_i | Omega J_j], so that the
//                 two kernels below recompute nothing with other rounding.  The flag off is the trial point's evaluation.
//   k_ml_gather   one lane per own pose: g_p = the sum of its incidence list's terms, ascending edges; |g|^2 into the polish's
//                 partial slot; zeros on the anchor's row
//   k_ml_hessian  one wave per pose, k_cov_hessian's entry mapping on the factorisation's value array: every entry the sum
//                 over its block's edge list (ascending edges; parallel and reversed edges share a block, the diagonal block
//                 takes every incident edge) of ml_block_entry; the anchor's rows and columns are the identity's
// The lists are RobustPlan's (robust.h: robust_plan_lists), built once per (group, graph).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "graph.h"
#include "kernels.h"
#include "polish.h"
#include "robust.h"

namespace dpgo {

// PolishResult with the ML objective's extras: chi2_total = 2 F_ml at both ends, near_pi at the final point
struct MlResult : PolishResult {
  long long near_pi = 0;
  double chi2_initial = 0, chi2_final = 0;
};

// what the final pass leaves on the device
struct MlSummaryDev {
  double F;
  long long near_pi;
};

// doubles per edge of the stored record [J_i | J_j | Omega J_i | Omega J_j]
constexpr int ml_jw_doubles(int d) { return 4 * graph_dof(d) * graph_dof(d); }

// The arrays an edge pass writes (device): r, wr: m x dof; chi2: m; g: 2 m x dof (edge e's term of pose i at 2 e, of pose j at
// 2 e + 1); jw: m x ml_jw_doubles.  r == nullptr: none of them is written (the trial point).
struct MlEdgeOut {
  double *r = nullptr, *wr = nullptr, *chi2 = nullptr, *g = nullptr, *jw = nullptr;
};

// device (ml.hip); everything is enqueued on st.  partials: nb doubles, counts: nb, nb = ceil(m / 64); F_ml goes to sum and to
// fslot[0] with fslot[1 .. nslot) zeroed (null: not)
void launch_ml_edge(int d, hipStream_t st, int m, const double *rec, const double *omega, const double *X, const MlEdgeOut &out,
                    double *partials, long long *counts, MlSummaryDev *sum, double *fslot, int nslot);
// g (dof per own row) from the edges' terms; slot_g2: |g|^2 per segment into the polish's partials
void launch_ml_gather(const LaunchCtx &lc, const int *inc_ptr, const int *inc, const double *ge, int anchor, double *g, int slot_g2,
                      double *partials);
void launch_ml_hessian(int d, hipStream_t st, int nposes, const int *bptr, const int *bcol, const int *blk_ptr, const int *blk,
                       const double *jw, int anchor, double *val);

// Host (no GPU): Omega_e of every edge checked symmetric positive definite; -1 with the edge named otherwise
int ml_check_information(int d, const std::vector<double> &omega, const char *who);
// Host, debug (no GPU): per edge of g in graph order r, wr (dof), chi2, Ji, Jj (dof^2), grad (2 dof: of pose i, of pose j) and
// blocks (4 dof^2: (i, i), (i, j), (j, i), (j, j)) through ml_math.h; near_pi: the count.  Output pointers may be null.
int ml_edge_host(const Graph &g, const double *X, int ld, double *r, double *wr, double *chi2, double *Ji, double *Jj, double *grad,
                 double *blocks, long long *near_pi);

}  // namespace dpgo
