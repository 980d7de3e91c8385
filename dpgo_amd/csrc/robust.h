// The robust objective behind the Newton polish and the covariances: its value, gradient and TRUE Hessian on the device.
//
//     F(X) = 1/2 sum_intra s_e + 1/2 sum_inter rho(s_e),       w_e = rho'(s_e),       c_e = 2 rho''(s_e)
//
// with s_e = tr(X^T M_e X), the residuals, the inter / intra rule and the loss formulas of edges.h (edge_lane, edge_math.h).
// c_e = 0 on intra edges, under the trivial loss and where w_e is exactly 0; Huber: 0 for s <= delta, -w / s above;
// Geman-McClure: -4 w / (s + delta); Welsch: -2 w / delta.  In the tangent coordinates of cov.h (layout, anchor, dof):
//
//     M_w = sum_e w_e M_e,        g = sum_e w_e g_e,     g_e[dof p + a] = tr(E_a(p)^T (M_e X)_p)   (p an endpoint of e)
//     H   = H(S_w) + sum_inter c_e g_e g_e^T,            S_w = M_w - blkdiag(0, Lambda_w(X))
//
// g is the tangent projection of M_w X, so k_cert_lambda and k_polish_grad serve it unchanged; H(.) is what k_cov_hessian
// writes, here from M_w in a buffer of its own and Lambda_w; the rank-one term of an edge touches the blocks (i, i), (i, j),
// (j, i), (j, j) only, so the pattern, the symbolic analysis, the numeric context and the factor are the covariance's.
// curvature = 0 leaves the rank-one terms out: the Hessian of the re-weighted problem (an IRLS-Newton step).
//
// Four kernels (robust.hip), fp64, fixed-order sums, no floating-point atomics: the same bits run to run.
//   k_robust_edge    one lane per edge in graph order, 64 per workgroup: s_rot, s_trans, rho, w through edge_lane (EdgeEval's
//                    bits), c_e, behind a flag the rows (M_e X)_i, (M_e X)_j; F_intra, F_inter by wave shuffle, one partial per
//                    workgroup, one final wave in strided order (k_robust_final)
//   k_robust_gather  one lane per own pose: (M_w X)_p = sum w_e (M_e X)_p over the pose's incidence list, ascending edges
//   k_robust_mval    one wave per pose: M_w in the layout of CertState::Mval, every entry the sum over its block's edge list
//                    (ascending edges; parallel and reversed edges share a block, the diagonal block takes every incident edge)
//   k_robust_rank1   one wave per pose, k_cov_hessian's entry mapping on the factorisation's value array behind it: adds
//                    sum c_e g_e^p[a] g_e^q[b] over the block's edge list; the anchor's rows and columns stay the identity's
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "edges.h"
#include "graph.h"
#include "kernels.h"

namespace dpgo {

// The host's lists of one (group, graph): built once on the group's unified own rows (robust.cpp)
struct RobustPlan {
  int d = 0, N = 0, m = 0, nb = 0;
  std::vector<double> rec;        // edge records (edges.h) with i, j the unified own rows
  std::vector<int> inc_ptr, inc;  // pose -> 2 e + role (0: the edge's i, 1: its j), ascending
  std::vector<int> blk_ptr, blk;  // block of the certificate's pattern -> 4 e + 2 role(row) + role(column), ascending
};

// pl <- the lists of the records rec (heads on unified own rows; moved into the plan) with eb, per edge its blocks (i, i), (i, j),
// (j, i), (j, j) among the pattern's nblk (robust.cpp; the maximum-likelihood objective's plan is built by it too, ml.cpp)
void robust_plan_lists(int d, int N, std::vector<double> &&rec, const std::vector<int> &eb, size_t nblk, RobustPlan &pl);

// device (robust.hip); everything is enqueued on st
// out: 5 arrays of m doubles (s_rot, s_trans, rho, w, c); rows (null: not computed): 2 pose records per edge, (M_e X)_i then
// (M_e X)_j; the summary goes to sum, and F = F_intra + F_inter to fslot[0] with fslot[1 .. nslot) zeroed (null: neither)
void launch_robust_edge(int d, hipStream_t st, int m, const double *rec, const double *X, int loss, double loss_reg, double *out,
                        double *rows, double *partials, long long *counts, EdgeSummaryDev *sum, double *fslot, int nslot);
// MX (own rows) = M_w X from the stored rows
void launch_robust_gather(const LaunchCtx &lc, const int *inc_ptr, const int *inc, const double *w, const double *rows, double *MX);
void launch_robust_mval(int d, hipStream_t st, int nposes, const int *bptr, const int *blk_ptr, const int *blk, const double *rec,
                        const double *w, double *Mw);
void launch_robust_rank1(int d, hipStream_t st, int nposes, const int *bptr, const int *bcol, const int *blk_ptr, const int *blk,
                         const double *c, const double *rows, const double *X, int anchor, double *val);

// Host, debug (no GPU): per edge of g in graph order w, c, the rows (2 pose records per edge) and the tangent gradients
// (2 dof per edge: of pose i, of pose j) through robust_math.h.  Output pointers may be null.
int robust_edge_host(const Graph &g, const double *X, int ld, int loss, double loss_reg, double *w, double *c, double *rows,
                     double *ghat);

}  // namespace dpgo
