// Measurement sensitivities of the ROBUST objective: sens.h at a critical point of
//     F(X; theta, delta) = 1/2 sum_intra s_e + 1/2 sum_inter rho(s_e; delta)          (robust.h: w_e, c_e, g, the TRUE Hessian H)
// with the loss threshold delta one more parameter.  The adjoint is lambda = H^-1 c on the true robust Hessian (curvature 1,
// anchored as in cov.h), and with phi_e = lambda_i^T ghat_e(i) + lambda_j^T ghat_e(j) of sens.h
//     dL/dtheta_e = -[ w_e d phi_e / d theta_e + (c_e / 2) phi_e d s_e / d theta_e ],        dL/ddelta = -sum_inter (d w_e / d delta) phi_e
// (rsens_math.h: d s / d theta, d w / d delta, the combination).  One robust edge pass, one factorisation, one per-edge
// preparation pass, ceil(k / 64) block solves and one per-edge kernel for k upstream gradients.
//
//  * upstream, adjoint: as sens.h.
//  * sens: k x num_edges x (3 + dof): d L_l / d (kappa, tau, t~[0..d), eta[0..dof - d)) and, last, the edge's term of d L_l / d delta.
//  * dloss_reg: k doubles, d L_l / d delta: the last entries summed over the edges in ascending order on the host.
//  * Intra edges (w = 1, c = 0) carry sens.h's values; where w_e is exactly 0 every entry of the edge is an exact zero; under
//    the trivial loss everything equals sens.h's in value and the delta terms are 0.
//  * A column's bits do not depend on k, on its position or on its companions, as in sens.h.
//
// The robust set is the inter-node edges of the graph, the group a trivial-loss group that hosts every node (robust.h).  H can
// honestly fail to be positive definite under Geman-McClure and Welsch: SENS_NOT_PD, zero outputs.
#pragma once
#include <hip/hip_runtime.h>

#include "sens.h"

namespace dpgo {

// ---- kernels (rsens.hip) ----
// prep (m x (3 + dof)): per edge d s / d (kappa, tau, t~, eta) and d w / d delta; rec: the edge records on unified own rows,
// X: the pose records, eo: k_robust_edge's five arrays of m doubles (s_rot, s_trans, rho, w, c)
void launch_rsens_prep(int d, hipStream_t st, int m, const double *rec, const double *X, const double *eo, int loss, double loss_reg,
                       double *prep);
// out (nc x m x (3 + dof)): sens_one of every (edge, column j < nc) combined with the edge's w, c and prep
void launch_rsens_edge(int d, hipStream_t st, int m, const double *rec, const double *X, const double *eo, const double *prep,
                       const double *Xb, int ldx, int nc, double *out);

// host only: the arithmetic of both kernels for every edge of g at X (global (d+1)N x d) with one adjoint lambda (dof N by
// global pose); sens: num_edges x (3 + dof), phi (optional): num_edges
int robust_sens_edge_host(const Graph &g, const double *X, int ld, int loss, double loss_reg, const double *lambda, double *sens,
                          double *phi);

}  // namespace dpgo
