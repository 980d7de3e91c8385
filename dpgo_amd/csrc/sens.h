// Measurement sensitivities: how does the solution depend on the measurements it was computed from?
//
// At a critical point X* of F(X; theta) the implicit function theorem gives dX*/dtheta = -H^-1 d_theta g, with g the tangent
// gradient and H the anchored tangent-space Hessian of cov.h (the unknowns, the gauge, k_cov_hessian).  For a scalar L(X*) whose
// tangent gradient at X* is c (dof N numbers by global pose, cov.h's coordinates; the anchor's are ignored) the adjoint
//     lambda = H^-1 c        (zeros on the anchor; spd.h: spd_msolve_device, batches of at most 64 columns)
// turns that into dL/dtheta = -lambda^T d_theta g.  g is a sum over the edges and an edge's parameters theta_e = (kappa, tau, t~, R~)
// enter its own term only, so with phi_e(lambda; theta_e) = lambda_i^T ghat_e(i) + lambda_j^T ghat_e(j) = D_lambda (1/2 s_e)
//     dL/dtheta_e = -d phi_e / d theta_e       (sens_math.h: the perturbations and the closed forms)
// for every edge at once: one factorisation, ceil(k / 64) block solves and one per-edge kernel for k upstream gradients.
//
//  * upstream: (dof N) x k column-major by global pose.  adjoint (optional): lambda in the same layout.
//  * sens: k x num_edges x (2 + dof), edges in the order of the graph argument: d L_l / d (kappa, tau, t~[0..d), eta[0..dof - d))
//    with R~ <- R~ Exp(hat(eta)), the hat of cov.h.
//  * A column's bits do not depend on k, on its position or on its companions (spd.h guarantees it for the solve; k_sens_edge
//    runs the same arithmetic for every (edge, column)).
//
// The restrictions are cov.h's: the trivial loss, a group that hosts every node.  X should be a critical point: `stationarity`
// says whether it is, nothing is enforced.  The optimiser's state is not touched.
#pragma once
#include <hip/hip_runtime.h>

#include "hess.h"

namespace dpgo {

struct Graph;

enum { SENS_OK = 0, SENS_NOT_PD = 1, SENS_SKIPPED = 2 };

constexpr int SENS_BATCH = 64;   // columns per spd_msolve_device call

// unknowns ... device_bytes come from the symbolic analysis and the sizes of the call and are filled for SKIPPED too;
// device_bytes: the numeric phase with its W / WT panels, spd_msolve_bytes, the block-column map and this call's buffers (the
// batch, one batch of upstream, one batch of per-edge output, the edge records, the row lists).  columns: k, batches:
// spd_msolve_device calls, edges: of the graph.  factor_ms: k_cov_hessian and the factorisation up to its verdict; solve_ms:
// the uploads, right-hand sides, solves and adjoint read-outs of all batches; edge_ms: k_sens_edge and the copies of its output.
struct SensResult : HessAnalysis {
  int outcome = SENS_SKIPPED, columns = 0, batches = 0, edges = 0;
  double stationarity = 0, solve_ms = 0, edge_ms = 0;
};

// ---- kernels (sens.hip) ----
// Xb (n x ldx row-major, zeroed by the caller): column j < nc <- column j of U (n x nc column-major by global pose), the
// coordinates of global pose p at the rows dof row_of[p] ...; the anchor's (global pose) stay zero
void launch_sens_rhs(hipStream_t st, int dof, int nposes, const int *row_of, int anchor, const double *U, int nc, double *Xb, int ldx);
// A (n x nc column-major by global pose) <- the solved columns of Xb, gid[row] the global pose of a unified own row; exact
// zeros on the anchor
void launch_sens_adjoint(hipStream_t st, int dof, int nposes, const int *gid, int anchor, const double *Xb, int ldx, int nc, double *A);
// out (nc x m x (2 + dof)): sens_one of every (edge, column j < nc); rec: the edge records on unified own rows, X: the pose records
void launch_sens_edge(int d, hipStream_t st, int m, const double *rec, const double *X, const double *Xb, int ldx, int nc, double *out);

// host only: sens_one of every edge of g at X (global (d+1)N x d) with one adjoint lambda (dof N by global pose);
// sens: num_edges x (2 + dof), phi (optional): num_edges
int sens_edge_host(const Graph &g, const double *X, int ld, const double *lambda, double *sens, double *phi);

}  // namespace dpgo
