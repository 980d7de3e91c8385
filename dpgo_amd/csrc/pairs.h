// Joint covariances of arbitrary pose pairs and loop-closure gating.
//
// cov.h hands out the blocks of H^-1 inside the factor's pattern: every marginal, and the cross block of an EDGE.  Here the
// pair (p, q) is any two poses: with the factor of the same anchored tangent-space Hessian (cov.h: the unknowns, the gauge,
// k_cov_hessian) the columns of H^-1 that belong to the poses asked for are solved for,
//     H^-1 [e_p-columns, e_q-columns]    (spd.h: spd_msolve_device, batches of at most 64 columns),
// and read at the rows of p and q.  No block of the selected inversion is stored, so the refusal counts the numeric phase,
// the solve and this file's own buffers only: the call may run where Group::covariance answers COV_SKIPPED.
//
//  * joint: per pair three dof x dof blocks, row-major: S_pp, S_pq, S_qq.  S_pq has the ROWS of p and the COLUMNS of q,
//    S_pq[a][b] = cov(x_p[a], x_q[b]), as Group::covariance's `cross`.  Every entry is read from ONE solved column -- S_pp from
//    p's columns, S_pq and S_qq from q's -- so a pair's bits do not depend on the other pairs of the call (spd.h: a column's
//    bits do not depend on its companions).  Blocks that involve the anchor are exact zeros; p == q gives S_pq = S_pp = S_qq.
//  * rel: the covariance of the relative pose T_pq = T_p^-1 T_q, dof x dof, in the perturbation of cov.h carried over to
//    T_pq: t_pq + dt_pq, R_pq Exp(hat(domega_pq)).  To first order (pairs_math.h: J)
//        domega_pq = omega_q - R_pq^T omega_p,    dt_pq = R_p^T (dt_q - dt_p) + hat(t_pq) omega_p
//    (d = 2: the last term is -omega_p [[0, -1], [1, 0]] t_pq), and rel = J Sigma_joint J^T.
//  * gate, where a candidate measurement (R~, t~, kappa, tau) of the pair is given: the residual
//    r = [t_pq - t~ ; vee Log(R~^T R_pq)], the innovation covariance S = rel + Omega^-1 with
//    Omega = blkdiag(tau I_d, 2 kappa I_{dof - d}) -- the Hessian of that edge's own term of
//    F = 1/2 sum (kappa |.|_F^2 + tau |.|^2) at zero residual -- and d^2 = r^T S^-1 r by a Cholesky in registers.  No
//    threshold is applied: the caller compares d^2 with the chi-square quantile of its choice.
//
// The restrictions are cov.h's: the trivial loss, a group that hosts every node.  The optimiser's state is not touched.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "hess.h"

namespace dpgo {

enum { PAIRS_OK = 0, PAIRS_NOT_PD = 1, PAIRS_SKIPPED = 2 };

constexpr int PAIRS_BATCH = 64;   // columns per spd_msolve_device call

// unknowns ... device_bytes come from the symbolic analysis and the column plan and are filled for SKIPPED too; device_bytes:
// the numeric phase with its W / WT panels, spd_msolve_bytes, the block-column map and this call's buffers.  columns: solved
// unit columns (dof per distinct non-anchor pose), batches: spd_msolve_device calls.  factor_ms: k_cov_hessian and the
// factorisation up to its verdict; solve_ms: the batches (right-hand sides, solves, gathers) up to a synchronise; gate_ms:
// k_pairs_gate and the copies to the host.
struct PairsResult : HessAnalysis {
  int outcome = PAIRS_SKIPPED, columns = 0, batches = 0;
  double stationarity = 0, solve_ms = 0, gate_ms = 0;
  // what the batches cost by count: the useful flops of the two sweeps, sum over the fronts of 4 (w + u) w times the columns of
  // every batch rounded up to 16, and the factor bytes they stream, 16 sum (w + u) w per batch (W forward, WT backward)
  double solve_flops = 0, factor_bytes = 0;
};

// The column plan (host): the distinct poses among the pairs other than the anchor, ascending; pose i of that list owns the
// columns dof i ... dof i + dof - 1, batch b the columns 64 b ... 64 b + 63 -- a pose's columns may straddle two batches.
// pair_col[2 k], pair_col[2 k + 1]: the first column of pair k's p and q, -1 for the anchor.
struct PairsPlan {
  std::vector<int> poses, pair_col;
  int columns = 0, batches = 0, kb = 0;   // kb: the row length of the batch array, 16 ceil(min(columns, 64) / 16)
};
PairsPlan pairs_plan(int dof, int anchor, const int *pairs, int npairs);
// the batches and the batch array's row length of a plan with that many columns (marg.h's plan shares it)
inline void pairs_plan_sizes(int columns, int *batches, int *kb) {
  *batches = (columns + PAIRS_BATCH - 1) / PAIRS_BATCH;
  const int widest = columns < 1 ? 1 : columns < PAIRS_BATCH ? columns : PAIRS_BATCH;
  *kb = 16 * ((widest + 15) / 16);
}

// ---- kernels (pairs.hip) ----
// Xb (n x ldx, zeroed by the caller): column j < nc <- the unit vector of unknown col_unknown[c0 + j]
void launch_pairs_rhs(hipStream_t st, const int *col_unknown, int c0, int nc, double *Xb, int ldx);
// joint <- the entries whose column lies in [c0, c0 + nc): prow[2 k], prow[2 k + 1] the unified own rows of pair k's poses,
// pcol likewise their first columns (-1: the anchor)
void launch_pairs_gather(hipStream_t st, int dof, int npairs, const int *prow, const int *pcol, int c0, int nc, const double *Xb,
                         int ldx, double *joint);
// rel (npairs x dof^2) and, with cand (npairs x (d^2 + d + 2)), gate (npairs x (2 + dof): d^2, not_pd, residual)
void launch_pairs_gate(int d, hipStream_t st, int npairs, const int *prow, const double *joint, const double *X, const double *cand,
                       double *rel, double *gate);

}  // namespace dpgo
