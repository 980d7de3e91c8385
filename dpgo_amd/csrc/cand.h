// Joint compatibility and budgeted selection of loop-closure candidates.
//
// pairs.h gates ONE candidate at a time: d^2 = r^T (Sigma_rel + Omega^-1)^-1 r ignores every other candidate.  Here m
// candidates (pairs[m][2], p != q; a pair may repeat, pairs may share poses, either end may be the anchor) are judged
// TOGETHER, in pairs.h's perturbation and sign conventions (pairs_math.h):
//
//  * K: the distinct end poses in order of first appearance (p_0, q_0, p_1, ...); n = dof m.  Row block i of J holds
//    A_i = J_p(p_i, q_i) on p_i's columns and B_i = J_q(p_i, q_i) on q_i's.
//  * cov = J Sigma_KK J^T (n x n): the joint covariance of the candidates' predicted relative poses.  Sigma_KK comes from
//    marg.h's batch loop (Group::marg_sigma); the anchor's blocks are zeros.  Its diagonal blocks are pairs.h's `rel`.
//  * r stacks pairs.h's residuals; S = cov + blkdiag(Omega_i^-1), Omega_i = blkdiag(tau_i I_d, 2 kappa_i I_{dof - d}).
//  * the joint test (want_joint): Sinv = S^-1 and logdet_S by marg.h's dense factor of order n, d2_joint = r^T Sinv r,
//    gain_all = 1/2 (logdet_S - sum_i log det Omega_i^-1) -- the information all candidates would add together.
//  * the selection (budget > 0): greedy by conditional information gain, a left-looking block-pivoted Cholesky of S that
//    leaves S intact.  C_i (dof x dof) is candidate i's innovation covariance given the candidates already chosen, rho_i its
//    conditional residual; gain_i = 1/2 (log det C_i - log det Omega_i^-1), d2_i = rho_i^T C_i^-1 rho_i.  A candidate is
//    eligible iff C_i is positive definite and (d2_max <= 0 or d2_i <= d2_max) -- the gate acts on the CONDITIONAL d2.  The
//    eligible candidate of the largest gain is chosen; ties go to the lowest index.  Each step is two launches (k_cand_score,
//    k_cand_update) with the chosen index in device memory: no host round trip between steps; a step without an eligible
//    candidate raises a device flag that turns every later step into a no-op.
//    By the Cholesky identity sum gain = 1/2 (log det S_sel - log det R_sel) of the chosen principal submatrix
//    (R = blkdiag(Omega^-1)) and sum d2 = r_sel^T S_sel^-1 r_sel.
//
// The restrictions are cov.h's: the trivial loss, a group that hosts every node; X should be a critical point.  The
// optimiser's state is not touched.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "hess.h"
#include "marg.h"

namespace dpgo {

enum { CAND_OK = 0, CAND_NOT_PD = 1, CAND_SKIPPED = 2 };

// n, poses (|K|), columns, batches and device_bytes come from the analyses and the plan and are filled for SKIPPED too;
// device_bytes: the numeric phase of H, spd_msolve_bytes, this call's buffers (the batch block, Sigma_KK, cov, S, P, C, rho, the
// lists) and, with want_joint, the dense factor's bytes.  joint_not_pd: the dense factorisation of S met a non-positive pivot --
// info, logdet, d2_joint and gain_all are zeros, the selection still ran.  solve_ms: the batches and k_cand_innov up to a
// synchronise; dense_ms: the dense factorisation, its inversion, k_cand_quad and the copies; select_ms: the selection's launches
// and its one read-back.
struct CandResult : HessAnalysis {
  int outcome = CAND_SKIPPED, n = 0, poses = 0, columns = 0, batches = 0, n_selected = 0, joint_not_pd = 0;
  double dense_pivot_min = 0, dense_pivot_max = 0, stationarity = 0, solve_ms = 0, dense_ms = 0, select_ms = 0;
};

// What the call returns (host arrays of the caller; cov and S may be null).  scalars[5]: logdet_S, d2_joint, gain_all,
// gain_selected, d2_selected.  selected[budget] (-1 past n_selected), steps[budget][4]: index, gain, d2, the number of eligible
// candidates at that step (zeros past n_selected).  poses[2 m]: K in its order, the first result.poses entries.
struct CandOut {
  double *cov = nullptr, *S = nullptr, *residual = nullptr, *info = nullptr, *scalars = nullptr, *steps = nullptr;
  int *selected = nullptr, *poses = nullptr;
};

// K and the positions of every pair's ends in it (host): kpos[2 i], kpos[2 i + 1]
void cand_pose_list(const int *pairs, int m, std::vector<int> &K, std::vector<int> &kpos);

// The selection's device state: cur (the index chosen by the step under way, -1: none), done (raised by the first step without an
// eligible candidate), nsel, and per candidate whether it has been taken.
struct CandSelectBufs {
  int *state;       // [0] cur, [1] done, [2] nsel
  int *taken;       // m
  int *selected;    // budget
  double *steps;    // budget x 4
  double *sums;     // gain_selected, d2_selected
  double *piv;      // dof^2 (L_ss) + dof (z_s)
  double *P;        // n x dof budget, entry (a, c) at P[c n + a]: consecutive lanes read consecutive addresses
  double *C;        // m x dof^2
  double *rho;      // n
};

// ---- kernels (cand.hip) ----
// cov (optional), S and (optional) S2 from Sigma_KK (ld = dof |K|): one lane per block (i, j), i >= j.  prow[k]: the record of
// K[k] in X; kpos as above; winv[2 i], winv[2 i + 1]: 1 / tau_i, 1 / (2 kappa_i)
void launch_cand_innov(int d, hipStream_t st, int m, int nK, const int *prow, const int *kpos, const double *X, const double *sig,
                       const double *winv, double *cov, double *S, double *S2);
// r (dof m) and winv (2 m) of the candidates (m x (d^2 + d + 2))
void launch_cand_resid(int d, hipStream_t st, int m, const int *prow, const int *kpos, const double *X, const double *cand, double *r,
                       double *winv);
// *out <- r^T Sinv r, one workgroup, a fixed-order tree
void launch_cand_quad(hipStream_t st, int n, const double *Sinv, const double *r, double *out);
// C_i <- S_ii, rho <- r, the state cleared (selected and steps are the caller's to initialise)
void launch_cand_select_init(int d, hipStream_t st, int m, const double *S, const double *r, CandSelectBufs b);
// one step: score, then update (both no-ops behind the done flag)
void launch_cand_score(int d, hipStream_t st, int m, int t, double d2_max, const double *winv, CandSelectBufs b);
void launch_cand_update(int d, hipStream_t st, int m, int t, const double *S, CandSelectBufs b);

// The whole selection on device arrays S (n x n), r, winv: the buffers, the loop of 2 min(budget, m) - 1 launches, one read-back.
// selected / steps (host, budget entries) are uploaded as they are and come back with the chosen steps written: entries from
// n_selected on keep what the caller put there.  sums[2]: gain_selected, d2_selected.  Bytes it allocates: cand_select_bytes.
int cand_select_run(int d, hipStream_t st, int m, int budget, double d2_max, const double *d_S, const double *d_r, const double *d_winv,
                    int *selected, double *steps, double *sums, int *n_selected);
long long cand_select_bytes(int dof, int m, int budget);

// ---- test hooks (capi_debug.cpp), on the caller's host arrays ----
// cand_math.h on the host / the kernels on the current device.  X: nK records; sigma: (dof nK)^2; kpos: 2 m positions in the
// list; cand: m x (d^2 + d + 2); cov, S: (dof m)^2; r: dof m
int cand_innov_host(int d, int m, int nK, const int *kpos, const double *X, const double *sigma, const double *cand, double *cov,
                    double *S, double *r);
int cand_innov_device(int d, int m, int nK, const int *kpos, const double *X, const double *sigma, const double *cand, double *cov,
                      double *S, double *r);
// the selection on a GIVEN S (n x n), r, weights (m x 2: kappa, tau), no graph; selected / steps in and out as cand_select_run's
int cand_select_host(int d, int m, int budget, double d2_max, const double *S, const double *r, const double *weights, int *selected,
                     double *steps, double *sums, int *n_selected);
int cand_select_device(int d, int m, int budget, double d2_max, const double *S, const double *r, const double *weights, int *selected,
                       double *steps, double *sums, int *n_selected);

}  // namespace dpgo
