// Joint marginals of a pose set: covariance and information.
//
// cov.h hands out the marginal of every pose, pairs.h the joint covariance of any TWO.  Here `keep` is a list of K distinct
// global poses, and the answer is the dense Gaussian over all of them together -- the summary one robot hands to another, the
// prior a sliding window keeps when it drops the interior.  With the factor of the same anchored tangent-space Hessian
// (cov.h: the unknowns, the perturbation, the gauge) the columns of H^-1 of the kept poses are solved for in pairs.h's
// batches and read at the kept rows: Sigma_KK = (H^-1)_KK, in the order of the LIST.
//
//  * the absolute form (base < 0): n = dof K, cov = Sigma_KK with the anchor held fixed.  The anchor may not be kept: its
//    block is exactly zero and no information form exists.
//  * the relative form (base a member of keep, K >= 2): n = dof (K - 1), cov = J Sigma_KK J^T, the joint covariance of the
//    relative poses T_base^-1 T_k of the other kept poses in list order, in pairs.h's perturbation of T_pq.  Row block k of J
//    holds pairs_math.h's J_p on the base's columns and J_q on k's (marg_math.h).  The anchor may be anywhere -- kept, or the
//    base itself: its blocks of Sigma_KK are cov.h's zeros.  To first order this covariance does not depend on the anchor at
//    a critical point.
//  * info = cov^-1 (want_info): in the absolute form the Schur complement of the anchored H onto the kept poses.  A dense
//    pattern is ONE front of the multifrontal factorisation (spd.cpp: dissect_connected cannot cut a clique), and for a root
//    front spd_selinv_device returns W_top^T W_top = A^-1: a second SpdFactor on the dense pattern of order n is factored and
//    inverted by the kernels that factor H; no dense Cholesky of its own.  logdet = log det cov = -2 sum log W_top[ii] comes
//    from the same factor; without want_info neither is computed (logdet = 0).
//
// Every entry (i, j), i >= j, of Sigma_KK is read from ONE solved column, j, at row i and written to both (i, j) and (j, i): a
// block's bits do not depend on the other members of keep, cov is symmetric bit for bit, and its lower entries are
// pair_covariance's.  The restrictions are cov.h's: the trivial loss, a group that hosts every node.  The optimiser's state is
// not touched.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <memory>
#include <vector>

#include "hess.h"
#include "spd.h"

namespace dpgo {

enum { MARG_OK = 0, MARG_NOT_PD = 1, MARG_SKIPPED = 2 };

// unknowns ... device_bytes, n, columns, batches come from the symbolic analyses and the column plan and are filled for SKIPPED
// too; device_bytes: the numeric phase of H, spd_msolve_bytes, this call's buffers (the batch block, Sigma_KK, cov, the lists)
// and, with want_info, spd_numeric_bytes + spd_selinv_bytes of the dense factor.  info_not_pd: the dense factorisation of cov
// met a non-positive pivot -- cov is delivered, info and logdet are zeros.  dense_pivot_min / max: of that factorisation.
// factor_ms: k_cov_hessian and the factorisation of H; solve_ms: the batches (and k_marg_rel) up to a synchronise; dense_ms: the
// dense factorisation, its inversion, the log-determinant and the copies to the host.
struct MargResult : HessAnalysis {
  int outcome = MARG_SKIPPED, info_not_pd = 0, n = 0, columns = 0, batches = 0;
  double dense_pivot_min = 0, dense_pivot_max = 0, stationarity = 0, solve_ms = 0, dense_ms = 0;
};

// The column plan (host): pairs.h's rule on a list.  The kept poses other than the anchor, in LIST order, own dof consecutive
// columns each; col[i]: the first column of keep[i], -1 for the anchor.  Batches of 64 as pairs_plan_sizes states them.
struct MargPlan {
  std::vector<int> poses, col;
  int columns = 0, batches = 0, kb = 0;
};
MargPlan marg_plan(int dof, int anchor, const int *keep, int K);

// The dense factor of order n (one front, w = n, u = 0) and what its refusal counts, cached per n: a second call with the same
// n does no symbolic work.  The numeric context is set up by the first call that is not refused.
struct MargDense {
  CsrMatrix A;   // the dense pattern: CSR order == the row-major matrix
  SpdFactor F;
  long long bytes = 0;   // spd_numeric_bytes + spd_selinv_bytes
  ~MargDense();
};
struct MargCache {
  std::map<int, std::unique_ptr<MargDense>> by_n;
  MargDense *get(int n);   // the symbolic analysis on first use; null (and a line on stderr) where it is not one front
};
int marg_dense_prepare(MargDense &D);   // the numeric context (allocates), 0 / -1
// Behind values written into spd_numeric_values(D.F): factor, invert, un-permute into d_info (n x n, device) and the
// log-determinant into d_logdet (device, one double); enqueued on st behind the verdict.  0: done, 1: a non-positive pivot
// (nothing written), -1: error.  pivots[2] <- the pivot range.
int marg_dense_invert(MargDense &D, hipStream_t st, double *d_info, double *d_logdet, double *pivots);

// ---- kernels (marg.hip) ----
// Sigma_KK's entries (i, j), i >= j, whose column lies in [c0, c0 + nc): ns its order, row_unk[i] the unknown of H behind row i,
// col_of[j] the plan's column of j (-1: the anchor, whose zeros the caller wrote); both copies into dst and (optional) dst2
void launch_marg_gather(hipStream_t st, int ns, const int *row_unk, const int *col_of, int c0, int nc, const double *Xb, int ldx,
                        double *dst, double *dst2);
// the relative covariance (dof (K - 1) square) from Sigma_KK (dof K square, list order): b the base's position in the list,
// prow[i] the record of keep[i] in X ((d + 1) d doubles each); into C and (optional) C2
void launch_marg_rel(int d, hipStream_t st, int K, int b, const int *prow, const double *X, const double *sig, double *C, double *C2);
// info[piv[a]][piv[b]] <- S[a][b]
void launch_marg_scatter(hipStream_t st, int n, const int *piv, const double *S, double *info);
// *out <- -2 sum_i log W[i ldw + i], one workgroup, a fixed-order tree
void launch_marg_logdet(hipStream_t st, int n, const double *W, int ldw, double *out);

// ---- test hooks (capi_debug.cpp), on the caller's host arrays ----
// marg_math.h on the host / k_marg_rel on the current device: X: K records, sig: (dof K)^2, cov: (dof (K - 1))^2
int marg_rel_host(int d, int K, int b, const double *X, const double *sig, double *cov);
int marg_rel_device(int d, int K, int b, const double *X, const double *sig, double *cov);
// gather (in batches of 64 columns, as the call's), factor, invert and logdet of a GIVEN dense symmetric matrix of order n, no
// graph: cov <- the gathered copy; out: n, info_not_pd, the dense pivots, the dense factor's bytes, dense_ms
int marg_dense_device(int n, const double *A, double *cov, double *info, double *logdet, MargResult &out);

}  // namespace dpgo
