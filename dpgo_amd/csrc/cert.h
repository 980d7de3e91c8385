// Solution certification: is the point X the optimiser stopped at the global minimum of the trivial-loss problem?
//
// The reference answers this in its SE-Sync tree: SESyncProblem::compute_Lambda_blocks / verify_solution
// (C++/SESync/src/SESyncProblem.cpp:375-468) build the certificate matrix S = M - Lambda(X), and fast_verification
// (C++/SESync/src/SESync_utils.cpp:721-830) looks for its smallest eigenvalue with LOBPCG
// (C++/Optimization/include/Optimization/LinearAlgebra/LOBPCG.h:131-337).  Here:
//
//  * X is (d+1)N x d, column-major, rows 0..N-1 the translations, rows N + d p + r the rows of Y_p = R_p^T
//    (C++/DPGO/include/DPGO/DPGOProblem.h:167-171); M is the global data matrix of the trivial loss
//    (construct_data_matrix, C++/DPGO/src/DPGO_utils.cpp:440-718; F = 1/2 tr(X^T M X)).
//  * Lambda_p = 1/2 (P + P^T), P = (M X)[rows of Y_p] (X[rows of Y_p])^T (SESyncProblem.cpp:375-395 with Y = X^T), and
//    S = M - blkdiag(0_N, Lambda_0, ..., Lambda_{N-1}) (:444-447, the translation-explicit form).  On a record array V
//    (one (d+1) x d record per pose): (S V)_p.x = (M V)_p.x, (S V)_p.Y = (M V)_p.Y - Lambda_p V_p.Y.
//  * |S X|_F is the norm of the Riemannian gradient: the certificate only means something at a critical point, so the
//    result carries it as `stationarity`.
//  * The search is LOBPCG on S with block size d, basis [V W P] (LOBPCG.h:131-337; fast_verification STEP 2,
//    SESync_utils.cpp:765-826): |S| is estimated as |S Omega|_F / |Omega|_F on a Gaussian block (LOBPCG.h:199-214),
//    column 0 counts as converged when r_0 <= tau (|S|_est + |theta_0|) |x_0| (:298-307), and with stop_on_negative
//    the search ends at once when theta_0 < -eta / 2 (SESync_utils.cpp:775-793).
//  * theta and residual of the result are recomputed from ONE fresh product S x of the returned unit vector x
//    (theta = x^T S x, residual = |S x - theta x|), and the status is decided from those two numbers:
//      NEGATIVE     theta < -eta / 2: x proves lambda_min(S) < -eta / 2;
//      NONNEGATIVE  otherwise, and residual <= tau (|S|_est + |theta|): column 0 converged.  EVIDENCE, NOT PROOF: a
//                   converged Ritz pair need not be the smallest one (the proof is STEP 1 below);
//      UNDECIDED    max_iters reached without either.
//  * The proof is fast_verification STEP 1 (SESync_utils.cpp:731-754): a Cholesky factorisation of S + eta I, which
//    exists exactly when the matrix is positive definite.  Group::cert_factor writes S + eta I on the device
//    (k_cert_matrix, cert.hip) as a CSR matrix on pose-major unknowns (d+1) p + r -- r = 0 the translation, r = 1..d
//    the rows of Y_p; S acts alike on every column, so the matrix is (d+1)N x (d+1)N -- with one explicit dense
//    (d+1) x (d+1) block per pair of poses M couples, straight into the value array of the multifrontal
//    factorisation (spd.h: spd_symbolic on the quotient graph of the poses, spd_prepare_device, spd_refactor_device in
//    factor-only mode), and reads the verdict: FACTOR_PD, FACTOR_NOT_PD (a non-positive pivot: an answer, not an
//    error), or FACTOR_SKIPPED when the symbolic analysis predicts more device memory than the caller or the device
//    allows.  Group::verify is fast_verification itself: STEP 1, and the LOBPCG search only when it did not succeed.
//    PROVEN is a statement in floating point, as in the reference: the factorisation succeeds for S + eta I + E with
//    |E| of the order n^(3/2) u |S| (Higham, Accuracy and Stability of Numerical Algorithms, thm 10.7), and it says
//    "global minimum" only where `stationarity` is small (dpgo_amd.h has the warning example).
//
// Stated deviations from the reference:
//  - the block size is fixed to d: a block of d vectors of length (d+1)N IS a pose-record array, so the search runs
//    on the group's record layout, its block-sparse operators, its segment table and its halo copy;
//  - the preconditioner is block Jacobi, T_p = (M_pp)^-1 with M_pp the pose's (d+1) x (d+1) diagonal block of M
//    (identity for a pose without an edge), where the reference uses an incomplete LDL^T factor (STEP 3);
//  - trivial loss only: a group created with a robust loss returns -1 (its S operator is not assembled,
//    Group::upload_operators, and the certificate theory is that of the quadratic objective).  Whoever optimised with
//    a robust loss creates a second group with LOSS_NONE and max_iterations = 0;
//  - the group must host every node of the graph (-1 otherwise: the products would need the boundary exchange);
//  - the Rayleigh-Ritz step is a scaled Cholesky reduction + cyclic Jacobi on the host; rounding is not Eigen's.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace dpgo {

enum { CERT_UNDECIDED = 0, CERT_NONNEGATIVE = 1, CERT_NEGATIVE = 2, CERT_PROVEN = 3 };   // PROVEN: Group::verify only
enum { CERT_FACTOR_NOT_PD = 0, CERT_FACTOR_PD = 1, CERT_FACTOR_SKIPPED = 2 };

struct CertOptions {
  double eta = 1e-3;   // min_eig_num_tol, C++/SESync/include/SESync/SESync.h:88
  double tau = 1e-6;   // LOBPCG.h:138
  int max_iters = 2000;
  int precondition = 1;
  int stop_on_negative = 1;
  int refresh_every = 50;   // S V, S P by real products every so many iterations (drift of the recurrences)
  unsigned long long seed = 0;
};

struct CertResult {
  int status = CERT_UNDECIDED, iterations = 0, restarts = 0;
  double theta = 0, residual = 0, S_norm_est = 0, stationarity = 0;
};

// STEP 1 (SESync_utils.cpp:731-754).  fronts, levels, max_front, factor_entries (sum (w + u) w over the fronts) and
// factor_bytes (the device bytes of the numeric phase: every front matrix at once, the value array, the maps) come from
// the symbolic analysis and are filled for SKIPPED too; pivot_min / pivot_max: the range of the pivots d_kk of the
// fronts that factored (all of them for PD); symbolic_s: host seconds of the analysis (0 after the first call of a
// group), numeric_s: host seconds from the launch of k_cert_matrix to the verdict.
struct CertFactor {
  int outcome = CERT_FACTOR_SKIPPED, fronts = 0, levels = 0, max_front = 0;
  long long factor_entries = 0, factor_bytes = 0;
  double eta = 0, pivot_min = 0, pivot_max = 0, stationarity = 0, symbolic_s = 0, numeric_s = 0;
};

// ---- the host's Rayleigh-Ritz step (cert.cpp; no device) ----
// A, B: n x n row-major symmetric, n = ns * nblk (the Gram matrices B^T S B and B^T B of the basis, nblk blocks of ns
// columns).  Both are scaled by diag(B)^-1/2, B is Cholesky-factored; a pivot below 1e-12 drops the LAST block (the
// usual LOBPCG restart without P) and the step is redone on the leading blocks.  theta: the ns smallest Ritz values,
// ascending; C: n x ns row-major, C^T B C = I, C^T A C = diag(theta), rows of dropped blocks zero; *used: blocks used.
// -1 when not even the first block has a positive definite mass matrix.
int rayleigh_ritz(int ns, int nblk, const double *A, const double *B, double *theta, double *C, int *used);
// the cyclic Jacobi of that step on its own: A (n x n row-major, symmetric, n <= 9) = Z diag(w) Z^T, Z row-major with the
// eigenvectors in its columns, w in no particular order
int sym_eig(int n, const double *A, double *Z, double *w);

// ---- kernels (cert.hip) ----
constexpr int cert_ntri(int d) { return 3 * d * (3 * d + 1) / 2; }          // upper triangle of a 3d x 3d matrix
constexpr int cert_nsums(int d) { return 2 * cert_ntri(d) + 2 * d; }        // both Gram matrices + the stopping test's norms
constexpr int cert_tri(int n, int a, int b) { return a * n - a * (a - 1) / 2 + (b - a); }   // a <= b
struct CertCoef {
  double C[27];      // 3d x d row-major: rows [0, d) multiply V, [d, 2d) W, [2d, 3d) P
  double theta[3];
};
// All over the own rows, one workgroup per own segment; partial sums are stored at partials[s * T.nseg_own + segment].
// Lam[p] (d x d row-major) from the records of X and M X; with SX: (S X) stored; partial 0 = |(S X)_p|^2
void launch_cert_lambda(const LaunchCtx &lc, const double *X, const double *MX, double *Lam, double *SX, double *partials);
// out = MV - [0 ; Lam V.Y]  (out may be MV)
void launch_cert_apply(const LaunchCtx &lc, const double *Lam, const double *V, const double *MV, double *out);
// SW <- SW - [0 ; Lam W.Y] (SW holds M W on entry), then the upper triangles of B^T B (sums [0, ntri)) and B^T (S B)
// (sums [ntri, 2 ntri)), B = [V W P]
void launch_cert_gram(const LaunchCtx &lc, const double *Lam, const double *V, const double *W,
                      const double *P, const double *SV, double *SW, const double *SP, double *partials);
// P' = W C_w + P C_p, V' = V C_v + P', the same for S V', S P'; R' = S V' - V' diag(theta); W' = Tp R' (Tp: (d+1)^2 per
// pose, null: R'); sums 2 ntri + j = |R'_j|^2, 2 ntri + d + j = |V'_j|^2
void launch_cert_update(const LaunchCtx &lc, const CertCoef &c, const double *Tp, double *V,
                        double *W, double *P, double *SV, const double *SW, double *SP, double *partials);
// out = S + eta I in the CSR order of the pose-major matrix: the (d+1)^2 nb_p values of pose p's rows are one run starting
// at (d+1)^2 bptr[p] (row r, block j, column c at r (d+1) nb_p + j (d+1) + c); Mval: M in the same order; diag_pose[k]: p
// for the diagonal block of pose p, -1 for every other block
void launch_cert_matrix(int d, hipStream_t st, int nposes, const int *bptr, const int *diag_pose, const double *Mval,
                        const double *Lam, double eta, double *out);
// host[s] = sum over the own segments of partial s, s < nsums, in segment order; then the flag
void launch_cert_reduce(hipStream_t st, const SegTable &T, int nsums, const double *partials, double *host, ReadbackFlag flag);

}  // namespace dpgo
