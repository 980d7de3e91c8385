// Hessian modes: the k smallest eigenpairs of the anchored tangent-space Hessian H of cov.h, on the factor every other
// consumer of H uses (hess.h) -- at a saddle: how negative the curvature is, along which poses, and a lower point; at a
// minimum: 1 / lambda_min(H), the largest eigenvalue of the covariance (E-optimality), and the direction the graph
// determines worst.
//
// Shift-invert block subspace iteration with Rayleigh-Ritz.  The unknowns are cov.h's (n = dof N, pose-major, the pose
// `anchor` held fixed); the anchor's identity block is excluded: every vector has exact zeros on its rows.
//
//     mu = shift > 0 ? shift : 0;  H, hmax, g, F at X
//     factor A = H + mu I (non-anchor diagonal); a non-positive pivot: mu = max(10 mu, 1e-3 hmax), at most max_tries times
//     b = 16 ceil((k + guard) / 16) <= 64 columns;  V = V0(seed)             (k_modes_init)
//     for it = 1 ... max_iters:
//         W = A^-1 V                                                          (ONE batch of spd_msolve_device)
//         G = W'W, T = W'V = W'AW, lower triangles                            (k_modes_gram, k_modes_reduce, one read-back)
//         T c = theta G c, theta ascending, C'GC = I                          (modes_ritz, host);  lambda_j = theta_j - mu
//         V <- W C;  R = V_old C - (W C) Theta = A v_j - theta_j v_j;  |R_j|^2, |V_j|^2   (k_modes_update, k_modes_reduce)
//         |R_j| <= rel_tol hmax for every j < k  -> CONVERGED
//     -> MAX_ITERS, with the pairs and residuals of the last iteration
//
// The k smallest eigenvalues of A, minus mu, are the k smallest of H whatever mu is: an indefinite H is an input, not a
// refusal.  The guard columns only buy convergence rate and are never reported.  A pivot of the scaled G below 1e-12
// drops the trailing columns for that step (they are carried as W's, scaled); fewer than k left: STALLED.
//
// Escape (want_escape, lambda_0 < 0): with g the tangent gradient, s = -sign(g'v_0) (+1 at zero), alpha_0 = 0.5 / |v_0|_inf
// and pred(alpha) = alpha |g'v_0| + 1/2 alpha^2 |lambda_0|, alpha is halved up to 30 times until
// F(retract(X, alpha s v_0)) <= F(X) - 0.1 pred(alpha); that point and its F are returned, or escaped = 0 and X itself.
//
// Every sum is a fixed chain -- the rows of a workgroup in ascending order, four per matrix instruction, then the workgroups in
// order: the same bits on every call, no atomics, and an entry's bits do not depend on b or on the other columns.
#pragma once
#include <hip/hip_runtime.h>

#include "hess.h"
#include "kernels.h"

namespace dpgo {

enum { MODES_CONVERGED = 0, MODES_MAX_ITERS = 1, MODES_STALLED = 2, MODES_SKIPPED = 3 };

constexpr int MODES_MAX_K = 60;      // with guard >= 4 the block stays within one batch of the block solve
constexpr int MODES_MAX_B = 64;
constexpr int MODES_ROWS = 512;      // rows of the blocks one workgroup owns (k_modes_gram, k_modes_update)

struct ModesOptions {
  int guard = 4, max_iters = 100, max_tries = 8, want_escape = 0;
  double rel_tol = 1e-8, shift = 0;
  unsigned long long seed = 1;
};

// iterations: solves of the block; factorisations: all of them; shift_tries: those that met a non-positive pivot; block: b;
// negative: converged lambda_j < 0 among the k reported.  unknowns ... device_bytes are filled for SKIPPED too.  factor_ms:
// from the launch that writes H to the last verdict; solve_ms / gram_ms / ritz_ms / update_ms: host milliseconds of the phases
// of the loop, each up to its read-back (solve_ms is enqueue time: its launches finish under gram_ms).
struct ModesResult : HessAnalysis {
  int outcome = MODES_SKIPPED, iterations = 0, factorisations = 0, shift_tries = 0, block = 0, negative = 0, escaped = 0;
  double mu = 0, hmax = 0, stationarity = 0, escape_alpha = 0, F = 0, F_escape = 0;
  double solve_ms = 0, gram_ms = 0, ritz_ms = 0, update_ms = 0, total_ms = 0;
};

inline int modes_block(int k, int guard) { return 16 * ((k + guard + 15) / 16); }
inline int modes_workgroups(long long n) { return (int)((n + MODES_ROWS - 1) / MODES_ROWS); }
// doubles of the partial sums of one launch: [workgroup][2 b b] for the Gram matrices, [workgroup][2 b] for the update
inline long long modes_partials(long long n, int b) { return (long long)modes_workgroups(n) * 2 * b * b; }

// V0[i][j], i the unknown, j < 64 the column: splitmix64's finaliser of seed + 0x9e3779b97f4a7c15 (64 i + j + 1), its top 52
// bits m mapped to (2 m + 1 - 2^52) 2^-52 -- an odd integer below 2^52 in magnitude, converted exactly: in (-1, 1), never 0
__host__ __device__ inline double modes_start_entry(unsigned long long seed, unsigned long long i, unsigned j) {
  unsigned long long z = seed + 0x9e3779b97f4a7c15ull * (64ull * i + j + 1ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  z = z ^ (z >> 31);
  const long long m = (long long)(2ull * (z >> 12) + 1ull) - (1ll << 52);
  return (double)m * (1.0 / 4503599627370496.0);
}

// ---- kernels (modes.hip).  V, W: n x b row-major with row length ld >= b; the columns b ... ld are neither read nor written.
// a0, dof: the anchor's rows a0 ... a0 + dof (a0 < 0: none) ----
// V <- V0: entry (i, j) from the unknown row_dof * gid[i / row_dof] + i % row_dof (gid null: i itself); zeros on the anchor's rows
void launch_modes_init(hipStream_t st, long long n, int b, int ld, int a0, int dof, unsigned long long seed, const int *gid,
                       int row_dof, double *V);
// partials[wg][0 .. b b) <- the tiles on or below the diagonal of W'W over the workgroup's rows, [b b .. 2 b b) of W'V
void launch_modes_gram(hipStream_t st, long long n, int b, int ld, const double *W, const double *V, double *partials);
// out[0 .. b (b + 1) / 2) <- the lower triangle of G packed by rows (i (i + 1) / 2 + j), then T's, the workgroups' partials added
// in order; then the flag (flag.host null: none)
void launch_modes_reduce_gram(hipStream_t st, int nwg, int b, const double *partials, double *out, ReadbackFlag flag);
// V <- W C in place; partials[wg][j] <- sum over the workgroup's rows of (V_old C - (W C) theta_j)_rj^2, [b + j] of (W C)_rj^2.
// C (b x b row-major, column j the j-th coefficient vector) and theta (b) in device memory; zeros on the anchor's rows
void launch_modes_update(hipStream_t st, long long n, int b, int ld, int a0, int dof, const double *W, double *V, const double *C,
                         const double *theta, double *partials);
// out[0 .. nent) <- the sums over the workgroups, in order, of partials[wg * stride + e]; then the flag (flag.host null: none)
void launch_modes_reduce(hipStream_t st, int nwg, int stride, int nent, const double *partials, double *out, ReadbackFlag flag);
// sol[i] = coef V[i ld + col]
void launch_modes_column(hipStream_t st, long long n, int ld, int col, double coef, const double *V, double *sol);

// ---- the host's eigenproblem (modes.cpp): T c = theta G c for order b <= 64, both matrices b x b row-major, the LOWER triangles
// read.  G is scaled to a unit diagonal and factored; a pivot below 1e-12 at column p drops the columns p ... b - 1 (used = p).
// theta[0 .. used) ascending, C (b x b row-major): column j < used the coefficients with C'GC = I, column j >= used the unit
// vector e_j / sqrt(G_jj) (theta_j = 0).  Returns 0, or -1 for bad arguments or used = 0.
int modes_ritz(int b, const double *G, const double *T, double *theta, double *C, int *used);
// the packed read-back of launch_modes_reduce_gram as two full symmetric matrices
void modes_unpack(int b, const double *packed, double *G, double *T);

}  // namespace dpgo
