// The Riemannian staircase: from a point whose certificate is NEGATIVE to the certified global minimum, or to a lower bound.
//
// The reference does this in its SE-Sync tree: the loop of SESync (C++/SESync/src/SESync.cpp:280-440), escape_saddle
// (:575-680) and round_solution.  Here it runs on the group's record layout, with the certificate's products, Lambda, verify
// (cert.h) and block-Jacobi T_p, and the polish (polish.h) at the end.
//
// A point at rank r, d <= r <= 2d, is X in R^{(d+1)N x r} in the reference's row order: rows 0..N-1 the translations
// (r-vectors), rows N + d p + k the rows of Y_p in R^{d x r}, Y_p Y_p^T = I_d.
//     F        = 1/2 tr(X^T M X)
//     Lambda_p = sym((M X)_p.Y Y_p^T)                       d x d, as in cert.h
//     grad F   = S X,  S = M - Lambda, alike on every column
//     Hess[V]  = Proj_X(S V),  Proj_X(W)_p.Y = W_p.Y - sym(W_p.Y Y_p^T) Y_p,  translations untouched
//     retract  : Z_p.t = X_p.t + V_p.t;  A = Y_p + V_p.Y;  Z_p.Y = (A A^T)^-1/2 A   (the polar factor)
// A lifted array is TWO ordinary record arrays side by side: block A holds columns 0..d-1, block B columns d..2d-1; columns
// >= r are zero.  Every operation above keeps a zero column zero, so no kernel knows r; only the lift (which writes column
// r) and the rounding do.  A product with M is cert_apply_M once per block; block B is skipped while r = d.
//
//     r = d;  Y = X (block B zero)
//     repeat:
//         Y = TNT(Y) at rank r        TNT.h / STPCG as oracle/tnt.py restates them, matrix-free, Hess as above, preconditioner
//                                     Proj o T_p o Proj (precondition = 0: none)
//         Lambda = Lambda(Y);  verdict, theta, x = verify on the Lambda in place (Cholesky of S + eta I, then LOBPCG only
//                                     when it did not succeed)
//         verdict != NEGATIVE         -> SOLVED (PROVEN, or NONNEGATIVE / UNDECIDED kept as they are: evidence, not proof)
//         r == r_max                  -> MAX_RANK
//         lift: column r of Y is zero; Ydot = x in column r (tangent: Y_p Ydot_p^T = 0), |Ydot| = 1
//         alpha = 1; at most 30 times: Z = retract(Y, alpha Ydot); accept when F(Z) <= F(Y) + 1/4 alpha^2 theta, else alpha /= 2
//         none accepted               -> SADDLE
//         Y = Z;  r += 1
//     round: Gram matrix sum_p Y_p^T Y_p (2d x 2d) -> host symmetric eigenproblem (cert.cpp's cyclic Jacobi) -> B = the d
//            leading eigenvectors, each signed so that its entry of largest magnitude is positive -> X B, every Y_p B onto
//            SO(d) (the last column of B negated first where most det(Y_p B) are negative) -> Xhat.  At final rank d the
//            point is on SO(d)^N already and is taken as it is.
//     Xhat = polish(Xhat) (option, on by default; left as it is where polish is SKIPPED)
//     F(Xhat) > F(input) -> Xhat = the input        the result is never worse than what was handed in
//
// Stated deviations from the reference:
//  - the escape starts at alpha = 1 with a sufficient-decrease test on the second-order model; the reference starts at
//    10 tol / |theta| and adds a gradient test (SESync.cpp:575-680);
//  - r is capped at 2d (two record arrays); the reference's rmax is 10;
//  - the start is rank d from the caller's point; the reference starts at r0 = 5 from the chordal point;
//  - the host reads two sets of scalars per CG step (the curvature, then <r, z>), not one: the step length needs the first,
//    the next direction the second.
//
// gap = F_final - F_sdp is the reference's suboptimality_bound (SESync.h, SESyncResult): F_sdp is the value of the rank-r
// relaxation at the final Y, a lower bound on F of every feasible point ONLY where the final certificate is PROVEN and
// `stationarity` is small; otherwise it is the difference of two numbers.
//
// The restrictions of the certificate and the polish: the trivial loss, the group hosts every node.  The optimiser's state is
// not touched.  The refusal is the polish's: what this allocates (the lifted vectors below) is counted against max_bytes and
// against half of the free device memory before anything is allocated.
#pragma once
#include <hip/hip_runtime.h>

#include "cert.h"
#include "kernels.h"

namespace dpgo {

enum { STAIR_SOLVED = 0, STAIR_MAX_RANK = 1, STAIR_SADDLE = 2, STAIR_SKIPPED = 3 };

// the optimiser's options are named as in SESyncOpts (C++/SESync/include/SESync/SESync.h:25-67)
struct StairOptions {
  double grad_norm_tol = 1e-2, preconditioned_grad_norm_tol = 1e-4, rel_func_decrease_tol = 1e-6, stepsize_tol = 1e-3;
  int max_iterations = 1000, max_tCG_iterations = 10000;
  double STPCG_kappa = 0.1, STPCG_theta = 0.5;
  int r_max = 0;          // 0: 2d
  int precondition = 1;   // Proj o T_p o Proj
  int polish = 1;
  double min_eig_num_tol = 1e-3;   // eta of the certificate
  long long max_factor_bytes = 0;  // of verify's factorisation (0: no limit of the caller's)
};

struct StairResult {
  int outcome = STAIR_SKIPPED, cert_status = CERT_UNDECIDED, final_rank = 0, levels = 0;
  int tnt_iterations = 0, hess_products = 0, replaced_by_input = 0, polish_outcome = 3;
  double theta = 0, stationarity = 0, F_initial = 0, F_sdp = 0, F_rounded = 0, F_final = 0, gap = 0;
  double sigma[6] = {0, 0, 0, 0, 0, 0};   // the 2d singular values of the rotation rows of the final Y, descending
  long long device_bytes = 0;
  double optimise_ms = 0, verify_ms = 0, round_ms = 0, total_ms = 0;
};

// per level: rank, F in, F out, |grad| out, TNT iterations, Hessian products, certificate status, theta, accepted alpha (0: no
// escape from this level), halvings
constexpr int STAIR_LOG_COLS = 10;

// ---- kernels (stair.hip): one wave per own segment, lane = pose; a lifted array is the pair (a, b) of record arrays;
// partial sums at partials[slot * T.nseg_own + segment], reduced in segment order by launch_polish_reduce ----
struct Lifted {
  double *a = nullptr, *b = nullptr;
};
struct LiftedC {
  const double *a = nullptr, *b = nullptr;
  LiftedC() = default;
  __host__ __device__ LiftedC(const Lifted &l) : a(l.a), b(l.b) {}
  __host__ __device__ LiftedC(const double *a_, const double *b_) : a(a_), b(b_) {}
};
// Lam[p] (d x d row-major) from both blocks of X and M X; G (a null: not stored) = S X; slot 0: |G|^2, slot 1: F
void launch_stair_lambda(const LaunchCtx &lc, LiftedC X, LiftedC MX, double *Lam, Lifted G, double *partials);
// out = Proj_X(MV - Lam V); slot 0: <V, out>, slot 1: |out|^2, slot 2: |V|^2
void launch_stair_hess(const LaunchCtx &lc, LiftedC X, const double *Lam, LiftedC V, LiftedC MV, Lifted out, double *partials);
// init: s = hs = 0, r = G; else s += alpha p, hs += alpha Hp, and with `residual` r += alpha Hp.  With `residual` (or init)
// z = Proj_X(Tp Proj_X r) (Tp null: z = r); slot 0: <r, z>, slot 1: <z, z>
void launch_stair_cg_update(const LaunchCtx &lc, LiftedC X, const double *Tp, bool init, bool residual, double alpha, LiftedC G,
                            LiftedC p, LiftedC Hp, Lifted s, Lifted hs, Lifted r, Lifted z, double *partials);
// p = -z + beta p
void launch_stair_cg_dir(const LaunchCtx &lc, LiftedC z, double beta, Lifted p);
// Z = retract(X, alpha V); slot 0: <G, V>, slot 1: |V|^2, slot 2: <V, HV> (G, HV: a null: that slot is 0)
void launch_stair_retract(const LaunchCtx &lc, LiftedC X, LiftedC V, double alpha, LiftedC G, LiftedC HV, Lifted Z, double *partials);
// the upper triangle of sum_p Y_p^T Y_p (2d x 2d), slot cert_tri(2d, a, b)
void launch_stair_gram(const LaunchCtx &lc, LiftedC X, double *partials);
// W = X B (records, d columns; B: 2d x d row-major, by value); slot 0: the poses with det(W_p.Y) > 0
struct StairB {
  double v[18];
};
void launch_stair_round(const LaunchCtx &lc, LiftedC X, const StairB &B, double *W, double *partials);
// out.t = W.t on the own rows (out.Y: the projected rotations, written by launch_retract_rot)
void launch_stair_copy_t(const LaunchCtx &lc, const double *W, double *out);

}  // namespace dpgo
