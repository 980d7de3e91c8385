// Newton polish: from the point X the optimiser stopped at to a critical point of F = 1/2 tr(X^T M X) to working accuracy.
//
// AMM-PGO# is a first-order majorisation method, and the certificate (cert.h) and the covariances (cov.h) mean something
// only at a critical point.  Group::polish takes damped Riemannian Newton steps -- Levenberg-Marquardt on the anchored
// tangent-space Hessian H of cov.h, the same matrix in the same factor -- until the tangent gradient is at rounding level:
//
//     mu = 0
//     for k = 0 ... max_steps:
//         g, |g|, F0, H, hmax at X              (hmax: the largest diagonal entry of H over the non-anchor unknowns)
//         |g| <= (grad_tol > 0 ? grad_tol : rel_tol hmax)  -> CONVERGED
//         k == max_steps                                    -> MAX_STEPS
//         at most max_tries times:
//             factor H + mu I (non-anchor diagonal)
//             not positive definite:  indefinite += 1 if mu == 0;  mu = max(10 mu, 1e-3 hmax);  next try
//             delta = -(H + mu I)^-1 g;  Z = retract(X, delta);  F1 = F(Z)
//             pred = -1/2 g'delta + 1/2 mu |delta|^2;  rho = pred > 0 ? (F0 - F1) / pred : -1
//             accept if rho >= 0.1 or |F0 - F1| <= 1e-13 |F0|      (at the rounding floor rho is noise)
//                 X = Z;  rho > 0.75: mu = mu / 10, and mu = 0 once mu < 1e-8 hmax
//             else mu = max(10 mu, 1e-3 hmax)
//         no try accepted -> STALLED (X is the last accepted point)
//
//  * g[dof p + a] = tr(E_a(p)^T (M X)_p) with cov.h's basis: the translation row of (M X)_p for a < d, and
//    sum_c (Y_p[r2, c] (M X)_p.Y[r1, c] - Y_p[r1, c] (M X)_p.Y[r2, c]) for the rotation generator k (r1, r2 as in cov.hip).
//    The kernel reads M X, not S X: the Lambda term of S X is normal to the manifold and drops out of every trace.
//  * retract: Z_p.t = X_p.t + dt, Z_p.Y = Exp(hat(omega))^T X_p.Y, the exponential in closed form (d = 2: cos, sin;
//    d = 3: Rodrigues with a = sin(theta) / theta, b = 2 sin^2(theta / 2) / theta^2, their series below theta^2 = 1e-8).
//  * delta comes from spd_vsolve_device (spd.h) on the factor k_cov_hessian's values were factored into; F(Z) is one
//    product with M through the certificate's path, and a dot.
//  * Every sum is a fixed tree (lanes of a wave, then the segments in order): the same bits run to run, no atomics.
//
// The restrictions of the certificate and the covariance: the trivial loss only, the group hosts every node, one pose
// `anchor` is held fixed (its record is copied bit for bit).  The optimiser's state is not touched.  The refusal counts what
// polish allocates -- spd_numeric_bytes + spd_vsolve_bytes + its vectors, without the blocks of the selected inversion -- so it
// may run where covariance is SKIPPED.  max_bytes is compared with that whole figure (device_bytes); the free device memory
// with what is still to be allocated (a covariance call or an earlier polish may have left part of it).
#pragma once
#include <hip/hip_runtime.h>

#include "hess.h"
#include "kernels.h"

namespace dpgo {

enum { POLISH_CONVERGED = 0, POLISH_MAX_STEPS = 1, POLISH_STALLED = 2, POLISH_SKIPPED = 3 };

struct PolishOptions {
  int max_steps = 20, max_tries = 8;
  double rel_tol = 1e-9, grad_tol = 0;
};

// steps: accepted steps; factorisations: all of them; indefinite: factorisations at mu = 0 that met a non-positive pivot
// (the starting region was not convex).  unknowns ... device_bytes come from the symbolic analysis and are filled for
// SKIPPED too.  total_ms: host milliseconds of the loop; factor_ms: k_cov_hessian and the first shift from their launch
// (behind a synchronise) to the read-back, the later shifts and every factorisation up to its verdict; solve_ms: the vector
// solves with the retraction, the product and the read-back behind them; other_ms: the rest.
struct PolishResult : HessAnalysis {
  int outcome = POLISH_SKIPPED, steps = 0, factorisations = 0, indefinite = 0;
  double F_initial = 0, F_final = 0, grad_initial = 0, grad_final = 0, hmax = 0, mu_final = 0;
  double total_ms = 0, solve_ms = 0, other_ms = 0;
};

constexpr int POLISH_LOG_COLS = 5;   // per iteration k: F0, |g|, mu at entry, rho of the accepted try, tries

// ---- kernels (polish.hip): one wave per own segment, lane = pose; partial sums at partials[slot * T.nseg_own + segment] ----
// g (dof per own row, null: not written) from the records of X and M X, zeros on the anchor's row; slot_g2 (< 0: none):
// |g|^2, slot_F: 1/2 <X, M X>
void launch_polish_grad(const LaunchCtx &lc, const double *X, const double *MX, int anchor, double *g, int slot_g2, int slot_F,
                        double *partials);
// val: H in k_cov_hessian's order.  save: the dof diagonal entries of every row go to hdiag first, and their maximum over the
// non-anchor rows to slot_hmax; then, always, the diagonal entries of the non-anchor rows become hdiag + mu.
void launch_polish_shift(const LaunchCtx &lc, const int *bptr, const int *diag_pose, int anchor, double mu, bool save, double *hdiag,
                         double *val, int slot_hmax, double *partials);
// Z = retract(X, -sol) on the own rows (sol = (H + mu I)^-1 g), the anchor's record copied; slot_gd: g'delta, slot_dd: |delta|^2
void launch_polish_retract(const LaunchCtx &lc, const double *X, const double *sol, const double *g, int anchor, double *Z,
                           int slot_gd, int slot_dd, double *partials);
// host[s] = the segments' partials of slot s in order, s < nslots: their sum, or their maximum where bit s of max_mask is set;
// then the flag
void launch_polish_reduce(hipStream_t st, const SegTable &T, int nslots, unsigned max_mask, const double *partials, double *host,
                          ReadbackFlag flag);

}  // namespace dpgo
