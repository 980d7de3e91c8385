// Graduated non-convexity (GNC-TLS and GNC-GM; Yang, Antonante, Tzoumas, Carlone, "Graduated Non-Convexity for Robust Spatial
// Perception", RA-L 2020): which measurements are outliers, and what is the solution without them -- on the device.
//
// Definitions.  s_e = s_rot + s_trans is what edge_lane<D> returns under loss 0 (the bits of dpgo_edge_eval_run).
// c2 = barc2 > 0 is the caller's inlier threshold on s_e.  The robust set R is the edges the loss may touch: with
// robust_set == NULL the inter rule of edges.h, otherwise robust_set[e] != 0 (so that a one-node graph can use the feature).
// Every edge outside R keeps w_e = 1.
//
//     F_w(X)  = 1/2 sum_e w_e s_e
//     F_mu(X) = 1/2 sum_{e not in R} s_e + 1/2 sum_{e in R} rho_mu(s_e)
//
// TLS, in this order, the branches before any division (s = 0 is safe):
//     s <= mu / (mu + 1) c2:   w = 1, rho = s
//     s >= (mu + 1) / mu c2:   w = 0, rho = c2
//     otherwise:               w = sqrt(c2 (mu (mu + 1)) / s) - mu,    rho = 2 sqrt(c2 (mu (mu + 1)) s) - mu (c2 + s)
// (w is clamped to [0, 1]: the true value lies there and the rounding of the difference may not.)
// GM, with delta = mu c2, edge_loss's Geman-McClure formulas:  w = delta^2 / (s + delta)^2,  rho = delta s / (s + delta).
//
//     level 0:  w = 1;  X0 = inner(X, w);  s_max = max_{e in R} s_e(X0)
//               R empty -> ALL_INLIERS
//     TLS:      2 s_max <= c2 -> ALL_INLIERS (X0 returned, w = 1);  mu = c2 / (2 s_max - c2)
//     GM:       mu = max(1, 2 s_max / c2)
//     for k = 1 .. max_levels:
//         w_R = weight_mu(s(X_{k-1}));  record F_mu(X_{k-1}) and F_w(X_{k-1});  counts of w == 0, w == 1, 0 < w < 1 over R
//         X_k = inner(X_{k-1}, w);  an inner STALLED -> INNER_FAILED (X_{k-1} and the weights it was solved with returned)
//         evaluation-only pass at the same mu on X_k:  F_w(X_k), F_mu(X_k), s_max
//         TLS:  no weight strictly between 0 and 1 -> CONVERGED;   mu = mu_step mu
//         GM:   mu == 1 -> CONVERGED;                              mu = max(mu / mu_step, 1)
//     k == max_levels without the above -> MAX_LEVELS
//
// inner is polish_loop (polish.h) with fixed weights: the Levenberg-Marquardt loop on H(S_w), no rank-one terms, F = F_w.
// An inner STALLED at level 0 is INNER_FAILED too, with X itself and unit weights returned.
//
// The invariant.  rho_mu(s) = min_w [w s + Phi_mu(w)] (Black-Rangarajan duality; TLS: Phi_mu(w) = mu (1 - w) / (mu + w) c2, GM:
// Phi_mu(w) = mu c2 (sqrt(w) - 1)^2), attained at w = weight_mu(s).  With w_k = weight_mu(s(X_{k-1})):
//     F_mu(X_k) <= F_{w_k}(X_k) + 1/2 sum_R Phi(w_k) <= F_{w_k}(X_{k-1}) + 1/2 sum_R Phi(w_k) = F_mu(X_{k-1})
// whenever the inner solve does not increase F_w: within a level F_mu never increases.
//
// Connectivity.  A level whose zero weights disconnect the graph makes H singular.  The Levenberg-Marquardt shift then
// either copes or stalls; a stall is INNER_FAILED, an outcome, not an error.
//
// The outer loop is stated once, for this objective and for the maximum-likelihood one (ml_gnc.h): Group::gnc_loop (gnc.cpp)
// owns the option check, level 0, the ALL_INLIERS test, the mu schedule, the levels with their log rows, the failure return
// and the read-out into a GncResult.  What an objective is to it is a GncObjective (group.h), a plain struct the caller
// fills: the edge pass, its summary read back, what forms the gradient behind the point pass, the Hessian launch, the device
// weight array, the host mask of R, the download of the per-edge s, and two named differences of behaviour.
//
// Two kernels (gnc.hip), fp64, fixed-order sums (wave_reduce.h), no atomics: the same bits run to run.
//   k_gnc_edge   one lane per edge in graph order, EDGE_BLOCK per workgroup, records and poses read as 16-byte units as in
//                k_robust_edge: s_rot, s_trans through edge_lane<D> under loss 0; WEIGH: w = weight_mu(s) written for e in R
//                (the array is not touched elsewhere); FIXED: w read from the array for e in R; 1 outside R in both; behind a
//                flag the rows (M_e X)_i, (M_e X)_j through robust_rows<D>.  Per workgroup, by wave shuffle, one partial each
//                (gnc_partials.h, shared with k_ml_gnc_edge): sum_{not R} s, sum_R w s, sum_R rho_mu(s), max_R s, min_R w, and
//                the counts of w == 0, w == 1, 0 < w < 1 over R.
//   k_gnc_final<NC>  one wave over the partials in strided order (as k_robust_final) and over NC counts per workgroup: the
//                summary, and optionally F_w into a slot of the certificate's partial sums, where polish_loop's reduction looks
//                (fslot / nslot as launch_robust_edge).  NC = 3 here; 5 behind k_ml_gnc_edge, the two near-pi counts after the
//                three (launch_gnc_final serves both).
// R-membership of an edge is the inter word of the plan's own copy of its record (robust_begin's robust_set overwrites it).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "edges.h"
#include "polish.h"

namespace dpgo {

enum { GNC_TLS = 0, GNC_GM = 1 };
enum { GNC_CONVERGED = 0, GNC_ALL_INLIERS = 1, GNC_MAX_LEVELS = 2, GNC_INNER_FAILED = 3, GNC_SKIPPED = 4 };

struct GncOptions {
  int kind = GNC_TLS;
  double barc2 = 1.0, mu_step = 1.4;
  int max_levels = 100;
  PolishOptions inner;
  int anchor = 0;
};

struct GncResult {
  int outcome = GNC_SKIPPED, levels = 0, steps = 0, factorisations = 0, inner_outcome = POLISH_SKIPPED;
  double mu_initial = 0, mu_final = 0, s_max_initial = 0, F_initial = 0, F_weighted_final = 0, F_surrogate_final = 0;
  int num_robust = 0, num_zero = 0, num_one = 0, num_between = 0, num_outliers = 0;
  long long device_bytes = 0;
  double symbolic_s = 0, total_ms = 0, edge_ms = 0, inner_ms = 0;
};

constexpr int GNC_LOG_COLS = 10;   // per level k >= 1: mu, F_mu(X_{k-1}), F_w(X_{k-1}), F_w(X_k), F_mu(X_k), inner steps, inner outcome, zero, one, between

// What the final pass leaves on the device (64 bytes); F_w = 1/2 (sum_out + sum_ws), F_mu = 1/2 (sum_out + sum_rho).
// Over an empty R: s_max = 0, w_min = +inf.
struct GncSummaryDev {
  double sum_out, sum_ws, sum_rho, s_max, w_min;
  long long num_zero, num_one, num_between;
};
static_assert(sizeof(GncSummaryDev) == 64, "five sums, three counts");
// per workgroup, in the order of the struct; the maximum-likelihood pass has two more counts (ml_gnc.h: MlGncSummaryDev)
constexpr int GNC_PARTIAL_SLOTS = 5, GNC_COUNT_SLOTS = 3, ML_GNC_COUNT_SLOTS = GNC_COUNT_SLOTS + 2;
// the bytes of a pass's reduction: the partials and ncounts counts of nb workgroups, and nsum summaries
constexpr long long gnc_reduce_bytes(int nb, int ncounts, int nsum) {
  return 8ll * (GNC_PARTIAL_SLOTS + ncounts) * nb + (long long)nsum * ((long long)sizeof(GncSummaryDev) + 8ll * (ncounts - GNC_COUNT_SLOTS));
}

// A summary on the host, of either objective: what gnc_loop works on.  The near-pi counts stay zero for this objective.
struct GncSummary {
  GncSummaryDev sums = {};
  long long near_pi = 0, near_pi_all = 0;
};
constexpr int GNC_SUMS = 8, ML_GNC_SUMS = 10;   // a summary as doubles, in the order of the struct (gnc_eval; ml_gnc_eval)
void gnc_summary_doubles(const GncSummary &q, int n, double *sums);   // its first n fields

// device (gnc.hip); enqueued on st.  s_out: 2 arrays of m doubles (s_rot, s_trans); w: m doubles (weigh: written on R, read
// nowhere; else read on R); rows (null: not computed): as launch_robust_edge; partials: 5 nb doubles, counts: 3 nb;
// fslot[0] = F_w with fslot[1 .. nslot) zeroed (null: neither)
void launch_gnc_edge(int d, hipStream_t st, int m, const double *rec, const double *X, int kind, double mu, double c2, bool weigh,
                     double *w, double *s_out, double *rows, double *partials, long long *counts, GncSummaryDev *sum, double *fslot,
                     int nslot);
// the final wave alone, behind an edge kernel that left 5 nb partials and ncounts nb counts (3, or 5: then sum is the head of an
// MlGncSummaryDev, whose two counts follow it); launch_gnc_edge and launch_ml_gnc_edge end with it
void launch_gnc_final(hipStream_t st, int nb, int ncounts, const double *partials, const long long *counts, GncSummaryDev *sum,
                      double *fslot, int nslot);

// Host: kind in {TLS, GM}, mu and barc2 finite and positive; otherwise false, with a line on stderr that names `who` (shared
// with ml_gnc.cpp)
bool gnc_args_ok(int kind, double mu, double barc2, const char *who);
// Host: in_R <- per edge of the m records rec (edges.h) whether it is in R: robust_set[e] != 0, or the record's inter word when
// robust_set is null.  Returns |R|.
int gnc_robust_mask(int d, int m, const double *rec, const int *robust_set, std::vector<int> &in_R);
// Host, debug (no GPU): gnc_weight_rho (gnc_math.h) on n values of s
int gnc_weight_host(int kind, double mu, double c2, const double *s, int n, double *w, double *rho);

}  // namespace dpgo
