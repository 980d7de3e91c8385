// Per-edge reliability: how well is each measurement of the graph checked by the others, and does it agree with them?
//
// pairs.h's gate answers for a CANDIDATE: its d^2 = r^T (rel + Omega^-1)^-1 r counts an edge twice when rel was computed with that
// edge in the graph.  For an edge that is in, at a critical point X of F and with Sigma = H^-1 the covariance of cov.h (the
// unknowns, the gauge, k_cov_hessian), rel = J Sigma_joint J^T, r and Omega = blkdiag(tau I_d, 2 kappa I_{dof - d}) as in
// pairs_math.h -- the edge's own (R~, t~, kappa, tau) taken as the candidate --
//     C = Omega^-1 - rel                       the covariance of the residual,
//     d2_loo = r^T C^-1 r                      the leave-one-out statistic (Baarda / Pope data snooping): what the gate would say
//                                              of this edge at the solution of the graph without it; 1/2 d2_loo is the first-order
//                                              drop of the optimum when the edge is removed,
//     r_loo = Omega^-1 C^-1 r                  the residual the edge would have there,
//     influence = z^T rel z,  z = C^-1 r       the H-norm squared of the displacement of that solution,
//     redundancy = dof - sum_i Omega_ii rel_ii = tr(I - Omega rel), redundancy_trans = d - tau sum_{i < d} rel_ii,
//     d2_own = r^T Omega r                     twice the edge's own term of F, to second order in r.
// The redundancies of all edges sum to dof (m - N + 1) where the Gauss-Newton model is exact (zero residuals).  No threshold is
// applied anywhere: d2_loo is the caller's to compare with a chi-square quantile of dof degrees of freedom, and `redundancy`
// says how far it can be trusted -- an edge nothing else checks (a pendant edge) has redundancy 0 and C = 0 up to rounding.
//
// One record per listed edge, 6 + 2 dof doubles (rely_math.h: RelyDims):
//     d2_loo, flag, redundancy, redundancy_trans, d2_own, influence, r[dof], r_loo[dof]
// flag 0: every pivot of C's Cholesky factor is positive.  1: one is not (no redundancy, or the Gauss-Newton model does not
// hold at X): d2_loo, influence and r_loo are exact zeros, the rest is filled.  2: kappa or tau of the edge is not > 0 (what
// scale_edges can leave): zeros but the flag; such edges are not uploaded.
//
// Everything needed is what the selected inversion leaves on the device -- S_pp, S_pq and S_qq of every edge -- so
//   RELY_SELINV   k_cov_hessian, spd_refactor_device, spd_selinv_device, then k_rely_gather reads the three blocks of every
//                 listed edge straight out of spd_selinv_values into pairs.h's `joint` layout (nothing goes through the host);
//   RELY_SOLVE    pairs.h's column plan and batches on the distinct poses of the listed edges (no block of the inverse is
//                 stored: for graphs where the selected inversion is refused, or for a few edges);
//   RELY_AUTO     SELINV where its bytes are not refused, otherwise SOLVE, otherwise RELY_SKIPPED.
// Behind either, launch_pairs_gate supplies rel and r, and k_rely_edge runs rely_math.h with one lane per edge.
//
// The restrictions are cov.h's: the trivial loss, a group that hosts every node.  The optimiser's state is not touched.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hess.h"

namespace dpgo {

struct Graph;

enum { RELY_OK = 0, RELY_NOT_PD = 1, RELY_SKIPPED = 2 };
enum { RELY_AUTO = 0, RELY_SELINV = 1, RELY_SOLVE = 2 };

// unknowns ... max_front, the three byte counts and symbolic_s come from the symbolic analysis and the sizes of the call and are
// filled for SKIPPED too.  device_bytes_selinv: cov.h's count (the numeric phase with its W / WT panels, the blocks of the
// selected inversion, the maps) plus this call's buffers (the gather map, joint, rel, the candidates, the gate's output, the
// records, the row list); device_bytes_solve: pairs.h's count for the column plan of the listed edges plus the same buffers;
// device_bytes: that of method_used (of the method asked for where the call is SKIPPED; AUTO: the smaller of the two).
// edges: listed; flagged: records with flag 1; unweighted: with flag 2; redundancy_sum: the sum of the records' redundancy in
// list order on the host, flag-2 edges left out.  factor_ms: k_cov_hessian and the factorisation up to its verdict;
// inverse_ms: the selected inversion and k_rely_gather, or the batches, up to a synchronise; edge_ms: k_pairs_gate, k_rely_edge
// and the copies to the host.
struct RelyResult : HessAnalysis {
  int outcome = RELY_SKIPPED, method_used = RELY_AUTO, edges = 0, flagged = 0, unweighted = 0, columns = 0, batches = 0;
  long long device_bytes_selinv = 0, device_bytes_solve = 0;
  double redundancy_sum = 0, stationarity = 0, inverse_ms = 0, edge_ms = 0;
};

constexpr int rely_width(int d) { return 6 + 2 * (d + d * (d - 1) / 2); }
// the gather map of one edge: off (3 int64 per edge): the first entry of the front that holds S_pp, S_pq, S_qq (-1: a block that
// involves the anchor, zeros); loc (3 + 4 dof ints per edge): the row lengths w + u of those three fronts, then the positions of
// p's and of q's unknowns in their own fronts, then those of p's and of q's in the front that holds S_pq
constexpr int rely_map_ints(int dof) { return 3 + 4 * dof; }

// ---- kernels (rely.hip) ----
// joint (nedges x 3 dof^2, pairs.h's layout) <- the entries of Sig = spd_selinv_values named by the map; one thread per entry
void launch_rely_gather(hipStream_t st, int dof, int nedges, const int64_t *off, const int *loc, const double *Sig, double *joint);
// rec (nedges x rely_width(d)) <- rely_one of every edge: rel (nedges x dof^2); r: edge k's residual at r + k ldr (k_pairs_gate's
// output: gate + 2, ldr = 2 + dof); kt: its kappa, tau at kt + k ldkt (the candidates: cand + d^2 + d, ldkt = d^2 + d + 2)
void launch_rely_edge(int d, hipStream_t st, int nedges, const double *rel, const double *r, int ldr, const double *kt, int ldkt,
                      double *rec);

// host only: rely_one (rely_math.h) of n edges -- rel: n x dof^2, r: n x dof, kappa, tau: n each, rec: n x rely_width(d)
int rely_edge_host(int d, int n, const double *rel, const double *r, const double *kappa, const double *tau, double *rec);
// k_rely_edge alone on the same (host) arrays, on the current device
int rely_edge_device(int d, int n, const double *rel, const double *r, const double *kappa, const double *tau, double *rec);

}  // namespace dpgo
