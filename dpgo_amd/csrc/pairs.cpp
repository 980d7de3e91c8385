// Host side of the joint pair covariances (pairs.h): the column plan, the parts of the refusal, and the loop -- H written on the
// device (k_cov_hessian) and factored (hess.cpp: hess_factor), the unit columns of the poses asked for solved batch by batch
// (spd_msolve_device), the blocks gathered, the relative covariance and the gate of every pair.  The matrix is the
// covariance's (cov.cpp): its pattern, its symbolic analysis and its numeric context are shared.  The optimiser's state is not
// touched (cert_begin).
#include "pairs.h"

#include <algorithm>
#include <chrono>
#include <cmath>

#include "cert_state.h"
#include "cov_state.h"
#include "group.h"

namespace dpgo {

PairsPlan pairs_plan(int dof, int anchor, const int *pairs, int npairs) {
  PairsPlan pl;
  for (int k = 0; k < 2 * npairs; k++)
    if (pairs[k] != anchor) pl.poses.push_back(pairs[k]);
  std::sort(pl.poses.begin(), pl.poses.end());
  pl.poses.erase(std::unique(pl.poses.begin(), pl.poses.end()), pl.poses.end());
  pl.pair_col.assign((size_t)2 * npairs, -1);
  for (int k = 0; k < 2 * npairs; k++)
    if (pairs[k] != anchor)
      pl.pair_col[k] = dof * (int)(std::lower_bound(pl.poses.begin(), pl.poses.end(), pairs[k]) - pl.poses.begin());
  pl.columns = dof * (int)pl.poses.size();
  pairs_plan_sizes(pl.columns, &pl.batches, &pl.kb);
  return pl;
}

// The analysis and the refusal of the block solves (pair_covariance, sensitivity, robust_sensitivity): the numeric phase, the
// block solve of kb columns -- counted as still to allocate whether an earlier call has left its buffers or not -- and the
// call's own buffers; not the blocks of the selected inversion.
int Group::pairs_setup(long long max_bytes, HessPart own, int kb, HessAnalysis &out) {
  if (cov_analyse(out) != 0) return -1;
  const long long solve = (long long)spd_msolve_bytes(cov_->F, kb);
  return hess_reserve(max_bytes, "pair_covariance", {cov_->numeric_part(), {solve, solve}, own}, out);
}

// The batches of a column plan behind a factorisation that succeeded: per batch the unit right-hand sides, the block solve and the
// gather of the blocks whose columns it holds.  d_prow (2 npairs unified own rows) and d_joint (npairs x 3 dof^2, zeroed by the
// caller: the anchor's blocks) are the caller's, on the device, where joint stays; returns behind a synchronise.
int Group::pairs_solve_joint(const PairsPlan &pl, int npairs, const int *d_prow, double *d_joint, const char *who) {
  CovState &s = *cov_;
  const std::vector<int> &row_of = cert_->row_of;
  const int dof = cov_dof(d_);
  const long long n = (long long)dof * P0_;
  std::vector<int> col_unknown((size_t)std::max(pl.columns, 1), 0);
  for (int i = 0; i < (int)pl.poses.size(); i++)
    for (int a = 0; a < dof; a++) col_unknown[(size_t)dof * i + a] = dof * row_of[pl.poses[i]] + a;
  DevBuf<int> d_pcol, d_unk;
  DevBuf<double> d_Xb;
  d_pcol.upload(pl.pair_col);
  d_unk.upload(col_unknown);
  d_Xb.alloc((size_t)n * pl.kb, false);
  for (int b = 0; b < pl.batches; b++) {
    const int c0 = b * PAIRS_BATCH, nc = std::min(PAIRS_BATCH, pl.columns - c0);
    HIP_CHECK(hipMemsetAsync(d_Xb.p, 0, sizeof(double) * (size_t)n * pl.kb, st_));
    launch_pairs_rhs(st_, d_unk.p, c0, nc, d_Xb.p, pl.kb);
    if (spd_msolve_device(s.F, d_Xb.p, nc, pl.kb, st_) != 0) {
      fprintf(stderr, "[dpgo_amd] ERROR: %s: the solve failed on the device.\n", who);
      return -1;
    }
    launch_pairs_gather(st_, dof, npairs, d_prow, d_pcol.p, c0, nc, d_Xb.p, pl.kb, d_joint);
  }
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(st_));
  return 0;
}

int Group::pair_covariance(const double *X, int ld, int anchor, long long max_bytes, const int *pairs, int npairs,
                           const double *candidates, double *joint, double *rel, double *gate, PairsResult &out) {
  out = PairsResult();
  if (npairs < 0 || (npairs > 0 && (!pairs || !joint || !rel)) || (candidates && !gate)) {
    fprintf(stderr, "[dpgo_amd] ERROR: pair_covariance: missing output or pair arrays.\n");
    return -1;
  }
  if (cov_begin(X, ld, anchor) != 0) return -1;
  CertState &c = *cert_;
  CovState &s = *cov_;
  const int d = d_, dof = cov_dof(d), DD = dof * dof, N = P0_, ncand = d * d + d + 2, ngate = 2 + dof;
  if (!pairs_args_ok("pair_covariance", pairs, npairs)) return -1;
  if (candidates)
    for (int k = 0; k < npairs; k++) {
      const double kappa = candidates[(size_t)k * ncand + d * d + d], tau = candidates[(size_t)k * ncand + d * d + d + 1];
      if (!(kappa > 0) || !(tau > 0) || !std::isfinite(kappa) || !std::isfinite(tau)) {
        fprintf(stderr, "[dpgo_amd] ERROR: pair_covariance: candidate %d has a weight that is not positive.\n", k);
        return -1;
      }
    }
  const PairsPlan pl = pairs_plan(dof, anchor, pairs, npairs);
  out.columns = pl.columns;
  out.batches = pl.batches;
  const long long n = (long long)dof * N;
  const long long own = 8ll * (n * pl.kb + (long long)npairs * (4 * DD + (candidates ? ncand + ngate : 0))) +
                        4ll * (4ll * npairs + pl.columns);
  const int ready = pairs_setup(max_bytes, {own, own}, pl.kb, out);
  if (ready < 0) return -1;
  for (int b = 0; b < pl.batches; b++) {
    const int nc = std::min(PAIRS_BATCH, pl.columns - b * PAIRS_BATCH);
    out.solve_flops += 4.0 * (double)s.F.entries * (16 * ((nc + 15) / 16));
    out.factor_bytes += 16.0 * (double)s.F.entries;
  }
  cert_prepare(X, ld, &out.stationarity);
  if (ready != 0) return 0;   // SKIPPED, with what the analysis and the plan predict
  std::fill(joint, joint + (size_t)npairs * 3 * DD, 0.0);
  std::fill(rel, rel + (size_t)npairs * DD, 0.0);
  if (candidates) std::fill(gate, gate + (size_t)npairs * ngate, 0.0);
  typedef std::chrono::steady_clock Clock;
  auto ms_since = [](Clock::time_point t) { return 1e3 * std::chrono::duration<double>(Clock::now() - t).count(); };
  const int rc = hess_factor("pair_covariance", [&] { launch_cov_hessian_at(own_row(anchor)); }, out);
  if (rc < 0) return -1;
  out.outcome = rc != 0 ? PAIRS_NOT_PD : PAIRS_OK;
  if (rc != 0 || npairs == 0) return 0;
  auto t0 = Clock::now();
  // this call's buffers: the pairs' rows, the outputs (the batch and the plan's lists: pairs_solve_joint)
  std::vector<int> prow((size_t)2 * npairs);
  for (int k = 0; k < 2 * npairs; k++) prow[k] = own_row(pairs[k]);
  DevBuf<int> d_prow;
  DevBuf<double> d_joint, d_rel, d_gate, d_cand;
  d_prow.upload(prow);
  d_joint.alloc((size_t)npairs * 3 * DD);   // (zeroed: the anchor's blocks)
  d_rel.alloc((size_t)npairs * DD);
  if (candidates) {
    d_cand.upload(std::vector<double>(candidates, candidates + (size_t)npairs * ncand));
    d_gate.alloc((size_t)npairs * ngate);
  }
  if (pairs_solve_joint(pl, npairs, d_prow.p, d_joint.p, "pair_covariance") != 0) return -1;
  out.solve_ms = ms_since(t0);
  t0 = Clock::now();
  launch_pairs_gate(d, st_, npairs, d_prow.p, d_joint.p, c.X.p, candidates ? d_cand.p : nullptr, d_rel.p, candidates ? d_gate.p : nullptr);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(joint, d_joint.p, sizeof(double) * (size_t)npairs * 3 * DD, hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipMemcpyAsync(rel, d_rel.p, sizeof(double) * (size_t)npairs * DD, hipMemcpyDeviceToHost, st_));
  if (candidates) HIP_CHECK(hipMemcpyAsync(gate, d_gate.p, sizeof(double) * (size_t)npairs * ngate, hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
  out.gate_ms = ms_since(t0);
  out.outcome = PAIRS_OK;
  return 0;
}

int Group::pairs_vsolve_baseline(const double *X, int ld, int anchor, int ncols, double *ms) {
  if (cov_begin(X, ld, anchor) != 0) return -1;
  CovState &s = *cov_;
  PairsResult r;
  const long long n = (long long)cov_dof(d_) * P0_;
  if (pairs_setup(0, {8 * n, 8 * n}, 16, r) != 0) return -1;
  cert_prepare(X, ld, nullptr);
  launch_cov_hessian_at(own_row(anchor));
  if (spd_refactor_device(s.F, st_, false) != 0) return -1;
  DevBuf<double> x;
  x.alloc((size_t)n);
  std::vector<int> unk_h((size_t)ncols);
  for (int k = 0; k < ncols; k++) unk_h[k] = (int)((long long)k * 7919 % n);
  DevBuf<int> unk;
  unk.upload(unk_h);
  HIP_CHECK(hipStreamSynchronize(st_));
  const auto t0 = std::chrono::steady_clock::now();
  for (int k = 0; k < ncols; k++) {   // (enqueued as the block path enqueues a batch: a memset, k_pairs_rhs, the solve)
    HIP_CHECK(hipMemsetAsync(x.p, 0, sizeof(double) * (size_t)n, st_));
    launch_pairs_rhs(st_, unk.p, k, 1, x.p, 1);
    if (spd_vsolve_device(s.F, x.p, st_) != 0) return -1;
  }
  HIP_CHECK(hipStreamSynchronize(st_));
  *ms = 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}

}  // namespace dpgo
