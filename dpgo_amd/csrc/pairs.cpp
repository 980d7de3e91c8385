// Host side of the joint pair covariances (pairs.h): the column plan, the refusal, and the loop -- H written on the device
// (k_cov_hessian), factored (spd_refactor_device), the unit columns of the poses asked for solved batch by batch
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
  pl.batches = (pl.columns + PAIRS_BATCH - 1) / PAIRS_BATCH;
  pl.kb = 16 * ((std::min(std::max(pl.columns, 1), PAIRS_BATCH) + 15) / 16);
  return pl;
}

// The analysis (first call), the prediction, the refusal, the numeric context (first call that is not refused): polish_setup's
// rule on the bytes of the numeric phase, the block solve and this call's own buffers -- not on the blocks of the selected
// inversion.
int Group::pairs_setup(long long max_bytes, long long own_bytes, int kb, PairsResult &out, long long own_remain) {
  CovResult cr;
  if (cov_analyse(cr) != 0) return -1;
  CertState &c = *cert_;
  CovState &s = *cov_;
  const long long nblk = c.bptr_h[P0_];
  const long long numeric = (long long)spd_numeric_bytes(s.F, (long long)s.A.col.size()) + 4ll * nblk;
  const long long solve = (long long)spd_msolve_bytes(s.F, kb);
  out.unknowns = cr.unknowns;
  out.fronts = cr.fronts;
  out.levels = cr.levels;
  out.max_front = cr.max_front;
  out.symbolic_s = cr.symbolic_s;
  out.device_bytes = numeric + solve + own_bytes;
  out.outcome = PAIRS_SKIPPED;
  if (max_bytes > 0 && out.device_bytes > max_bytes) return 1;
  // against the free memory: the numeric phase only where no earlier call has left it (the solve's buffers are counted
  // whether an earlier call has left them or not)
  const long long remain = (s.F.numeric ? 0 : numeric) + solve + (own_remain < 0 ? own_bytes : own_remain);
  size_t free_b = 0, total_b = 0;
  HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
  if ((unsigned long long)remain > free_b / 2) return 1;   // (nothing that cannot fit is asked of a shared device)
  if (!s.F.numeric) {
    s.bcol.upload(s.bcol_h);
    if (spd_prepare_device(s.A, s.F) != 0) {
      fprintf(stderr, "[dpgo_amd] ERROR: pair_covariance: the device state of the factorisation could not be set up.\n");
      return -1;
    }
  }
  return 0;
}

// The batches of a column plan behind a factorisation that succeeded: per batch the unit right-hand sides, the block solve and the
// gather of the blocks whose columns it holds.  d_prow (2 npairs unified own rows) and d_joint (npairs x 3 dof^2, zeroed by the
// caller: the anchor's blocks) are the caller's, on the device, where joint stays; returns behind a synchronise.
int Group::pairs_solve_joint(const PairsPlan &pl, const std::vector<int> &row_of, int npairs, const int *d_prow, double *d_joint,
                             const char *who) {
  CovState &s = *cov_;
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
  for (int k = 0; k < 2 * npairs; k++)
    if (pairs[k] < 0 || pairs[k] >= N) {
      fprintf(stderr, "[dpgo_amd] ERROR: pair_covariance: pair %d names a pose that is not in the graph.\n", k / 2);
      return -1;
    }
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
  const int ready = pairs_setup(max_bytes, own, pl.kb, out);
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
  std::vector<int> row_of(N);
  for (int p = 0; p < N; p++) row_of[c.gid[p]] = p;
  typedef std::chrono::steady_clock Clock;
  auto ms_since = [](Clock::time_point t) { return 1e3 * std::chrono::duration<double>(Clock::now() - t).count(); };
  auto t0 = Clock::now();
  launch_cov_hessian(d, st_, N, c.bptr.p, s.bcol.p, c.Mval.p, c.Lam.p, c.X.p, row_of[anchor], spd_numeric_values(s.F));
  const int rc = spd_refactor_device(s.F, st_, false);   // (returns with the verdict read)
  if (rc != 0 && !s.F.not_pd) {
    fprintf(stderr, "[dpgo_amd] ERROR: pair_covariance: the factorisation failed on the device.\n");
    return -1;
  }
  out.pivot_max = s.F.pivot_max;
  out.pivot_min = s.F.pivot_max > 0 ? s.F.pivot_min : 0.0;
  out.factor_ms = ms_since(t0);
  if (rc != 0) {
    HIP_CHECK(hipStreamSynchronize(st_));
    out.outcome = PAIRS_NOT_PD;
    return 0;
  }
  if (npairs == 0) {
    out.outcome = PAIRS_OK;
    return 0;
  }
  t0 = Clock::now();
  // this call's buffers: the pairs' rows, the outputs (the batch and the plan's lists: pairs_solve_joint)
  std::vector<int> prow((size_t)2 * npairs);
  for (int k = 0; k < 2 * npairs; k++) prow[k] = row_of[pairs[k]];
  DevBuf<int> d_prow;
  DevBuf<double> d_joint, d_rel, d_gate, d_cand;
  d_prow.upload(prow);
  d_joint.alloc((size_t)npairs * 3 * DD);   // (zeroed: the anchor's blocks)
  d_rel.alloc((size_t)npairs * DD);
  if (candidates) {
    d_cand.upload(std::vector<double>(candidates, candidates + (size_t)npairs * ncand));
    d_gate.alloc((size_t)npairs * ngate);
  }
  if (pairs_solve_joint(pl, row_of, npairs, d_prow.p, d_joint.p, "pair_covariance") != 0) return -1;
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
  CertState &c = *cert_;
  CovState &s = *cov_;
  const int dof = cov_dof(d_), N = P0_;
  PairsResult r;
  const long long n = (long long)dof * N;
  if (pairs_setup(0, 8 * n, 16, r) != 0) return -1;
  cert_prepare(X, ld, nullptr);
  int arow = 0;
  for (int p = 0; p < N; p++)
    if (c.gid[p] == anchor) arow = p;
  launch_cov_hessian(d_, st_, N, c.bptr.p, s.bcol.p, c.Mval.p, c.Lam.p, c.X.p, arow, spd_numeric_values(s.F));
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
