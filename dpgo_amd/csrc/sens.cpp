// Host side of the measurement sensitivities (sens.h): the graph against the group, the refusal's own part, and the loop -- H
// written on the device (k_cov_hessian) and factored (hess.cpp: hess_factor), the upstream columns solved batch by batch
// (spd_msolve_device), the per-edge derivatives of every column (k_sens_edge).  The upstream's check and the batch loop are
// shared with the robust objective's sensitivities (rsens.cpp), which pass their own edge step.  The matrix, its symbolic
// analysis and its numeric context are the covariance's (cov.cpp), the refusal is the block solves' (pairs.cpp: pairs_setup),
// the edge records are the robust objective's (robust.cpp: graph_records_own).  The optimiser's state is not touched
// (cert_begin).
#include "sens.h"

#include <algorithm>
#include <chrono>
#include <cmath>

#include "cert_state.h"
#include "cov_state.h"
#include "edges.h"
#include "group.h"
#include "sens_math.h"

namespace dpgo {

static int sens_kb(int k) { return 16 * ((std::min(k, SENS_BATCH) + 15) / 16); }

// The upstream array of a call, and its sizes: columns and batches into out.  Returns kb, the row length of the batch array
// (the columns of the largest batch rounded up to 16), or -1.
int Group::sens_begin(const char *who, const double *upstream, int ldu, int k, SensResult &out) {
  const long long n = (long long)cov_dof(d_) * P0_;
  if (ldu < n) {
    fprintf(stderr, "[dpgo_amd] ERROR: %s: the upstream array has fewer than dof N = %lld rows.\n", who, n);
    return -1;
  }
  for (int l = 0; l < k; l++)
    for (long long u = 0; u < n; u++)
      if (!std::isfinite(upstream[(size_t)l * ldu + u])) {
        fprintf(stderr, "[dpgo_amd] ERROR: %s: upstream column %d has an entry that is not finite.\n", who, l);
        return -1;
      }
  out.columns = k;
  out.batches = (k + SENS_BATCH - 1) / SENS_BATCH;
  return sens_kb(k);
}

// The batches behind a factorisation that succeeded: per batch the upload of its upstream columns, the right-hand sides, the
// block solve and the adjoint's read-out (solve_ms), then the caller's edge step on the solved columns (edge_ms), which ends
// behind a synchronise.
int Group::sens_batches(const char *who, int anchor, const double *upstream, int ldu, int k, double *adjoint,
                        const std::function<void(const SensBatch &)> &edge, SensResult &out) {
  CertState &c = *cert_;
  CovState &s = *cov_;
  const int dof = cov_dof(d_), N = P0_, ncmax = std::min(k, SENS_BATCH), kb = sens_kb(k);
  const long long n = (long long)dof * N;
  typedef std::chrono::steady_clock Clock;
  auto ms_since = [](Clock::time_point t) { return 1e3 * std::chrono::duration<double>(Clock::now() - t).count(); };
  DevBuf<int> d_row_of, d_gid;
  DevBuf<double> d_Xb, d_U;
  d_row_of.upload(c.row_of);
  d_gid.upload(c.gid);
  d_Xb.alloc((size_t)n * kb, false);
  d_U.alloc((size_t)n * ncmax, false);
  std::vector<double> packed;
  for (int b = 0; b < out.batches; b++) {
    const int c0 = b * SENS_BATCH, nc = std::min(SENS_BATCH, k - c0);
    auto t0 = Clock::now();
    const double *src = upstream + (size_t)c0 * ldu;
    if (ldu != n) {   // the columns of this batch, packed
      packed.resize((size_t)n * nc);
      for (int j = 0; j < nc; j++) std::copy(src + (size_t)j * ldu, src + (size_t)j * ldu + n, packed.begin() + (size_t)j * n);
      src = packed.data();
    }
    HIP_CHECK(hipMemcpyAsync(d_U.p, src, sizeof(double) * (size_t)n * nc, hipMemcpyHostToDevice, st_));
    HIP_CHECK(hipMemsetAsync(d_Xb.p, 0, sizeof(double) * (size_t)n * kb, st_));
    launch_sens_rhs(st_, dof, N, d_row_of.p, anchor, d_U.p, nc, d_Xb.p, kb);
    if (spd_msolve_device(s.F, d_Xb.p, nc, kb, st_) != 0) {
      fprintf(stderr, "[dpgo_amd] ERROR: %s: the solve failed on the device.\n", who);
      return -1;
    }
    if (adjoint) {   // (the upstream's buffer has been read: it takes lambda by global pose)
      launch_sens_adjoint(st_, dof, N, d_gid.p, anchor, d_Xb.p, kb, nc, d_U.p);
      HIP_CHECK(hipMemcpyAsync(adjoint + (size_t)c0 * n, d_U.p, sizeof(double) * (size_t)n * nc, hipMemcpyDeviceToHost, st_));
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(st_));
    out.solve_ms += ms_since(t0);
    t0 = Clock::now();
    edge({b, c0, nc, kb, d_Xb.p});
    out.edge_ms += ms_since(t0);
  }
  out.outcome = SENS_OK;
  return 0;
}

int Group::sensitivity(const Graph &g, const double *X, int ld, int anchor, long long max_bytes, const double *upstream, int ldu,
                       int k, double *adjoint, double *sens, SensResult &out) {
  out = SensResult();
  if (!upstream || !sens || k < 1) {
    fprintf(stderr, "[dpgo_amd] ERROR: sensitivity: missing upstream or output arrays, or no column.\n");
    return -1;
  }
  if (cov_begin(X, ld, anchor) != 0) return -1;
  const int kb = sens_begin("sensitivity", upstream, ldu, k, out);
  std::vector<double> rec;
  if (kb < 0 || graph_records_own(g, "sensitivity", rec) != 0) return -1;
  const int d = d_, dof = cov_dof(d), N = P0_, NO = 2 + dof, m = (int)g.all.size(), L = edge_rec_doubles(d);
  const int ncmax = std::min(k, SENS_BATCH);
  const long long n = (long long)dof * N;
  out.edges = m;
  // this call's buffers: the batch, one batch of upstream, one batch of per-edge output, the edge records, the two row lists
  const long long own = 8ll * (n * kb + n * ncmax + (long long)ncmax * m * NO + (long long)m * L) + 4ll * 2 * N;
  const int ready = pairs_setup(max_bytes, {own, own}, kb, out);
  if (ready < 0) return -1;
  cert_prepare(X, ld, &out.stationarity);
  if (ready != 0) return 0;   // SKIPPED, with what the analysis and the sizes predict
  std::fill(sens, sens + (size_t)k * m * NO, 0.0);
  if (adjoint) std::fill(adjoint, adjoint + (size_t)k * n, 0.0);
  const int rc = hess_factor("sensitivity", [&] { launch_cov_hessian_at(own_row(anchor)); }, out);
  if (rc < 0) return -1;
  if (rc != 0) {
    out.outcome = SENS_NOT_PD;
    return 0;
  }
  DevBuf<double> d_rec, d_out;
  d_rec.upload(rec);
  d_out.alloc((size_t)ncmax * m * NO, false);
  return sens_batches("sensitivity", anchor, upstream, ldu, k, adjoint, [&](const SensBatch &b) {
    launch_sens_edge(d, st_, m, d_rec.p, cert_->X.p, b.Xb, b.kb, b.nc, d_out.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(sens + (size_t)b.c0 * m * NO, d_out.p, sizeof(double) * (size_t)b.nc * m * NO, hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
  }, out);
}

// ---- host only: the per-edge arithmetic of k_sens_edge through sens_math.h ----
int sens_edge_host(const Graph &g, const double *X, int ld, const double *lambda, double *sens, double *phi) {
  const int d = g.d, N = g.num_poses, m = (int)g.all.size();
  if ((d != 2 && d != 3) || N <= 0 || m == 0 || !X || ld < (d + 1) * N || !lambda || !sens) return -1;
  for (const Measurement &mm : g.all)
    if (mm.ipose < 0 || mm.ipose >= N || mm.jpose < 0 || mm.jpose >= N) return -1;
  std::vector<double> rec, pose((size_t)N * pose_rec_doubles(d));
  edge_records(g, rec);
  pose_records(d, N, X, ld, pose.data());
  const int L = edge_rec_doubles(d), RS = pose_rec_doubles(d), dof = cov_dof(d), NO = 2 + dof;
  for (int e = 0; e < m; e++) {
    const double *q = rec.data() + (size_t)e * L;
    int i, j;
    bool inter;
    edge_head(q, i, j, inter);
    const double *a = pose.data() + (size_t)i * RS, *b = pose.data() + (size_t)j * RS;
    const double *li = lambda + (size_t)dof * i, *lj = lambda + (size_t)dof * j;
    double *o = sens + (size_t)e * NO, *ph = phi ? phi + e : nullptr;
    if (d == 2) sens_one<2>(q, a, b, li, lj, o, ph);
    else sens_one<3>(q, a, b, li, lj, o, ph);
  }
  return 0;
}

}  // namespace dpgo
