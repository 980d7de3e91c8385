// Host side of the sensitivities of the robust objective (rsens.h): sens.cpp's loop on the TRUE robust Hessian.  The lists,
// the edge pass and the Hessian are the robust objective's (robust.cpp: robust_begin, robust_eval, robust_hessian_launch), the
// matrix, its analysis and the refusal are the pair covariances' (pairs.cpp: pairs_setup, with the robust buffers behind the
// same refusal), the right-hand sides and the adjoint's read-out are sens.hip's.  The optimiser's state is not touched.
#include "rsens.h"

#include <algorithm>
#include <chrono>
#include <cmath>

#include "cert_state.h"
#include "cov_state.h"
#include "edges.h"
#include "group.h"
#include "robust_math.h"
#include "robust_state.h"
#include "rsens_math.h"
#include "sens_math.h"

namespace dpgo {

int Group::robust_sensitivity(const Graph &g, const double *X, int ld, int loss, double loss_reg, int anchor, long long max_bytes,
                              const double *upstream, int ldu, int k, double *adjoint, double *sens, double *dloss_reg,
                              SensResult &out) {
  out = SensResult();
  if (!upstream || !sens || !dloss_reg || k < 1) {
    fprintf(stderr, "[dpgo_amd] ERROR: robust sensitivity: missing upstream or output arrays, or no column.\n");
    return -1;
  }
  if (robust_begin(g, X, ld, loss, loss_reg, 1, anchor, "robust sensitivity") != 0) return -1;
  const int d = d_, dof = cov_dof(d), N = P0_, NO = 3 + dof;
  const long long n = (long long)dof * N;
  if (ldu < n) {
    fprintf(stderr, "[dpgo_amd] ERROR: robust sensitivity: the upstream array has fewer than dof N = %lld rows.\n", n);
    return -1;
  }
  for (int l = 0; l < k; l++)
    for (long long u = 0; u < n; u++)
      if (!std::isfinite(upstream[(size_t)l * ldu + u])) {
        fprintf(stderr, "[dpgo_amd] ERROR: robust sensitivity: upstream column %d has an entry that is not finite.\n", l);
        return -1;
      }
  CertState &c = *cert_;
  const int m = rob_->plan.m;
  const int batches = (k + SENS_BATCH - 1) / SENS_BATCH, kb = 16 * ((std::min(k, SENS_BATCH) + 15) / 16);
  const int ncmax = std::min(k, SENS_BATCH);
  out.columns = k;
  out.batches = batches;
  out.edges = m;
  // this call's buffers: the batch, one batch of upstream, one batch of per-edge output, the preparation array, the two row
  // lists; behind them the robust objective's, which an earlier call may have left on the device
  const long long own = 8ll * (n * kb + n * ncmax + (long long)ncmax * m * NO + (long long)m * NO) + 4ll * 2 * N;
  PairsResult pr;
  const int ready = pairs_setup(max_bytes, own + rob_->bytes, kb, pr, own + robust_remain());
  if (ready < 0) return -1;
  out.unknowns = pr.unknowns;
  out.fronts = pr.fronts;
  out.levels = pr.levels;
  out.max_front = pr.max_front;
  out.symbolic_s = pr.symbolic_s;
  out.device_bytes = pr.device_bytes;
  if (ready != 0) return 0;   // SKIPPED: nothing allocated, nothing written, the stationarity not computed
  robust_alloc();
  CovState &s = *cov_;
  RobustState &r = *rob_;
  std::vector<int> row_of(N);
  for (int p = 0; p < N; p++) row_of[c.gid[p]] = p;
  const int arow = row_of[anchor];
  const NodeMask all{all_bits(), nullptr};
  cert_upload(X, ld, d, c.X.p);
  robust_eval(c.X.p, loss, loss_reg, true, -1);
  launch_robust_gather(lc(all), r.inc_ptr.p, r.inc.p, r.out.p + 3 * (size_t)m, r.rows.p, c.MX.p);
  launch_cert_lambda(lc(all), c.X.p, c.MX.p, c.Lam.p, nullptr, c.partials.p);
  launch_cert_reduce(st_, T_, 1, c.partials.p, c.h_sums, sched_.flag());
  wait_flag(sched_.last_seq());
  out.stationarity = std::sqrt(c.h_sums[0]);   // |S_w X|_F
  std::fill(sens, sens + (size_t)k * m * NO, 0.0);
  std::fill(dloss_reg, dloss_reg + k, 0.0);
  if (adjoint) std::fill(adjoint, adjoint + (size_t)k * n, 0.0);
  typedef std::chrono::steady_clock Clock;
  auto ms_since = [](Clock::time_point t) { return 1e3 * std::chrono::duration<double>(Clock::now() - t).count(); };
  auto t0 = Clock::now();
  robust_hessian_launch(arow, 1);
  const int rc = spd_refactor_device(s.F, st_, false);   // (returns with the verdict read)
  if (rc != 0 && !s.F.not_pd) {
    fprintf(stderr, "[dpgo_amd] ERROR: robust sensitivity: the factorisation failed on the device.\n");
    return -1;
  }
  out.pivot_max = s.F.pivot_max;
  out.pivot_min = s.F.pivot_max > 0 ? s.F.pivot_min : 0.0;
  out.factor_ms = ms_since(t0);
  if (rc != 0) {
    HIP_CHECK(hipStreamSynchronize(st_));
    out.outcome = SENS_NOT_PD;
    return 0;
  }
  DevBuf<int> d_row_of, d_gid;
  DevBuf<double> d_prep, d_Xb, d_U, d_out;
  d_row_of.upload(row_of);
  d_gid.upload(c.gid);
  d_prep.alloc((size_t)m * NO, false);
  d_Xb.alloc((size_t)n * kb, false);
  d_U.alloc((size_t)n * ncmax, false);
  d_out.alloc((size_t)ncmax * m * NO, false);
  std::vector<double> packed;
  for (int b = 0; b < batches; b++) {
    const int c0 = b * SENS_BATCH, nc = std::min(SENS_BATCH, k - c0);
    t0 = Clock::now();
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
      fprintf(stderr, "[dpgo_amd] ERROR: robust sensitivity: the solve failed on the device.\n");
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
    if (b == 0) launch_rsens_prep(d, st_, m, r.rec.p, c.X.p, r.out.p, loss, loss_reg, d_prep.p);   // once: every batch reads it
    launch_rsens_edge(d, st_, m, r.rec.p, c.X.p, r.out.p, d_prep.p, d_Xb.p, kb, nc, d_out.p);
    HIP_CHECK(hipGetLastError());
    double *dst = sens + (size_t)c0 * m * NO;
    HIP_CHECK(hipMemcpyAsync(dst, d_out.p, sizeof(double) * (size_t)nc * m * NO, hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
    // dL/ddelta: the edges' terms in ascending order, one column per thread (a column's sum is one thread's, in order)
#pragma omp parallel for schedule(static) if ((long long)nc * m > 65536)
    for (int j = 0; j < nc; j++) {
      double sum = 0;
      for (int e = 0; e < m; e++) sum += dst[((size_t)j * m + e) * NO + NO - 1];
      dloss_reg[c0 + j] = sum;
    }
    out.edge_ms += ms_since(t0);
  }
  out.outcome = SENS_OK;
  return 0;
}

// ---- host only: the per-edge arithmetic of k_rsens_prep and k_rsens_edge through rsens_math.h ----
template <int D>
static void rsens_edge_one(const double *q, const double *a, const double *b, bool inter, int loss, double dl, const double *li,
                           const double *lj, double *o, double *ph) {
  constexpr int NO = 2 + D + D * (D - 1) / 2;
  double v[4], ds[NO], so[NO], phi;
  edge_lane<D>(q, a, b, inter, loss, dl, v);
  const double s = v[0] + v[1], w = v[3];
  rsens_ds<D>(q, a, b, ds);
  sens_one<D>(q, a, b, li, lj, so, &phi);
  rsens_combine<D>(w, robust_curv(loss, dl, s, w, inter), phi, ds, rsens_dw(loss, dl, s, w, inter), so, o);
  if (ph) *ph = phi;
}

int robust_sens_edge_host(const Graph &g, const double *X, int ld, int loss, double loss_reg, const double *lambda, double *sens,
                          double *phi) {
  const int d = g.d, N = g.num_poses, m = (int)g.all.size();
  if ((d != 2 && d != 3) || N <= 0 || m == 0 || !X || ld < (d + 1) * N || !lambda || !sens) return -1;
  if (loss < 0 || loss > 3 || (loss != 0 && !(std::isfinite(loss_reg) && loss_reg > 0))) return -1;
  for (const Measurement &mm : g.all)
    if (mm.ipose < 0 || mm.ipose >= N || mm.jpose < 0 || mm.jpose >= N) return -1;
  std::vector<double> rec, pose((size_t)N * pose_rec_doubles(d));
  edge_records(g, rec);
  pose_records(d, N, X, ld, pose.data());
  const int L = edge_rec_doubles(d), RS = pose_rec_doubles(d), dof = cov_dof(d), NO = 3 + dof;
  for (int e = 0; e < m; e++) {
    const double *q = rec.data() + (size_t)e * L;
    int i, j;
    bool inter;
    edge_head(q, i, j, inter);
    const double *a = pose.data() + (size_t)i * RS, *b = pose.data() + (size_t)j * RS;
    const double *li = lambda + (size_t)dof * i, *lj = lambda + (size_t)dof * j;
    double *o = sens + (size_t)e * NO, *ph = phi ? phi + e : nullptr;
    if (d == 2) rsens_edge_one<2>(q, a, b, inter, loss, loss_reg, li, lj, o, ph);
    else rsens_edge_one<3>(q, a, b, inter, loss, loss_reg, li, lj, o, ph);
  }
  return 0;
}

}  // namespace dpgo
