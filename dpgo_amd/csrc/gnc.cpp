// Host side of graduated non-convexity (gnc.h): the outer loop.  The plan, the lists, the refusal and every launcher behind
// the weights are the robust objective's (robust.cpp); the inner solve is polish_loop (polish.cpp), once per level, with the
// weights of k_gnc_edge held fixed.  The optimiser's state is not touched (cert_begin).
#include "gnc.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

#include "cert_state.h"
#include "cov_state.h"
#include "gnc_math.h"
#include "group.h"
#include "robust_state.h"

namespace dpgo {

bool gnc_args_ok(int kind, double mu, double barc2, const char *who) {
  if (kind != GNC_TLS && kind != GNC_GM) {
    fprintf(stderr, "[dpgo_amd] ERROR: %s: kind %d is neither 0 (TLS) nor 1 (GM).\n", who, kind);
    return false;
  }
  if (!(std::isfinite(barc2) && barc2 > 0) || !(std::isfinite(mu) && mu > 0)) {
    fprintf(stderr, "[dpgo_amd] ERROR: %s: barc2 and mu must be finite and positive.\n", who);
    return false;
  }
  return true;
}

void Group::gnc_alloc() {
  RobustState &r = *rob_;
  if (r.gnc_on_device) return;
  r.gnc_partials.alloc((size_t)GNC_PARTIAL_SLOTS * r.plan.nb);
  r.gnc_counts.alloc((size_t)GNC_COUNT_SLOTS * r.plan.nb);
  r.gnc_sum.alloc(sizeof(GncSummaryDev) / sizeof(double));
  r.gnc_on_device = true;
}

void Group::gnc_pass(const double *Xdev, int kind, double mu, double c2, bool weigh, bool with_rows, int fslot) {
  RobustState &r = *rob_;
  const int nseg = std::max(T_.nseg_own, 1);
  const size_t m = (size_t)r.plan.m;
  launch_gnc_edge(d_, st_, r.plan.m, r.rec.p, Xdev, kind, mu, c2, weigh, r.out.p + 3 * m, r.out.p, with_rows ? r.rows.p : nullptr,
                  r.gnc_partials.p, reinterpret_cast<long long *>(r.gnc_counts.p), r.gnc_sum_dev(),
                  fslot >= 0 ? cert_->partials.p + (size_t)fslot * nseg : nullptr, nseg);
}

void Group::gnc_summary(GncSummaryDev &sd) {
  HIP_CHECK(hipMemcpyAsync(&sd, rob_->gnc_sum_dev(), sizeof(sd), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
}

int Group::gnc(const Graph &g, const double *X, int ld, const GncOptions &o, const int *robust_set, long long max_bytes, double *Xout,
               int ldout, double *weights, double *log, int log_cap, GncResult &out) {
  out = GncResult();
  const int rows = (d_ + 1) * num_poses_global_;
  const PolishOptions &po = o.inner;
  if (!gnc_args_ok(o.kind, 1.0, o.barc2, "gnc")) return -1;
  if (!X || !Xout || !weights || ld < rows || ldout < rows || !(o.mu_step > 1) || !std::isfinite(o.mu_step) || o.max_levels < 1 ||
      po.max_steps < 0 || po.max_tries < 1 || !(po.rel_tol >= 0) || !(po.grad_tol >= 0) || log_cap < 0 || (log_cap > 0 && !log)) {
    fprintf(stderr, "[dpgo_amd] ERROR: gnc: bad options or inconsistent size of the output.\n");
    return -1;
  }
  if (robust_begin(g, X, ld, 0, 1.0, 0, o.anchor, "gnc", robust_set) != 0) return -1;
  PolishResult pr;
  {
    const RobustState &r0 = *rob_;
    const int ready = polish_setup(max_bytes, pr, {r0.bytes + r0.gnc_bytes(), robust_remain() + (r0.gnc_on_device ? 0 : r0.gnc_bytes())});
    out.device_bytes = pr.device_bytes;
    out.symbolic_s = pr.symbolic_s;
    if (ready < 0) return -1;
    if (ready != 0) return 0;   // SKIPPED, with what the analysis predicts
  }
  robust_alloc();
  gnc_alloc();
  typedef std::chrono::steady_clock Clock;
  auto ms_since = [](Clock::time_point t) { return 1e3 * std::chrono::duration<double>(Clock::now() - t).count(); };
  const auto t_start = Clock::now();
  CertState &c = *cert_;
  CovState &s = *cov_;
  RobustState &r = *rob_;
  const int arow = own_row(o.anchor);
  const NodeMask all{all_bits(), nullptr};
  const size_t m = (size_t)r.plan.m;
  const int d = d_, L = edge_rec_doubles(d);
  const double c2 = o.barc2;
  double *wdev = r.out.p + 3 * m;
  std::vector<uint8_t> in_R(m);
  for (size_t e = 0; e < m; e++) {
    int i, j;
    bool f;
    edge_head(&r.plan.rec[e * L], i, j, f);
    in_R[e] = f;
    out.num_robust += f;
  }
  std::vector<double> w_cur(m, 1.0), w_prev(m, 1.0), Xa((size_t)rows * d), Xb((size_t)rows * d);
  HIP_CHECK(hipMemcpyAsync(wdev, w_cur.data(), sizeof(double) * m, hipMemcpyHostToDevice, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
  double mu = 1.0;   // (level 0: the surrogate's sum is not used)
  PolishHooks hooks;
  hooks.point = [&] {
    gnc_pass(c.X.p, o.kind, mu, c2, false, true, 1);
    launch_robust_gather(lc(all), r.inc_ptr.p, r.inc.p, wdev, r.rows.p, c.MX.p);
    launch_cert_lambda(lc(all), c.X.p, c.MX.p, c.Lam.p, nullptr, c.partials.p);
    launch_polish_grad(lc(all), c.X.p, c.MX.p, arow, s.pol_g.p, 0, 3, c.partials.p);   // (slot 3: nobody reads it, as robust_polish)
  };
  hooks.hessian = [&] { robust_hessian_launch(arow, 0); };
  hooks.trial = [&] { gnc_pass(c.V.p, o.kind, mu, c2, false, false, 2); };
  // one inner solve from `from` into `to`; the counts and the time are added up
  auto inner = [&](const double *from, int ldf, double *to, PolishResult &res) -> int {
    res = PolishResult();
    const int rc = polish_loop(from, ldf, arow, po, hooks, to, rows, nullptr, 0, res);
    out.steps += res.steps;
    out.factorisations += res.factorisations;
    out.inner_outcome = res.outcome;
    out.inner_ms += res.total_ms;
    return rc;
  };
  auto finish = [&](int outcome, const std::vector<double> &Xh, int ldh, const std::vector<double> &wh) {
    out.outcome = outcome;
    for (int col = 0; col < d; col++) std::memcpy(Xout + (size_t)col * ldout, Xh.data() + (size_t)col * ldh, sizeof(double) * rows);
    std::copy(wh.begin(), wh.end(), weights);
    out.total_ms = ms_since(t_start);
    return 0;
  };
  // level 0
  PolishResult res;
  if (inner(X, ld, Xa.data(), res) != 0) return -1;
  out.F_initial = res.F_initial;
  if (res.outcome == POLISH_STALLED) {
    for (int col = 0; col < d; col++) std::memcpy(Xa.data() + (size_t)col * rows, X + (size_t)col * ld, sizeof(double) * rows);
    return finish(GNC_INNER_FAILED, Xa, rows, w_cur);
  }
  GncSummaryDev sd;
  auto t0 = Clock::now();
  gnc_pass(c.X.p, o.kind, mu, c2, false, false, -1);   // (polish_loop leaves its final point in CertState's X)
  gnc_summary(sd);
  out.edge_ms += ms_since(t0);
  auto read_final = [&](const GncSummaryDev &q) {
    out.F_weighted_final = 0.5 * (q.sum_out + q.sum_ws);
    out.F_surrogate_final = 0.5 * (q.sum_out + q.sum_rho);
    out.num_zero = (int)q.num_zero;
    out.num_one = (int)q.num_one;
    out.num_between = (int)q.num_between;
    std::vector<double> sv(2 * m);
    HIP_CHECK(hipMemcpyAsync(sv.data(), r.out.p, sizeof(double) * 2 * m, hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
    out.num_outliers = 0;
    for (size_t e = 0; e < m; e++) out.num_outliers += in_R[e] && sv[e] + sv[m + e] > c2;
  };
  const double s_max0 = sd.s_max;
  out.s_max_initial = s_max0;
  if (out.num_robust == 0 || (o.kind == GNC_TLS && 2 * s_max0 <= c2)) {
    read_final(sd);
    out.F_surrogate_final = out.F_weighted_final;   // (unit weights: no surrogate was formed)
    return finish(GNC_ALL_INLIERS, Xa, rows, w_cur);
  }
  mu = o.kind == GNC_TLS ? c2 / (2 * s_max0 - c2) : std::max(1.0, 2 * s_max0 / c2);
  out.mu_initial = mu;
  std::vector<double> *Xprev = &Xa, *Xnext = &Xb;
  int outcome = GNC_MAX_LEVELS;
  for (int k = 1; k <= o.max_levels; k++) {
    t0 = Clock::now();
    w_prev = w_cur;
    gnc_pass(c.X.p, o.kind, mu, c2, true, false, -1);   // WEIGH at X_{k-1}
    HIP_CHECK(hipMemcpyAsync(w_cur.data(), wdev, sizeof(double) * m, hipMemcpyDeviceToHost, st_));
    GncSummaryDev sw;
    gnc_summary(sw);
    out.edge_ms += ms_since(t0);
    double *row = k - 1 < log_cap ? log + (size_t)(k - 1) * GNC_LOG_COLS : nullptr;
    if (row) {
      row[0] = mu;
      row[1] = 0.5 * (sw.sum_out + sw.sum_rho);
      row[2] = 0.5 * (sw.sum_out + sw.sum_ws);
      row[3] = row[4] = row[5] = 0.0;
      row[6] = POLISH_STALLED;
      row[7] = (double)sw.num_zero;
      row[8] = (double)sw.num_one;
      row[9] = (double)sw.num_between;
    }
    out.levels = k;
    out.mu_final = mu;
    if (inner(Xprev->data(), rows, Xnext->data(), res) != 0) return -1;
    if (row) {
      row[5] = res.steps;
      row[6] = res.outcome;
    }
    if (res.outcome == POLISH_STALLED) {
      // X_{k-1} and the weights it was solved with; the sums describe that pair at this level's mu
      HIP_CHECK(hipMemcpyAsync(wdev, w_prev.data(), sizeof(double) * m, hipMemcpyHostToDevice, st_));
      cert_upload(Xprev->data(), rows, d_, c.X.p);
      gnc_pass(c.X.p, o.kind, mu, c2, false, false, -1);
      gnc_summary(sd);
      read_final(sd);
      return finish(GNC_INNER_FAILED, *Xprev, rows, w_prev);
    }
    t0 = Clock::now();
    gnc_pass(c.X.p, o.kind, mu, c2, false, false, -1);   // evaluation only, the same mu, at X_k
    gnc_summary(sd);
    out.edge_ms += ms_since(t0);
    if (row) {
      row[3] = 0.5 * (sd.sum_out + sd.sum_ws);
      row[4] = 0.5 * (sd.sum_out + sd.sum_rho);
    }
    std::swap(Xprev, Xnext);
    if (o.kind == GNC_TLS ? sw.num_between == 0 : mu == 1.0) {
      outcome = GNC_CONVERGED;
      break;
    }
    mu = o.kind == GNC_TLS ? o.mu_step * mu : std::max(mu / o.mu_step, 1.0);
  }
  read_final(sd);
  return finish(outcome, *Xprev, rows, w_cur);
}

int Group::gnc_eval(const Graph &g, const double *X, int ld, int kind, double mu, double barc2, const int *robust_set, const double *w_in,
                    double *s_rot, double *s_trans, double *w, double *sums) {
  if (!X || !s_rot || !s_trans || !w || !sums || !gnc_args_ok(kind, mu, barc2, "gnc eval")) return -1;
  if (robust_begin(g, X, ld, 0, 1.0, 0, 0, "gnc eval", robust_set) != 0) return -1;
  if (!device_has_room(robust_remain() + (rob_->gnc_on_device ? 0 : rob_->gnc_bytes()))) {
    fprintf(stderr, "[dpgo_amd] ERROR: gnc eval: the buffers do not fit the device.\n");
    return -1;
  }
  robust_alloc();
  gnc_alloc();
  CertState &c = *cert_;
  RobustState &r = *rob_;
  const size_t m = (size_t)r.plan.m;
  cert_upload(X, ld, d_, c.X.p);
  HIP_CHECK(hipMemcpyAsync(r.out.p + 3 * m, w_in ? w_in : w, sizeof(double) * m, hipMemcpyHostToDevice, st_));
  gnc_pass(c.X.p, kind, mu, barc2, w_in == nullptr, false, -1);
  std::vector<double> eo(4 * m);
  HIP_CHECK(hipMemcpyAsync(eo.data(), r.out.p, sizeof(double) * 4 * m, hipMemcpyDeviceToHost, st_));
  GncSummaryDev sd;
  gnc_summary(sd);   // (synchronises)
  std::copy(eo.begin(), eo.begin() + m, s_rot);
  std::copy(eo.begin() + m, eo.begin() + 2 * m, s_trans);
  std::copy(eo.begin() + 3 * m, eo.end(), w);
  const double v[8] = {sd.sum_out, sd.sum_ws, sd.sum_rho, sd.s_max, sd.w_min, (double)sd.num_zero, (double)sd.num_one, (double)sd.num_between};
  std::copy(v, v + 8, sums);
  return 0;
}

// ---- host only ----
int gnc_weight_host(int kind, double mu, double c2, const double *s, int n, double *w, double *rho) {
  if (n < 0 || (n > 0 && (!s || !w || !rho)) || !gnc_args_ok(kind, mu, c2, "gnc weight debug")) return -1;
  for (int k = 0; k < n; k++) {
    if (!(s[k] >= 0)) return -1;
    gnc_weight_rho(kind, mu, c2, s[k], w[k], rho[k]);
  }
  return 0;
}

}  // namespace dpgo
