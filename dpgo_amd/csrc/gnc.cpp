// Host side of graduated non-convexity (gnc.h): the outer loop, gnc_loop, for this objective and for the maximum-likelihood
// one (ml_gnc.cpp), and this objective's description of itself.  The plan, the lists, the refusal and every launcher behind the
// weights are the robust objective's (robust.cpp); the inner solve is polish_loop (polish.cpp), once per level, with the
// weights of the edge pass held fixed.  The optimiser's state is not touched (cert_begin).
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

void Group::gnc_summary(GncSummary &q) {
  HIP_CHECK(hipMemcpyAsync(&q.sums, rob_->gnc_sum_dev(), sizeof(q.sums), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
}

void gnc_summary_doubles(const GncSummary &q, int n, double *sums) {
  const GncSummaryDev &u = q.sums;
  const double v[ML_GNC_SUMS] = {u.sum_out, u.sum_ws, u.sum_rho, u.s_max, u.w_min, (double)u.num_zero, (double)u.num_one,
                                 (double)u.num_between, (double)q.near_pi, (double)q.near_pi_all};
  std::copy(v, v + n, sums);
}

int gnc_robust_mask(int d, int m, const double *rec, const int *robust_set, std::vector<int> &in_R) {
  const int L = edge_rec_doubles(d);
  in_R.resize(m);
  int count = 0;
  for (int e = 0; e < m; e++) {
    int i, j;
    bool f;
    edge_head(rec + (size_t)e * L, i, j, f);
    in_R[e] = robust_set ? robust_set[e] != 0 : f;
    count += in_R[e];
  }
  return count;
}

int Group::gnc_loop(const char *who, const double *X, int ld, const GncOptions &o, const GncObjective &ob, double *Xout, int ldout,
                    double *weights, double *log, int log_cap, GncResult &out, GncSummary *last) {
  const int rows = (d_ + 1) * num_poses_global_;
  const PolishOptions &po = o.inner;
  if (!gnc_args_ok(o.kind, 1.0, o.barc2, who)) return -1;
  if (!X || !Xout || !weights || ld < rows || ldout < rows || !(o.mu_step > 1) || !std::isfinite(o.mu_step) || o.max_levels < 1 ||
      po.max_steps < 0 || po.max_tries < 1 || !(po.rel_tol >= 0) || !(po.grad_tol >= 0) || log_cap < 0 || (log_cap > 0 && !log)) {
    fprintf(stderr, "[dpgo_amd] ERROR: %s: bad options or inconsistent size of the output.\n", who);
    return -1;
  }
  typedef std::chrono::steady_clock Clock;
  auto ms_since = [](Clock::time_point t) { return 1e3 * std::chrono::duration<double>(Clock::now() - t).count(); };
  const auto t_start = Clock::now();
  CertState &c = *cert_;
  const int arow = own_row(o.anchor);
  const size_t m = ob.in_R.size();
  const int d = d_;
  const double c2 = o.barc2;
  out.num_robust = ob.num_robust;
  std::vector<double> w_cur(m, 1.0), w_prev(m, 1.0), Xa((size_t)rows * d), Xb((size_t)rows * d);
  HIP_CHECK(hipMemcpyAsync(ob.wdev, w_cur.data(), sizeof(double) * m, hipMemcpyHostToDevice, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
  double mu = 1.0;   // (level 0: the surrogate's sum is not used)
  PolishHooks hooks;
  hooks.point = [&] {
    ob.pass(c.X.p, mu, false, true, 1);
    ob.gradient();
  };
  hooks.hessian = ob.hessian;
  hooks.trial = [&] { ob.pass(c.V.p, mu, false, false, 2); };
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
  // The sums of q describe the returned pair.  s per edge is what the last per-edge-writing pass left: for an objective whose
  // evaluation passes write none, on every exit of polish_loop but STALLED that pass ran at the point the loop hands out.
  auto read_final = [&](const GncSummary &q) {
    out.F_weighted_final = 0.5 * (q.sums.sum_out + q.sums.sum_ws);
    out.F_surrogate_final = 0.5 * (q.sums.sum_out + q.sums.sum_rho);
    out.num_zero = (int)q.sums.num_zero;
    out.num_one = (int)q.sums.num_one;
    out.num_between = (int)q.sums.num_between;
    if (last) *last = q;
    std::vector<double> sv(m);
    ob.edge_s(sv.data());
    out.num_outliers = 0;
    for (size_t e = 0; e < m; e++) out.num_outliers += ob.in_R[e] && sv[e] > c2;
  };
  auto finish = [&](int outcome, const std::vector<double> &Xh, const std::vector<double> &wh) {
    out.outcome = outcome;
    for (int col = 0; col < d; col++) std::memcpy(Xout + (size_t)col * ldout, Xh.data() + (size_t)col * rows, sizeof(double) * rows);
    std::copy(wh.begin(), wh.end(), weights);
    out.total_ms = ms_since(t_start);
    return 0;
  };
  // after an inner stall: Xh and the weights it was solved with go back; the sums describe that pair at this level's mu
  auto failed = [&](const std::vector<double> &Xh, const std::vector<double> &wh) {
    GncSummary q;
    HIP_CHECK(hipMemcpyAsync(ob.wdev, wh.data(), sizeof(double) * m, hipMemcpyHostToDevice, st_));
    cert_upload(Xh.data(), rows, d_, c.X.p);
    ob.pass(c.X.p, mu, false, ob.failure_per_edge, -1);
    ob.summary(q, ob.failure_per_edge);
    read_final(q);
    return finish(GNC_INNER_FAILED, Xh, wh);
  };
  // an evaluation-only pass at CertState's X, where polish_loop leaves its final point
  auto evaluate = [&](GncSummary &q) {
    ob.pass(c.X.p, mu, false, false, -1);
    ob.summary(q, false);
  };
  // level 0
  PolishResult res;
  if (inner(X, ld, Xa.data(), res) != 0) return -1;
  out.F_initial = res.F_initial;
  if (res.outcome == POLISH_STALLED) {
    for (int col = 0; col < d; col++) std::memcpy(Xa.data() + (size_t)col * rows, X + (size_t)col * ld, sizeof(double) * rows);
    return ob.level0_stall_evaluated ? failed(Xa, w_cur) : finish(GNC_INNER_FAILED, Xa, w_cur);
  }
  GncSummary sd;
  auto t0 = Clock::now();
  evaluate(sd);
  out.edge_ms += ms_since(t0);
  const double s_max0 = sd.sums.s_max;
  out.s_max_initial = s_max0;
  if (out.num_robust == 0 || (o.kind == GNC_TLS && 2 * s_max0 <= c2)) {
    read_final(sd);
    out.F_surrogate_final = out.F_weighted_final;   // (unit weights: no surrogate was formed)
    return finish(GNC_ALL_INLIERS, Xa, w_cur);
  }
  mu = o.kind == GNC_TLS ? c2 / (2 * s_max0 - c2) : std::max(1.0, 2 * s_max0 / c2);
  out.mu_initial = mu;
  std::vector<double> *Xprev = &Xa, *Xnext = &Xb;
  int outcome = GNC_MAX_LEVELS;
  for (int k = 1; k <= o.max_levels; k++) {
    t0 = Clock::now();
    w_prev = w_cur;
    GncSummary sw;
    ob.pass(c.X.p, mu, true, false, -1);   // WEIGH at X_{k-1}
    HIP_CHECK(hipMemcpyAsync(w_cur.data(), ob.wdev, sizeof(double) * m, hipMemcpyDeviceToHost, st_));
    ob.summary(sw, false);
    out.edge_ms += ms_since(t0);
    double *row = k - 1 < log_cap ? log + (size_t)(k - 1) * GNC_LOG_COLS : nullptr;
    if (row) {
      row[0] = mu;
      row[1] = 0.5 * (sw.sums.sum_out + sw.sums.sum_rho);
      row[2] = 0.5 * (sw.sums.sum_out + sw.sums.sum_ws);
      row[3] = row[4] = row[5] = 0.0;
      row[6] = POLISH_STALLED;
      row[7] = (double)sw.sums.num_zero;
      row[8] = (double)sw.sums.num_one;
      row[9] = (double)sw.sums.num_between;
    }
    out.levels = k;
    out.mu_final = mu;
    if (inner(Xprev->data(), rows, Xnext->data(), res) != 0) return -1;
    if (row) {
      row[5] = res.steps;
      row[6] = res.outcome;
    }
    // (an inner MAX_STEPS is a level like any other: its point is the last accepted one, and F_w has not increased)
    if (res.outcome == POLISH_STALLED) return failed(*Xprev, w_prev);
    t0 = Clock::now();
    evaluate(sd);   // the same mu, at X_k
    out.edge_ms += ms_since(t0);
    if (row) {
      row[3] = 0.5 * (sd.sums.sum_out + sd.sums.sum_ws);
      row[4] = 0.5 * (sd.sums.sum_out + sd.sums.sum_rho);
    }
    std::swap(Xprev, Xnext);
    if (o.kind == GNC_TLS ? sw.sums.num_between == 0 : mu == 1.0) {
      outcome = GNC_CONVERGED;
      break;
    }
    mu = o.kind == GNC_TLS ? o.mu_step * mu : std::max(mu / o.mu_step, 1.0);
  }
  read_final(sd);
  return finish(outcome, *Xprev, w_cur);
}

int Group::gnc(const Graph &g, const double *X, int ld, const GncOptions &o, const int *robust_set, long long max_bytes, double *Xout,
               int ldout, double *weights, double *log, int log_cap, GncResult &out) {
  out = GncResult();
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
  CertState &c = *cert_;
  CovState &s = *cov_;
  RobustState &r = *rob_;
  const int arow = own_row(o.anchor);
  const NodeMask all{all_bits(), nullptr};
  const size_t m = (size_t)r.plan.m;
  GncObjective ob;
  ob.wdev = r.out.p + 3 * m;
  ob.num_robust = gnc_robust_mask(d_, r.plan.m, r.plan.rec.data(), nullptr, ob.in_R);   // (robust_begin wrote robust_set into the records)
  ob.pass = [&](const double *Xdev, double mu, bool weigh, bool with_rows, int fslot) {
    gnc_pass(Xdev, o.kind, mu, o.barc2, weigh, with_rows, fslot);
  };
  ob.summary = [&](GncSummary &q, bool) { gnc_summary(q); };
  ob.gradient = [&] {
    launch_robust_gather(lc(all), r.inc_ptr.p, r.inc.p, ob.wdev, r.rows.p, c.MX.p);
    launch_cert_lambda(lc(all), c.X.p, c.MX.p, c.Lam.p, nullptr, c.partials.p);
    launch_polish_grad(lc(all), c.X.p, c.MX.p, arow, s.pol_g.p, 0, 3, c.partials.p);   // (slot 3: nobody reads it, as robust_polish)
  };
  ob.hessian = [&] { robust_hessian_launch(arow, 0); };
  ob.edge_s = [&](double *sv) {   // s_rot + s_trans, the rounded sum of the two rounded parts as the kernel forms it
    std::vector<double> parts(2 * m);
    HIP_CHECK(hipMemcpyAsync(parts.data(), r.out.p, sizeof(double) * 2 * m, hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
    for (size_t e = 0; e < m; e++) sv[e] = parts[e] + parts[m + e];
  };
  return gnc_loop("gnc", X, ld, o, ob, Xout, ldout, weights, log, log_cap, out);
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
  GncSummary sd;
  gnc_summary(sd);   // (synchronises)
  std::copy(eo.begin(), eo.begin() + m, s_rot);
  std::copy(eo.begin() + m, eo.begin() + 2 * m, s_trans);
  std::copy(eo.begin() + 3 * m, eo.end(), w);
  gnc_summary_doubles(sd, GNC_SUMS, sums);
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
