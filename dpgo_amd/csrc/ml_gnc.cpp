// Host side of graduated non-convexity on the maximum-likelihood objective (ml_gnc.h): the outer loop of gnc.cpp on chi2.  The
// plan, the lists, Omega's check and the refusal are the ML objective's (ml.cpp); the inner solve is polish_loop (polish.cpp),
// once per level, with the weights of k_ml_gnc_edge held fixed; the gather and the Hessian kernel are ml.hip's, unchanged.  The
// optimiser's state is not touched (cert_begin).
#include "ml_gnc.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

#include "cert_state.h"
#include "cov_state.h"
#include "edge_math.h"
#include "gnc_math.h"
#include "group.h"
#include "ml_gnc_math.h"
#include "ml_state.h"

namespace dpgo {

void Group::ml_gnc_alloc() {
  MlState &n = *ml_;
  if (n.gnc_on_device) return;
  n.gnc_w.alloc((size_t)n.plan.m);
  n.gnc_in_R.alloc((size_t)n.plan.m);
  n.gnc_partials.alloc((size_t)ML_GNC_PARTIAL_SLOTS * n.plan.nb);
  n.gnc_counts.alloc((size_t)ML_GNC_COUNT_SLOTS * n.plan.nb);
  n.gnc_sum.alloc(2 * sizeof(MlGncSummaryDev) / sizeof(double));
  n.gnc_on_device = true;
}

// R of this call: robust_set, or the inter word of the plan's records; uploaded (the stream is synchronised).  Returns |R|.
int Group::ml_gnc_set(const int *robust_set, std::vector<int> &in_R) {
  MlState &n = *ml_;
  const size_t m = (size_t)n.plan.m;
  const int L = edge_rec_doubles(d_);
  in_R.resize(m);
  int count = 0;
  for (size_t e = 0; e < m; e++) {
    int i, j;
    bool f;
    edge_head(&n.plan.rec[e * L], i, j, f);
    in_R[e] = robust_set ? robust_set[e] != 0 : f;
    count += in_R[e];
  }
  HIP_CHECK(hipMemcpyAsync(n.gnc_in_R.p, in_R.data(), sizeof(int) * m, hipMemcpyHostToDevice, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
  return count;
}

void Group::ml_gnc_pass(const double *Xdev, int kind, double mu, double c2, bool weigh, bool full, int fslot) {
  MlState &n = *ml_;
  const int nseg = std::max(T_.nseg_own, 1);
  launch_ml_gnc_edge(d_, st_, n.plan.m, n.rec.p, n.om.p, Xdev, n.gnc_in_R.p, kind, mu, c2, weigh, n.gnc_w.p, full ? n.out() : MlEdgeOut(),
                     n.gnc_partials.p, reinterpret_cast<long long *>(n.gnc_counts.p), n.gnc_sum_dev(full),
                     fslot >= 0 ? cert_->partials.p + (size_t)fslot * nseg : nullptr, nseg);
}

void Group::ml_gnc_summary(MlGncSummaryDev &sd, bool full) {
  HIP_CHECK(hipMemcpyAsync(&sd, ml_->gnc_sum_dev(full), sizeof(sd), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
}

int Group::ml_gnc(const Graph &g, const double *X, int ld, const GncOptions &o, const int *robust_set, long long max_bytes, double *Xout,
                  int ldout, double *weights, double *log, int log_cap, MlGncResult &out) {
  out = MlGncResult();
  const int rows = (d_ + 1) * num_poses_global_;
  const PolishOptions &po = o.inner;
  if (!gnc_args_ok(o.kind, 1.0, o.barc2, "ml gnc")) return -1;
  if (!X || !Xout || !weights || ld < rows || ldout < rows || !(o.mu_step > 1) || !std::isfinite(o.mu_step) || o.max_levels < 1 ||
      po.max_steps < 0 || po.max_tries < 1 || !(po.rel_tol >= 0) || !(po.grad_tol >= 0) || log_cap < 0 || (log_cap > 0 && !log)) {
    fprintf(stderr, "[dpgo_amd] ERROR: ml gnc: bad options or inconsistent size of the output.\n");
    return -1;
  }
  if (ml_begin(g, X, ld, o.anchor, "ml gnc") != 0) return -1;
  PolishResult pr;
  {
    const MlState &n0 = *ml_;
    const int ready = polish_setup(max_bytes, pr, {n0.bytes + n0.gnc_bytes(), ml_remain() + n0.gnc_remain()});
    out.device_bytes = pr.device_bytes;
    out.symbolic_s = pr.symbolic_s;
    if (ready < 0) return -1;
    if (ready != 0) return 0;   // SKIPPED, with what the analysis predicts
  }
  ml_alloc();
  ml_gnc_alloc();
  typedef std::chrono::steady_clock Clock;
  auto ms_since = [](Clock::time_point t) { return 1e3 * std::chrono::duration<double>(Clock::now() - t).count(); };
  const auto t_start = Clock::now();
  CertState &c = *cert_;
  CovState &s = *cov_;
  MlState &n = *ml_;
  const int arow = own_row(o.anchor);
  const NodeMask all{all_bits(), nullptr};
  const size_t m = (size_t)n.plan.m;
  const int d = d_;
  const double c2 = o.barc2;
  double *wdev = n.gnc_w.p;
  std::vector<int> in_R;
  std::vector<double> w_cur(m, 1.0), w_prev(m, 1.0), Xa((size_t)rows * d), Xb((size_t)rows * d);
  HIP_CHECK(hipMemcpyAsync(wdev, w_cur.data(), sizeof(double) * m, hipMemcpyHostToDevice, st_));
  out.num_robust = ml_gnc_set(robust_set, in_R);   // (synchronises)
  double mu = 1.0;   // (level 0: the surrogate's sum is not used)
  PolishHooks hooks;
  hooks.point = [&] {
    ml_gnc_pass(c.X.p, o.kind, mu, c2, false, true, 1);
    launch_ml_gather(lc(all), n.inc_ptr.p, n.inc.p, n.ge.p, arow, s.pol_g.p, 0, c.partials.p);
  };
  hooks.hessian = [&] { ml_hessian_launch(arow); };
  hooks.trial = [&] { ml_gnc_pass(c.V.p, o.kind, mu, c2, false, false, 2); };
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
  // The sums of q describe the returned pair.  chi2 per edge is what the last FULL pass left: on every exit of polish_loop but
  // STALLED that pass ran at the point the loop hands out (ml.cpp: ml_polish), and the evaluation passes write none.
  auto read_final = [&](const MlGncSummaryDev &q) {
    out.F_weighted_final = 0.5 * (q.sum_out + q.sum_ws);
    out.F_surrogate_final = 0.5 * (q.sum_out + q.sum_rho);
    out.num_zero = (int)q.num_zero;
    out.num_one = (int)q.num_one;
    out.num_between = (int)q.num_between;
    out.near_pi = q.near_pi;
    out.near_pi_all = q.near_pi_all;
    std::vector<double> sv(m);
    HIP_CHECK(hipMemcpyAsync(sv.data(), n.chi2.p, sizeof(double) * m, hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
    out.num_outliers = 0;
    for (size_t e = 0; e < m; e++) out.num_outliers += in_R[e] && sv[e] > c2;
  };
  auto finish = [&](int outcome, const std::vector<double> &Xh, int ldh, const std::vector<double> &wh) {
    out.outcome = outcome;
    for (int col = 0; col < d; col++) std::memcpy(Xout + (size_t)col * ldout, Xh.data() + (size_t)col * ldh, sizeof(double) * rows);
    std::copy(wh.begin(), wh.end(), weights);
    out.total_ms = ms_since(t_start);
    return 0;
  };
  // X_{k-1} and the weights it was solved with, after an inner stall: a FULL pass there, so that chi2 is that point's too
  auto failed = [&](const std::vector<double> &Xh, int ldh, const std::vector<double> &wh) {
    MlGncSummaryDev q;
    HIP_CHECK(hipMemcpyAsync(wdev, wh.data(), sizeof(double) * m, hipMemcpyHostToDevice, st_));
    cert_upload(Xh.data(), ldh, d_, c.X.p);
    ml_gnc_pass(c.X.p, o.kind, mu, c2, false, true, -1);
    ml_gnc_summary(q, true);
    read_final(q);
    return finish(GNC_INNER_FAILED, Xh, ldh, wh);
  };
  // level 0
  PolishResult res;
  if (inner(X, ld, Xa.data(), res) != 0) return -1;
  out.F_initial = res.F_initial;
  if (res.outcome == POLISH_STALLED) {
    for (int col = 0; col < d; col++) std::memcpy(Xa.data() + (size_t)col * rows, X + (size_t)col * ld, sizeof(double) * rows);
    return failed(Xa, rows, w_cur);
  }
  MlGncSummaryDev sd;
  auto t0 = Clock::now();
  ml_gnc_pass(c.X.p, o.kind, mu, c2, false, false, -1);   // (polish_loop leaves its final point in CertState's X)
  ml_gnc_summary(sd, false);
  out.edge_ms += ms_since(t0);
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
    ml_gnc_pass(c.X.p, o.kind, mu, c2, true, false, -1);   // WEIGH at X_{k-1}
    HIP_CHECK(hipMemcpyAsync(w_cur.data(), wdev, sizeof(double) * m, hipMemcpyDeviceToHost, st_));
    MlGncSummaryDev sw;
    ml_gnc_summary(sw, false);
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
    // (an inner MAX_STEPS is a level like any other: its point is the last accepted one, and F_w has not increased)
    if (res.outcome == POLISH_STALLED) return failed(*Xprev, rows, w_prev);
    t0 = Clock::now();
    ml_gnc_pass(c.X.p, o.kind, mu, c2, false, false, -1);   // evaluation only, the same mu, at X_k
    ml_gnc_summary(sd, false);
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

int Group::ml_gnc_eval(const Graph &g, const double *X, int ld, int kind, double mu, double barc2, const int *robust_set,
                       const double *w_in, bool full, double *chi2, double *w, double *sums, double *r, double *wr, double *grad,
                       double *jw) {
  if (!X || !chi2 || !w || !sums || !gnc_args_ok(kind, mu, barc2, "ml gnc eval")) return -1;
  if (ml_begin(g, X, ld, 0, "ml gnc eval") != 0) return -1;
  if (!device_has_room(ml_remain() + ml_->gnc_remain())) {
    fprintf(stderr, "[dpgo_amd] ERROR: ml gnc eval: the buffers do not fit the device.\n");
    return -1;
  }
  ml_alloc();
  ml_gnc_alloc();
  CertState &c = *cert_;
  MlState &n = *ml_;
  const size_t m = (size_t)n.plan.m, dof = cov_dof(d_);
  std::vector<int> in_R;
  cert_upload(X, ld, d_, c.X.p);
  HIP_CHECK(hipMemcpyAsync(n.gnc_w.p, w_in ? w_in : w, sizeof(double) * m, hipMemcpyHostToDevice, st_));
  ml_gnc_set(robust_set, in_R);
  // chi2 is a FULL pass's output: the pass is FULL either way, and `full` only says what else is handed out
  ml_gnc_pass(c.X.p, kind, mu, barc2, w_in == nullptr, true, -1);
  HIP_CHECK(hipMemcpyAsync(chi2, n.chi2.p, sizeof(double) * m, hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipMemcpyAsync(w, n.gnc_w.p, sizeof(double) * m, hipMemcpyDeviceToHost, st_));
  if (full) {
    if (r) HIP_CHECK(hipMemcpyAsync(r, n.r.p, sizeof(double) * m * dof, hipMemcpyDeviceToHost, st_));
    if (wr) HIP_CHECK(hipMemcpyAsync(wr, n.wr.p, sizeof(double) * m * dof, hipMemcpyDeviceToHost, st_));
    if (grad) HIP_CHECK(hipMemcpyAsync(grad, n.ge.p, sizeof(double) * 2 * m * dof, hipMemcpyDeviceToHost, st_));
    if (jw) HIP_CHECK(hipMemcpyAsync(jw, n.jw.p, sizeof(double) * m * ml_jw_doubles(d_), hipMemcpyDeviceToHost, st_));
  }
  MlGncSummaryDev sd;
  ml_gnc_summary(sd, true);   // (synchronises)
  const double v[ML_GNC_SUMS] = {sd.sum_out, sd.sum_ws, sd.sum_rho, sd.s_max, sd.w_min, (double)sd.num_zero, (double)sd.num_one,
                                 (double)sd.num_between, (double)sd.near_pi, (double)sd.near_pi_all};
  std::copy(v, v + ML_GNC_SUMS, sums);
  return 0;
}

// Debug: the gradient g_w and the anchored H_w of given weights (FIXED) as ml_hessian hands out g and H: one FULL pass, the
// gather, k_ml_hessian into the factorisation's value array, read back.
int Group::ml_gnc_hessian(const Graph &g, const double *X, int ld, int anchor, const int *robust_set, const double *w_in, int *ptr,
                          int *col, double *val, long long cap, long long *nnz, double *grad) {
  if (!nnz || !w_in || ml_begin(g, X, ld, anchor, "ml gnc hessian") != 0) return -1;
  CertState &c = *cert_;
  CovState &s = *cov_;
  CovResult cr;
  const int ready = cov_setup(0, cr, {ml_->bytes + ml_->gnc_bytes(), ml_remain() + ml_->gnc_remain()});
  if (ready < 0) return -1;
  *nnz = (long long)s.A.col.size();
  if (!ptr && !col && !val) return 0;   // (the size alone)
  if (!ptr || !col || !val || cap < *nnz || ready != 0) {
    fprintf(stderr, "[dpgo_amd] ERROR: ml gnc hessian: room for %lld entries is needed, on the host and on the device.\n", *nnz);
    return -1;
  }
  ml_alloc();
  ml_gnc_alloc();
  MlState &n = *ml_;
  const NodeMask all{all_bits(), nullptr};
  const int dof = cov_dof(d_), N = P0_, arow = own_row(anchor);
  std::vector<int> in_R;
  cert_upload(X, ld, d_, c.X.p);
  HIP_CHECK(hipMemcpyAsync(n.gnc_w.p, w_in, sizeof(double) * n.plan.m, hipMemcpyHostToDevice, st_));
  ml_gnc_set(robust_set, in_R);
  ml_gnc_pass(c.X.p, GNC_TLS, 1.0, 1.0, false, true, -1);
  launch_ml_gather(lc(all), n.inc_ptr.p, n.inc.p, n.ge.p, arow, n.grad.p, 0, c.partials.p);
  ml_hessian_launch(arow);
  std::vector<double> v(s.A.col.size()), gh((size_t)dof * N);
  HIP_CHECK(hipMemcpyAsync(v.data(), spd_numeric_values(s.F), sizeof(double) * v.size(), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipMemcpyAsync(gh.data(), n.grad.p, sizeof(double) * gh.size(), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
  cov_csr_out(v, ptr, col, val);
  if (grad)
    for (int p = 0; p < N; p++) std::copy(&gh[(size_t)dof * p], &gh[(size_t)dof * (p + 1)], grad + (size_t)dof * c.gid[p]);
  return 0;
}

// ---- host only: the per-edge arithmetic of k_ml_gnc_edge<D, true> through ml_math.h and ml_gnc_math.h ----
template <int D>
static bool ml_gnc_edge_one(const double *q, const double *a, const double *b, const double *Om, double w, double *r, double *wr,
                            double *chi2, double *gi, double *gj, double *jw) {
  constexpr int DOF = cov_dof(D), DD = DOF * DOF;
  double Ji[DD], Jj[DD], orr[DOF];
  const bool near = ml_residual<D>(q, a, b, r, Ji, Jj);
  *chi2 = ml_weigh<D>(Om, r, orr);
  ml_gnc_edge_out<D>(w, Om, Ji, Jj, orr, wr, gi, gj, jw);
  return near;
}

int ml_gnc_edge_host(const Graph &g, const double *X, int ld, const double *w, double *r, double *wr, double *chi2, double *grad,
                     double *jw, long long *near_pi, long long *near_pi_all) {
  const int d = g.d, N = g.num_poses, m = (int)g.all.size();
  if ((d != 2 && d != 3) || N <= 0 || m == 0 || !X || !w || ld < (d + 1) * N) return -1;
  for (const Measurement &mm : g.all)
    if (mm.ipose < 0 || mm.ipose >= N || mm.jpose < 0 || mm.jpose >= N) return -1;
  for (int e = 0; e < m; e++)
    if (!(w[e] >= 0 && w[e] <= 1)) return -1;
  std::vector<double> rec, omega, pose((size_t)N * pose_rec_doubles(d));
  graph_information(g, omega);
  const int L = edge_rec_doubles(d), RS = pose_rec_doubles(d), dof = graph_dof(d), DD = dof * dof;
  if (omega.size() != (size_t)m * DD || ml_check_information(d, omega, "ml gnc edge debug") != 0) return -1;
  edge_records(g, rec);
  pose_records(d, N, X, ld, pose.data());
  long long near_w = 0, near_all = 0;
  for (int e = 0; e < m; e++) {
    const double *q = rec.data() + (size_t)e * L, *Om = omega.data() + (size_t)e * DD;
    int i, j;
    bool inter;
    edge_head(q, i, j, inter);
    const double *a = pose.data() + (size_t)i * RS, *b = pose.data() + (size_t)j * RS;
    double re[6], we[6], gi[6], gj[6], rec_e[4 * 36], c2;
    const bool near = d == 2 ? ml_gnc_edge_one<2>(q, a, b, Om, w[e], re, we, &c2, gi, gj, rec_e)
                             : ml_gnc_edge_one<3>(q, a, b, Om, w[e], re, we, &c2, gi, gj, rec_e);
    near_all += near;
    near_w += near && w[e] > 0.0;
    if (r) std::copy(re, re + dof, r + (size_t)e * dof);
    if (wr) std::copy(we, we + dof, wr + (size_t)e * dof);
    if (chi2) chi2[e] = c2;
    if (grad) {
      std::copy(gi, gi + dof, grad + (size_t)2 * e * dof);
      std::copy(gj, gj + dof, grad + ((size_t)2 * e + 1) * dof);
    }
    if (jw) std::copy(rec_e, rec_e + 4 * DD, jw + (size_t)e * 4 * DD);
  }
  if (near_pi) *near_pi = near_w;
  if (near_pi_all) *near_pi_all = near_all;
  return 0;
}

}  // namespace dpgo
