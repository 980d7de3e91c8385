// Host side of graduated non-convexity on the maximum-likelihood objective (ml_gnc.h): what this objective is to gnc.cpp's outer
// loop (gnc_loop), on chi2.  The plan, the lists, Omega's check and the refusal are the ML objective's (ml.cpp); the inner solve
// is polish_loop (polish.cpp), once per level, with the weights of k_ml_gnc_edge held fixed; the gather and the Hessian kernel
// are ml.hip's, unchanged.  The optimiser's state is not touched (cert_begin).
#include "ml_gnc.h"

#include <algorithm>

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
  n.gnc_partials.alloc((size_t)GNC_PARTIAL_SLOTS * n.plan.nb);
  n.gnc_counts.alloc((size_t)ML_GNC_COUNT_SLOTS * n.plan.nb);
  n.gnc_sum.alloc(2 * sizeof(MlGncSummaryDev) / sizeof(double));
  n.gnc_on_device = true;
}

// R of this call (gnc_robust_mask on the plan's records), uploaded (the stream is synchronised).  Returns |R|.
int Group::ml_gnc_set(const int *robust_set, std::vector<int> &in_R) {
  MlState &n = *ml_;
  const int count = gnc_robust_mask(d_, n.plan.m, n.plan.rec.data(), robust_set, in_R);
  HIP_CHECK(hipMemcpyAsync(n.gnc_in_R.p, in_R.data(), sizeof(int) * in_R.size(), hipMemcpyHostToDevice, st_));
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

void Group::ml_gnc_summary(GncSummary &q, bool full) {
  MlGncSummaryDev sd;
  HIP_CHECK(hipMemcpyAsync(&sd, ml_->gnc_sum_dev(full), sizeof(sd), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
  q.sums = sd.gnc;
  q.near_pi = sd.near_pi;
  q.near_pi_all = sd.near_pi_all;
}

int Group::ml_gnc(const Graph &g, const double *X, int ld, const GncOptions &o, const int *robust_set, long long max_bytes, double *Xout,
                  int ldout, double *weights, double *log, int log_cap, MlGncResult &out) {
  out = MlGncResult();
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
  CertState &c = *cert_;
  CovState &s = *cov_;
  MlState &n = *ml_;
  const int arow = own_row(o.anchor);
  const NodeMask all{all_bits(), nullptr};
  GncObjective ob;
  ob.wdev = n.gnc_w.p;
  ob.num_robust = ml_gnc_set(robust_set, ob.in_R);
  ob.pass = [&](const double *Xdev, double mu, bool weigh, bool full, int fslot) {
    ml_gnc_pass(Xdev, o.kind, mu, o.barc2, weigh, full, fslot);
  };
  ob.summary = [&](GncSummary &q, bool full) { ml_gnc_summary(q, full); };
  ob.gradient = [&] { launch_ml_gather(lc(all), n.inc_ptr.p, n.inc.p, n.ge.p, arow, s.pol_g.p, 0, c.partials.p); };
  ob.hessian = [&] { ml_hessian_launch(arow); };
  ob.edge_s = [&](double *sv) {
    HIP_CHECK(hipMemcpyAsync(sv, n.chi2.p, sizeof(double) * n.plan.m, hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
  };
  ob.failure_per_edge = true;
  ob.level0_stall_evaluated = true;
  GncSummary last;
  const int rc = gnc_loop("ml gnc", X, ld, o, ob, Xout, ldout, weights, log, log_cap, out, &last);
  out.near_pi = last.near_pi;
  out.near_pi_all = last.near_pi_all;
  return rc;
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
  GncSummary sd;
  ml_gnc_summary(sd, true);   // (synchronises)
  gnc_summary_doubles(sd, ML_GNC_SUMS, sums);
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
