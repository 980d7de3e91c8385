// Host side of the maximum-likelihood objective (ml.h): the lists of a (group, graph) -- RobustPlan's, built by
// robust_plan_lists -- with the graph's Omega checked, its part of the refusals, and the calls that put F_ml, its gradient and
// its Gauss-Newton Hessian under the polish's loop (polish.cpp: polish_loop) and the covariance's tail (cov.cpp: cov_finish).
// The optimiser's state is not touched (cert_begin); the certificate's M is never written.
#include "ml.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "cert_state.h"
#include "cov_state.h"
#include "edge_math.h"
#include "group.h"
#include "ml_math.h"
#include "ml_state.h"

namespace dpgo {

void Group::ml_release() {
  delete ml_;
  ml_ = nullptr;
}

// every Omega_e symmetric (to 1e-12 of its largest diagonal entry) and positive definite (its Cholesky factor exists)
int ml_check_information(int d, const std::vector<double> &omega, const char *who) {
  const int dof = graph_dof(d), DD = dof * dof;
  const size_t m = omega.size() / DD;
  for (size_t e = 0; e < m; e++) {
    const double *O = &omega[e * DD];
    double L[36], dmax = 0;
    bool ok = true;
    for (int k = 0; k < dof; k++) dmax = std::max(dmax, std::fabs(O[k * dof + k]));
    for (int k = 0; k < dof && ok; k++)
      for (int l = 0; l < dof && ok; l++) ok = std::isfinite(O[k * dof + l]) && std::fabs(O[k * dof + l] - O[l * dof + k]) <= 1e-12 * dmax;
    for (int k = 0; k < dof && ok; k++)
      for (int l = 0; l <= k && ok; l++) {
        double s = O[k * dof + l];
        for (int c = 0; c < l; c++) s -= L[k * dof + c] * L[l * dof + c];
        if (l == k) {
          ok = s > 0;
          L[k * dof + k] = ok ? std::sqrt(s) : 0;
        } else {
          L[k * dof + l] = s / L[l * dof + l];
        }
      }
    if (!ok) {
      fprintf(stderr, "[dpgo_amd] ERROR: %s: the information matrix of edge %zu is not symmetric positive definite.\n", who, e);
      return -1;
    }
  }
  return 0;
}

// The group (cov_begin), the pattern, and the lists of g with its Omega on the group's unified own rows -- rebuilt only when the
// records or Omega differ from those of the last call.  Nothing is allocated on the device here.
int Group::ml_begin(const Graph &g, const double *X, int ld, int anchor, const char *who) {
  if (cov_begin(X, ld, anchor) != 0) return -1;
  std::vector<double> rec, omega;
  std::vector<int> eb;
  if (graph_records_own(g, who, rec, &eb) != 0) return -1;
  graph_information(g, omega);
  const int dof = cov_dof(d_), DD = dof * dof, m = (int)g.all.size();
  if (omega.size() != (size_t)m * DD) {
    fprintf(stderr, "[dpgo_amd] ERROR: %s: the graph's information matrices do not match its edges.\n", who);
    return -1;
  }
  auto same = [](const std::vector<double> &a, const std::vector<double> &b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
  };
  if (ml_ && same(ml_->plan.rec, rec) && same(ml_->omega, omega)) return 0;
  if (ml_check_information(d_, omega, who) != 0) return -1;
  // a new graph: the old buffers go, the next call that is not refused allocates
  delete ml_;
  ml_ = new MlState();
  MlState &n = *ml_;
  robust_plan_lists(d_, P0_, std::move(rec), eb, cert_->bptr_h[P0_], n.plan);
  n.omega = std::move(omega);
  const RobustPlan &pl = n.plan;
  n.bytes = 8ll * (long long)pl.rec.size() + 8ll * (long long)n.omega.size() + 8ll * m * (2 * dof + 1 + 2 * dof + ml_jw_doubles(d_)) +
            8ll * 2 * pl.nb + 2ll * (long long)sizeof(MlSummaryDev) + 8ll * dof * P0_ +
            4ll * ((long long)pl.inc_ptr.size() + (long long)pl.inc.size() + (long long)pl.blk_ptr.size() + (long long)pl.blk.size());
  return 0;
}

long long Group::ml_remain() const { return ml_->on_device ? 0 : ml_->bytes; }

void Group::ml_alloc() {
  MlState &s = *ml_;
  if (s.on_device) return;
  const RobustPlan &pl = s.plan;
  const size_t m = pl.m, dof = cov_dof(d_);
  s.rec.upload(pl.rec);
  s.om.upload(s.omega);
  s.inc_ptr.upload(pl.inc_ptr);
  s.inc.upload(pl.inc);
  s.blk_ptr.upload(pl.blk_ptr);
  s.blk.upload(pl.blk);
  s.r.alloc(m * dof);
  s.wr.alloc(m * dof);
  s.chi2.alloc(m);
  s.ge.alloc(2 * m * dof);
  s.jw.alloc(m * ml_jw_doubles(d_));
  s.partials.alloc(pl.nb);
  s.counts.alloc(pl.nb);
  s.sum.alloc(2 * sizeof(MlSummaryDev) / sizeof(double));
  s.grad.alloc(dof * P0_);
  s.on_device = true;
}

void Group::ml_edge_pass(const double *Xdev, bool full, int fslot) {
  MlState &s = *ml_;
  const int nseg = std::max(T_.nseg_own, 1);
  launch_ml_edge(d_, st_, s.plan.m, s.rec.p, s.om.p, Xdev, full ? s.out() : MlEdgeOut(), s.partials.p,
                 reinterpret_cast<long long *>(s.counts.p), s.sum_dev(full), fslot >= 0 ? cert_->partials.p + (size_t)fslot * nseg : nullptr, nseg);
}

void Group::ml_point(int arow, double *g, int slot_g2, int fslot) {
  MlState &s = *ml_;
  const NodeMask all{all_bits(), nullptr};
  ml_edge_pass(cert_->X.p, true, fslot);
  launch_ml_gather(lc(all), s.inc_ptr.p, s.inc.p, s.ge.p, arow, g, slot_g2, cert_->partials.p);
}

void Group::ml_hessian_launch(int arow) {
  MlState &s = *ml_;
  launch_ml_hessian(d_, st_, P0_, cert_->bptr.p, cov_->bcol.p, s.blk_ptr.p, s.blk.p, s.jw.p, arow, spd_numeric_values(cov_->F));
}

int Group::ml_polish(const Graph &g, const double *X, int ld, int anchor, const PolishOptions &o, long long max_bytes, double *Xout,
                     int ldout, double *log, int log_cap, MlResult &out) {
  out = MlResult();
  const int rows = (d_ + 1) * num_poses_global_;
  if (!Xout || ldout < rows || o.max_steps < 0 || o.max_tries < 1 || !(o.rel_tol >= 0) || !(o.grad_tol >= 0) || log_cap < 0 ||
      (log_cap > 0 && !log)) {
    fprintf(stderr, "[dpgo_amd] ERROR: ml polish: bad options or inconsistent size of the output.\n");
    return -1;
  }
  if (ml_begin(g, X, ld, anchor, "ml polish") != 0) return -1;
  const int ready = polish_setup(max_bytes, out, {ml_->bytes, ml_remain()});
  if (ready < 0) return -1;
  if (ready != 0) return 0;   // SKIPPED, with what the analysis predicts
  ml_alloc();
  CertState &c = *cert_;
  CovState &s = *cov_;
  MlState &n = *ml_;
  const int arow = own_row(anchor);
  PolishHooks hooks;
  hooks.point = [&] { ml_point(arow, s.pol_g.p, 0, 1); };
  hooks.hessian = [&] { ml_hessian_launch(arow); };
  hooks.trial = [&] { ml_edge_pass(c.V.p, false, 2); };
  const int rc = polish_loop(X, ld, arow, o, hooks, Xout, ldout, log, log_cap, out);
  if (rc != 0) return rc;
  // near_pi of the final point: on every exit of the loop -- CONVERGED and MAX_STEPS straight behind hooks.point, STALLED with
  // every try behind it rejected -- the last full edge pass ran at the point the loop hands out, and the trial passes write a
  // summary of their own
  MlSummaryDev sd;
  HIP_CHECK(hipMemcpyAsync(&sd, n.sum_dev(), sizeof(sd), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
  out.near_pi = sd.near_pi;
  out.chi2_initial = 2 * out.F_initial;
  out.chi2_final = 2 * out.F_final;
  return 0;
}

int Group::ml_covariance(const Graph &g, const double *X, int ld, int anchor, long long max_bytes, const int *pairs, int npairs,
                         double *marginals, double *cross, CovResult &out) {
  out = CovResult();
  if (!marginals || npairs < 0 || (npairs > 0 && (!pairs || !cross))) {
    fprintf(stderr, "[dpgo_amd] ERROR: ml covariance: missing output or pair arrays.\n");
    return -1;
  }
  if (ml_begin(g, X, ld, anchor, "ml covariance") != 0) return -1;
  if (!pairs_args_ok("ml covariance", pairs, npairs)) return -1;
  const int ready = cov_setup(max_bytes, out, {ml_->bytes, ml_remain()});
  if (ready < 0 || !pairs_are_edges("ml covariance", pairs, npairs)) return -1;
  if (ready != 0) return 0;   // SKIPPED: nothing allocated, the stationarity not computed
  ml_alloc();
  CertState &c = *cert_;
  const int arow = own_row(anchor);
  cert_upload(X, ld, d_, c.X.p);
  ml_point(arow, ml_->grad.p, 0, -1);   // stationarity: |g_ml|, the tangent gradient of F_ml
  launch_polish_reduce(st_, T_, 1, 0u, c.partials.p, c.h_sums, sched_.flag());
  wait_flag(sched_.last_seq());
  out.stationarity = std::sqrt(c.h_sums[0]);
  return cov_finish([&] { ml_hessian_launch(arow); }, arow, pairs, npairs, marginals, cross, out);
}

int Group::ml_hessian(const Graph &g, const double *X, int ld, int anchor, int *ptr, int *col, double *val, long long cap,
                      long long *nnz, double *grad, double *F) {
  if (!nnz || ml_begin(g, X, ld, anchor, "ml hessian") != 0) return -1;
  CertState &c = *cert_;
  CovState &s = *cov_;
  CovResult cr;
  const int ready = cov_setup(0, cr, {ml_->bytes, ml_remain()});
  if (ready < 0) return -1;
  *nnz = (long long)s.A.col.size();
  if (!ptr && !col && !val) return 0;   // (the size alone)
  if (!ptr || !col || !val || cap < *nnz) {
    fprintf(stderr, "[dpgo_amd] ERROR: ml hessian: room for %lld entries is needed.\n", *nnz);
    return -1;
  }
  if (ready != 0) {
    fprintf(stderr, "[dpgo_amd] ERROR: ml hessian: the value array of the factorisation does not fit the device.\n");
    return -1;
  }
  ml_alloc();
  MlState &n = *ml_;
  const int dof = cov_dof(d_), N = P0_, arow = own_row(anchor);
  cert_upload(X, ld, d_, c.X.p);
  ml_point(arow, n.grad.p, 0, -1);
  ml_hessian_launch(arow);
  std::vector<double> v(s.A.col.size()), gh((size_t)dof * N);
  MlSummaryDev sd;
  HIP_CHECK(hipMemcpyAsync(v.data(), spd_numeric_values(s.F), sizeof(double) * v.size(), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipMemcpyAsync(gh.data(), n.grad.p, sizeof(double) * gh.size(), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipMemcpyAsync(&sd, n.sum_dev(), sizeof(sd), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
  cov_csr_out(v, ptr, col, val);
  if (grad)
    for (int p = 0; p < N; p++) std::copy(&gh[(size_t)dof * p], &gh[(size_t)dof * (p + 1)], grad + (size_t)dof * c.gid[p]);
  if (F) *F = sd.F;
  return 0;
}

// Debug: k_ml_hessian on an array of the caller's making -- pad sentinels, the nnz values (sentinels too before the launch), pad
// sentinels -- instead of the factorisation's; guards: the 2 pad doubles around it as the device left them, val: the values as
// ml_hessian hands them out.  Behind an ml_hessian call of the same arguments, whose edge pass it repeats.
int Group::ml_hessian_guarded(const Graph &g, const double *X, int ld, int anchor, int pad, double sentinel, double *guards, double *val,
                              long long cap) {
  if (pad < 1 || !guards || !val || ml_begin(g, X, ld, anchor, "ml hessian (guarded)") != 0) return -1;
  CertState &c = *cert_;
  CovState &s = *cov_;
  CovResult cr;
  if (cov_setup(0, cr, {ml_->bytes, ml_remain()}) != 0) return -1;
  const size_t nnz = s.A.col.size();
  if (cap < (long long)nnz || !device_has_room(8ll * (long long)(nnz + 2 * (size_t)pad))) return -1;
  ml_alloc();
  MlState &n = *ml_;
  const int arow = own_row(anchor);
  std::vector<double> h(nnz + 2 * (size_t)pad, sentinel);
  DevBuf<double> buf;
  buf.upload(h);
  cert_upload(X, ld, d_, c.X.p);
  ml_point(arow, n.grad.p, 0, -1);
  launch_ml_hessian(d_, st_, P0_, c.bptr.p, s.bcol.p, n.blk_ptr.p, n.blk.p, n.jw.p, arow, buf.p + pad);
  HIP_CHECK(hipMemcpyAsync(h.data(), buf.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
  std::copy(h.begin(), h.begin() + pad, guards);
  std::copy(h.end() - pad, h.end(), guards + pad);
  std::vector<double> v(h.begin() + pad, h.end() - pad);
  std::vector<int> ptr(s.A.n + 1), col(nnz);
  cov_csr_out(v, ptr.data(), col.data(), val);
  return 0;
}

int Group::ml_eval(const Graph &g, const double *X, int ld, double *F, long long *near_pi, double *r, double *chi2, double *wr,
                   double *grad, double *jw) {
  if (ml_begin(g, X, ld, 0, "ml eval") != 0) return -1;
  if (!device_has_room(ml_remain())) {
    fprintf(stderr, "[dpgo_amd] ERROR: ml eval: the buffers do not fit the device.\n");
    return -1;
  }
  ml_alloc();
  CertState &c = *cert_;
  MlState &n = *ml_;
  const size_t m = n.plan.m, dof = cov_dof(d_);
  cert_upload(X, ld, d_, c.X.p);
  ml_edge_pass(c.X.p, true, -1);
  MlSummaryDev sd;
  if (r) HIP_CHECK(hipMemcpyAsync(r, n.r.p, sizeof(double) * m * dof, hipMemcpyDeviceToHost, st_));
  if (chi2) HIP_CHECK(hipMemcpyAsync(chi2, n.chi2.p, sizeof(double) * m, hipMemcpyDeviceToHost, st_));
  if (wr) HIP_CHECK(hipMemcpyAsync(wr, n.wr.p, sizeof(double) * m * dof, hipMemcpyDeviceToHost, st_));
  if (grad) HIP_CHECK(hipMemcpyAsync(grad, n.ge.p, sizeof(double) * 2 * m * dof, hipMemcpyDeviceToHost, st_));
  if (jw) HIP_CHECK(hipMemcpyAsync(jw, n.jw.p, sizeof(double) * m * ml_jw_doubles(d_), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipMemcpyAsync(&sd, n.sum_dev(), sizeof(sd), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
  if (F) *F = sd.F;
  if (near_pi) *near_pi = sd.near_pi;
  return 0;
}

// ---- host only: the per-edge arithmetic of the kernels through ml_math.h ----
int ml_edge_host(const Graph &g, const double *X, int ld, double *r, double *wr, double *chi2, double *Ji, double *Jj, double *grad,
                 double *blocks, long long *near_pi) {
  const int d = g.d, N = g.num_poses, m = (int)g.all.size();
  if ((d != 2 && d != 3) || N <= 0 || m == 0 || !X || ld < (d + 1) * N) return -1;
  for (const Measurement &mm : g.all)
    if (mm.ipose < 0 || mm.ipose >= N || mm.jpose < 0 || mm.jpose >= N) return -1;
  std::vector<double> rec, omega, pose((size_t)N * pose_rec_doubles(d));
  graph_information(g, omega);
  const int L = edge_rec_doubles(d), RS = pose_rec_doubles(d), dof = graph_dof(d), DD = dof * dof;
  if (omega.size() != (size_t)m * DD || ml_check_information(d, omega, "ml edge debug") != 0) return -1;
  edge_records(g, rec);
  pose_records(d, N, X, ld, pose.data());
  long long near = 0;
  for (int e = 0; e < m; e++) {
    const double *q = rec.data() + (size_t)e * L, *Om = omega.data() + (size_t)e * DD;
    int i, j;
    bool inter;
    edge_head(q, i, j, inter);
    const double *a = pose.data() + (size_t)i * RS, *b = pose.data() + (size_t)j * RS;
    double re[6], we[6], jw[4 * 36];
    double c2;
    if (d == 2) {
      near += ml_residual<2>(q, a, b, re, jw, jw + DD);
      c2 = ml_weigh<2>(Om, re, we);
    } else {
      near += ml_residual<3>(q, a, b, re, jw, jw + DD);
      c2 = ml_weigh<3>(Om, re, we);
    }
    for (int k = 0; k < dof; k++)
      for (int cc = 0; cc < dof; cc++) {
        jw[2 * DD + k * dof + cc] = d == 2 ? ml_w_entry<2>(Om, jw, k, cc) : ml_w_entry<3>(Om, jw, k, cc);
        jw[3 * DD + k * dof + cc] = d == 2 ? ml_w_entry<2>(Om, jw + DD, k, cc) : ml_w_entry<3>(Om, jw + DD, k, cc);
      }
    if (r) std::copy(re, re + dof, r + (size_t)e * dof);
    if (wr) std::copy(we, we + dof, wr + (size_t)e * dof);
    if (chi2) chi2[e] = c2;
    if (Ji) std::copy(jw, jw + DD, Ji + (size_t)e * DD);
    if (Jj) std::copy(jw + DD, jw + 2 * DD, Jj + (size_t)e * DD);
    if (grad)
      for (int k = 0; k < dof; k++) {
        grad[(size_t)2 * e * dof + k] = d == 2 ? ml_grad_entry<2>(jw, we, k) : ml_grad_entry<3>(jw, we, k);
        grad[((size_t)2 * e + 1) * dof + k] = d == 2 ? ml_grad_entry<2>(jw + DD, we, k) : ml_grad_entry<3>(jw + DD, we, k);
      }
    if (blocks)
      for (int ab = 0; ab < 4; ab++)
        for (int k = 0; k < dof; k++)
          for (int cc = 0; cc < dof; cc++)
            blocks[((size_t)4 * e + ab) * DD + k * dof + cc] =
                d == 2 ? ml_block_entry<2>(jw, ab >> 1, ab & 1, k, cc) : ml_block_entry<3>(jw, ab >> 1, ab & 1, k, cc);
  }
  if (near_pi) *near_pi = near;
  return 0;
}

}  // namespace dpgo
