// Host side of the robust objective (robust.h): the lists of a (group, graph), its part of the refusals, the robust point, and
// the calls that put the robust F, M_w X and the true Hessian under the polish's loop (polish.cpp: polish_loop) and the
// covariance's tail (cov.cpp: cov_finish).  The optimiser's state is not touched (cert_begin); the certificate's M is never written.
#include "robust.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

#include "cert_state.h"
#include "cov_state.h"
#include "group.h"
#include "robust_math.h"
#include "robust_state.h"

namespace dpgo {

void Group::robust_release() {
  delete rob_;
  rob_ = nullptr;
}

static bool robust_args_ok(int loss, double loss_reg, int curvature, const char *who) {
  if (loss < 0 || loss > 3) {
    fprintf(stderr, "[dpgo_amd] ERROR: %s: loss %d is not one of 0 (none), 1 (Huber), 2 (GM), 3 (Welsch).\n", who, loss);
    return false;
  }
  if (loss != 0 && !(std::isfinite(loss_reg) && loss_reg > 0)) {
    fprintf(stderr, "[dpgo_amd] ERROR: %s: a robust loss needs a finite loss_reg > 0.\n", who);
    return false;
  }
  if (curvature != 0 && curvature != 1) {
    fprintf(stderr, "[dpgo_amd] ERROR: %s: curvature %d is neither 0 (re-weighted) nor 1 (the true Hessian).\n", who, curvature);
    return false;
  }
  return true;
}

// The graph against the group (behind cert_begin): its dimension, its poses, and -- with the certificate's pattern built -- its
// edge records in graph order with the heads on unified own rows, every edge a block of the group's pattern.  eb (optional): per
// edge its blocks (i, i), (i, j), (j, i), (j, j).  Shared with sens.cpp and rely.cpp.
int Group::graph_records_own(const Graph &g, const char *who, std::vector<double> &rec, std::vector<int> *eb) {
  const int N = P0_, m = (int)g.all.size();
  if (g.d != d_ || g.num_poses != N || m == 0) {
    fprintf(stderr, "[dpgo_amd] ERROR: %s: the graph is not one of the group's poses (d %d / %d, poses %d / %d).\n", who, g.d, d_,
            g.num_poses, N);
    return -1;
  }
  for (const Measurement &mm : g.all)
    if (mm.ipose < 0 || mm.ipose >= N || mm.jpose < 0 || mm.jpose >= N || mm.ipose == mm.jpose) {
      fprintf(stderr, "[dpgo_amd] ERROR: %s: an edge names a pose outside the graph, or one pose twice.\n", who);
      return -1;
    }
  cert_build_pattern();
  const int L = edge_rec_doubles(d_);
  edge_records(g, rec);
  if (eb) eb->resize(4 * (size_t)m);
  for (int e = 0; e < m; e++) {   // the heads on unified own rows
    int head[4];
    std::memcpy(head, &rec[(size_t)e * L], sizeof(head));
    const int pq[2] = {head[0] = own_row(head[0]), head[1] = own_row(head[1])};
    std::memcpy(&rec[(size_t)e * L], head, sizeof(head));
    for (int ab = 0; ab < 4; ab++) {
      const int k = cert_block_of(pq[ab / 2], pq[ab % 2]);
      if (k < 0) {
        fprintf(stderr, "[dpgo_amd] ERROR: %s: edge %d (%d, %d) is no block of the group's pattern.\n", who, e, g.all[e].ipose,
                g.all[e].jpose);
        return -1;
      }
      if (eb) (*eb)[4 * (size_t)e + ab] = k;
    }
  }
  return 0;
}

// The lists of a plan from the records (heads on unified own rows) and every edge's four blocks: ascending e, so every list comes
// out in edge order.  Shared with ml.cpp.
void robust_plan_lists(int d, int N, std::vector<double> &&rec, const std::vector<int> &eb, size_t nblk, RobustPlan &pl) {
  const int L = edge_rec_doubles(d), m = (int)(rec.size() / L);
  pl.d = d;
  pl.N = N;
  pl.m = m;
  pl.nb = (m + EDGE_BLOCK - 1) / EDGE_BLOCK;
  std::vector<int> ninc(N + 1, 0), nbl(nblk + 1, 0);
  for (int e = 0; e < m; e++) {
    int head[4];
    std::memcpy(head, &rec[(size_t)e * L], sizeof(head));
    for (int ab = 0; ab < 4; ab++) nbl[eb[4 * (size_t)e + ab] + 1]++;
    ninc[head[0] + 1]++;
    ninc[head[1] + 1]++;
  }
  for (int p = 0; p < N; p++) ninc[p + 1] += ninc[p];
  for (size_t k = 0; k < nblk; k++) nbl[k + 1] += nbl[k];
  pl.inc_ptr = ninc;
  pl.blk_ptr = nbl;
  pl.inc.resize(2 * (size_t)m);
  pl.blk.resize(4 * (size_t)m);
  std::vector<int> fi(ninc.begin(), ninc.end() - 1), fb(nbl.begin(), nbl.end() - 1);
  for (int e = 0; e < m; e++) {
    int head[4];
    std::memcpy(head, &rec[(size_t)e * L], sizeof(head));
    pl.inc[fi[head[0]]++] = 2 * e;
    pl.inc[fi[head[1]]++] = 2 * e + 1;
    for (int ab = 0; ab < 4; ab++) pl.blk[fb[eb[4 * (size_t)e + ab]]++] = 4 * e + ab;
  }
  pl.rec = std::move(rec);
}

// The arguments, the group (cov_begin), the pattern, and the lists of g on the group's unified own rows -- rebuilt only when
// the records differ from those of the last call.  Nothing is allocated on the device for them here.  robust_set (optional,
// one int per edge): overwrites the inter word of the plan's records, which are the key of that comparison.
int Group::robust_begin(const Graph &g, const double *X, int ld, int loss, double loss_reg, int curvature, int anchor, const char *who,
                        const int *robust_set) {
  if (!robust_args_ok(loss, loss_reg, curvature, who)) return -1;
  if (cov_begin(X, ld, anchor) != 0) return -1;
  std::vector<double> rec;
  std::vector<int> eb;   // per edge: its blocks (i, i), (i, j), (j, i), (j, j)
  if (graph_records_own(g, who, rec, &eb) != 0) return -1;
  const int N = P0_, m = (int)g.all.size(), L = edge_rec_doubles(d_);
  CertState &c = *cert_;
  if (robust_set)
    for (int e = 0; e < m; e++) {   // the caller's robust set instead of the inter rule (gnc.h)
      int head[4];
      std::memcpy(head, &rec[(size_t)e * L], sizeof(head));
      head[2] = robust_set[e] != 0;
      std::memcpy(&rec[(size_t)e * L], head, sizeof(head));
    }
  if (rob_ && rob_->plan.rec.size() == rec.size() && std::memcmp(rob_->plan.rec.data(), rec.data(), rec.size() * sizeof(double)) == 0)
    return 0;
  const size_t nblk = c.bptr_h[N];
  const int BB = B_ * B_;
  RobustPlan pl;
  robust_plan_lists(d_, N, std::move(rec), eb, nblk, pl);
  // a new graph: the old buffers go, the next call that is not refused allocates
  delete rob_;
  rob_ = new RobustState();
  RobustState &n = *rob_;
  const long long RS = RS_;
  n.bytes = 8ll * (long long)pl.rec.size() + 8ll * 5 * m + 8ll * 2 * RS * m + 8ll * 3 * pl.nb + 8ll * 2 * pl.nb + 8ll * 5 +
            4ll * ((long long)pl.inc_ptr.size() + (long long)pl.inc.size() + (long long)pl.blk_ptr.size() + (long long)pl.blk.size()) +
            8ll * BB * (long long)nblk + 8ll * cov_dof(d_) * N;
  n.plan = std::move(pl);
  return 0;
}

long long Group::robust_remain() const { return rob_->on_device ? 0 : rob_->bytes; }

void Group::robust_alloc() {
  RobustState &r = *rob_;
  if (r.on_device) return;
  const RobustPlan &pl = r.plan;
  r.rec.upload(pl.rec);
  r.inc_ptr.upload(pl.inc_ptr);
  r.inc.upload(pl.inc);
  r.blk_ptr.upload(pl.blk_ptr);
  r.blk.upload(pl.blk);
  r.out.alloc(5 * (size_t)pl.m);
  r.rows.alloc(2 * (size_t)RS_ * pl.m);
  r.partials.alloc(3 * (size_t)pl.nb);
  r.counts.alloc(2 * (size_t)pl.nb);
  r.sum.alloc(5);
  r.Mw.alloc((size_t)B_ * B_ * cert_->bptr_h[P0_]);
  r.grad.alloc((size_t)cov_dof(d_) * P0_);
  r.on_device = true;
}

// the edge pass at a record array of the group; fslot >= 0: F into that slot of the certificate's partial sums
void Group::robust_eval(const double *Xdev, int loss, double loss_reg, bool with_rows, int fslot) {
  RobustState &r = *rob_;
  const int nseg = std::max(T_.nseg_own, 1);
  launch_robust_edge(d_, st_, r.plan.m, r.rec.p, Xdev, loss, loss_reg, r.out.p, with_rows ? r.rows.p : nullptr, r.partials.p,
                     reinterpret_cast<long long *>(r.counts.p), r.sum_dev(), fslot >= 0 ? cert_->partials.p + (size_t)fslot * nseg : nullptr,
                     nseg);
}

// The robust point: X uploaded, the edge pass with its rows, M_w X gathered, Lambda_w; with `stationarity` also |S_w X|_F, read
// back (a wait).
void Group::robust_point(const double *X, int ld, int loss, double loss_reg, double *stationarity) {
  CertState &c = *cert_;
  RobustState &r = *rob_;
  const NodeMask all{all_bits(), nullptr};
  cert_upload(X, ld, d_, c.X.p);
  robust_eval(c.X.p, loss, loss_reg, true, -1);
  launch_robust_gather(lc(all), r.inc_ptr.p, r.inc.p, r.out.p + 3 * (size_t)r.plan.m, r.rows.p, c.MX.p);
  launch_cert_lambda(lc(all), c.X.p, c.MX.p, c.Lam.p, nullptr, c.partials.p);
  if (!stationarity) return;
  launch_cert_reduce(st_, T_, 1, c.partials.p, c.h_sums, sched_.flag());
  wait_flag(sched_.last_seq());
  *stationarity = std::sqrt(c.h_sums[0]);
}

// M_w from the weights of the last robust_eval, H(S_w) on it and on Lambda_w, the rank-one terms behind it
void Group::robust_hessian_launch(int arow, int curvature) {
  CertState &c = *cert_;
  CovState &s = *cov_;
  RobustState &r = *rob_;
  const int m = r.plan.m;
  launch_robust_mval(d_, st_, P0_, c.bptr.p, r.blk_ptr.p, r.blk.p, r.rec.p, r.out.p + 3 * (size_t)m, r.Mw.p);
  launch_cov_hessian(d_, st_, P0_, c.bptr.p, s.bcol.p, r.Mw.p, c.Lam.p, c.X.p, arow, spd_numeric_values(s.F));
  if (curvature)
    launch_robust_rank1(d_, st_, P0_, c.bptr.p, s.bcol.p, r.blk_ptr.p, r.blk.p, r.out.p + 4 * (size_t)m, r.rows.p, c.X.p, arow,
                        spd_numeric_values(s.F));
}

void Group::robust_summary(EdgeSummary *sum) {
  if (!sum) return;
  EdgeSummaryDev sd;
  HIP_CHECK(hipMemcpyAsync(&sd, rob_->sum_dev(), sizeof(sd), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
  sum->F_intra = sd.F_intra;
  sum->F_inter = sd.F_inter;
  sum->F = sd.F_intra + sd.F_inter;
  sum->weight_min = sd.weight_min;
  sum->num_inter = (int)sd.num_inter;
  sum->num_downweighted = (int)sd.num_downweighted;
}

int Group::robust_polish(const Graph &g, const double *X, int ld, int loss, double loss_reg, int curvature, int anchor,
                         const PolishOptions &o, long long max_bytes, double *Xout, int ldout, double *log, int log_cap,
                         PolishResult &out, EdgeSummary *sum) {
  out = PolishResult();
  const int rows = (d_ + 1) * num_poses_global_;
  if (!Xout || ldout < rows || o.max_steps < 0 || o.max_tries < 1 || !(o.rel_tol >= 0) || !(o.grad_tol >= 0) || log_cap < 0 ||
      (log_cap > 0 && !log)) {
    fprintf(stderr, "[dpgo_amd] ERROR: robust polish: bad options or inconsistent size of the output.\n");
    return -1;
  }
  if (robust_begin(g, X, ld, loss, loss_reg, curvature, anchor, "robust polish") != 0) return -1;
  const int ready = polish_setup(max_bytes, out, {rob_->bytes, robust_remain()});
  if (ready < 0) return -1;
  if (ready != 0) return 0;   // SKIPPED, with what the analysis predicts
  robust_alloc();
  CertState &c = *cert_;
  CovState &s = *cov_;
  RobustState &r = *rob_;
  const int arow = own_row(anchor);
  const NodeMask all{all_bits(), nullptr};
  const int m = r.plan.m;
  PolishHooks hooks;
  hooks.point = [&] {
    robust_eval(c.X.p, loss, loss_reg, true, 1);
    launch_robust_gather(lc(all), r.inc_ptr.p, r.inc.p, r.out.p + 3 * (size_t)m, r.rows.p, c.MX.p);
    launch_cert_lambda(lc(all), c.X.p, c.MX.p, c.Lam.p, nullptr, c.partials.p);
    launch_polish_grad(lc(all), c.X.p, c.MX.p, arow, s.pol_g.p, 0, 3, c.partials.p);   // (its 1/2 <X, M_w X> is not F: a slot nobody reads)
  };
  hooks.hessian = [&] { robust_hessian_launch(arow, curvature); };
  hooks.trial = [&] { robust_eval(c.V.p, loss, loss_reg, false, 2); };
  const int rc = polish_loop(X, ld, arow, o, hooks, Xout, ldout, log, log_cap, out);
  if (rc != 0) return rc;
  if (sum) {   // the final point is in CertState's X
    robust_eval(c.X.p, loss, loss_reg, false, -1);
    robust_summary(sum);
  }
  return 0;
}

int Group::robust_covariance(const Graph &g, const double *X, int ld, int loss, double loss_reg, int curvature, int anchor,
                             long long max_bytes, const int *pairs, int npairs, double *marginals, double *cross, CovResult &out) {
  out = CovResult();
  if (!marginals || npairs < 0 || (npairs > 0 && (!pairs || !cross))) {
    fprintf(stderr, "[dpgo_amd] ERROR: robust covariance: missing output or pair arrays.\n");
    return -1;
  }
  if (robust_begin(g, X, ld, loss, loss_reg, curvature, anchor, "robust covariance") != 0) return -1;
  if (!pairs_args_ok("robust covariance", pairs, npairs)) return -1;
  const int ready = cov_setup(max_bytes, out, {rob_->bytes, robust_remain()});
  if (ready < 0 || !pairs_are_edges("robust covariance", pairs, npairs)) return -1;
  if (ready != 0) return 0;   // SKIPPED: nothing allocated, the stationarity not computed
  robust_alloc();
  robust_point(X, ld, loss, loss_reg, &out.stationarity);
  const int arow = own_row(anchor);
  return cov_finish([&] { robust_hessian_launch(arow, curvature); }, arow, pairs, npairs, marginals, cross, out);
}

int Group::robust_hessian(const Graph &g, const double *X, int ld, int loss, double loss_reg, int curvature, int anchor, int *ptr,
                          int *col, double *val, long long cap, long long *nnz, double *grad, double *F, double *w, double *cc,
                          double *s_rot, double *s_trans, double *rho) {
  if (!nnz || robust_begin(g, X, ld, loss, loss_reg, curvature, anchor, "robust hessian") != 0) return -1;
  CertState &c = *cert_;
  CovState &s = *cov_;
  CovResult cr;
  const int ready = cov_setup(0, cr, {rob_->bytes, robust_remain()});
  if (ready < 0) return -1;
  *nnz = (long long)s.A.col.size();
  if (!ptr && !col && !val) return 0;   // (the size alone)
  if (!ptr || !col || !val || cap < *nnz) {
    fprintf(stderr, "[dpgo_amd] ERROR: robust hessian: room for %lld entries is needed.\n", *nnz);
    return -1;
  }
  if (ready != 0) {
    fprintf(stderr, "[dpgo_amd] ERROR: robust hessian: the value array of the factorisation does not fit the device.\n");
    return -1;
  }
  robust_alloc();
  RobustState &r = *rob_;
  const NodeMask all{all_bits(), nullptr};
  const int dof = cov_dof(d_), N = P0_, m = r.plan.m, arow = own_row(anchor);
  robust_point(X, ld, loss, loss_reg, nullptr);   // (no reduction: the stationarity is not handed out)
  launch_polish_grad(lc(all), c.X.p, c.MX.p, arow, r.grad.p, 0, 3, c.partials.p);
  robust_hessian_launch(arow, curvature);
  std::vector<double> v(s.A.col.size()), gh((size_t)dof * N), eo(5 * (size_t)m);
  HIP_CHECK(hipMemcpyAsync(v.data(), spd_numeric_values(s.F), sizeof(double) * v.size(), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipMemcpyAsync(gh.data(), r.grad.p, sizeof(double) * gh.size(), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipMemcpyAsync(eo.data(), r.out.p, sizeof(double) * eo.size(), hipMemcpyDeviceToHost, st_));
  EdgeSummary sm;
  robust_summary(&sm);   // (synchronises)
  cov_csr_out(v, ptr, col, val);
  if (grad)
    for (int p = 0; p < N; p++) std::copy(&gh[(size_t)dof * p], &gh[(size_t)dof * (p + 1)], grad + (size_t)dof * c.gid[p]);
  if (F) *F = sm.F;
  double *first[3] = {s_rot, s_trans, rho};
  for (int k = 0; k < 3; k++)
    if (first[k]) std::copy(eo.begin() + k * (size_t)m, eo.begin() + (k + 1) * (size_t)m, first[k]);
  if (w) std::copy(eo.begin() + 3 * (size_t)m, eo.begin() + 4 * (size_t)m, w);
  if (cc) std::copy(eo.begin() + 4 * (size_t)m, eo.end(), cc);
  return 0;
}

int Group::robust_matrix(const Graph &g, const double *X, int ld, int loss, double loss_reg, int *ptr, int *col, double *val,
                         long long cap, long long *nnz) {
  if (!nnz || robust_begin(g, X, ld, loss, loss_reg, 0, 0, "robust matrix") != 0) return -1;
  CertState &c = *cert_;
  *nnz = (long long)c.A.col.size();
  if (!ptr && !col && !val) return 0;   // (the size alone)
  if (!ptr || !col || !val || cap < *nnz) {
    fprintf(stderr, "[dpgo_amd] ERROR: robust matrix: room for %lld entries is needed.\n", *nnz);
    return -1;
  }
  if (!device_has_room(robust_remain())) {
    fprintf(stderr, "[dpgo_amd] ERROR: robust matrix: the buffers do not fit the device.\n");
    return -1;
  }
  robust_alloc();
  RobustState &r = *rob_;
  const int m = r.plan.m;
  cert_upload(X, ld, d_, c.X.p);
  robust_eval(c.X.p, loss, loss_reg, false, -1);
  launch_robust_mval(d_, st_, P0_, c.bptr.p, r.blk_ptr.p, r.blk.p, r.rec.p, r.out.p + 3 * (size_t)m, r.Mw.p);
  std::vector<double> v(c.A.col.size());
  HIP_CHECK(hipMemcpyAsync(v.data(), r.Mw.p, sizeof(double) * v.size(), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
  cert_csr_out(v, ptr, col, val);
  return 0;
}

// ---- host only: the per-edge arithmetic of the kernels through robust_math.h ----
int robust_edge_host(const Graph &g, const double *X, int ld, int loss, double loss_reg, double *w, double *c, double *rows,
                     double *ghat) {
  const int d = g.d, N = g.num_poses, m = (int)g.all.size();
  if ((d != 2 && d != 3) || N <= 0 || m == 0 || !X || ld < (d + 1) * N || !robust_args_ok(loss, loss_reg, 0, "robust edge debug")) return -1;
  for (const Measurement &mm : g.all)
    if (mm.ipose < 0 || mm.ipose >= N || mm.jpose < 0 || mm.jpose >= N) return -1;
  std::vector<double> rec, pose((size_t)N * pose_rec_doubles(d));
  edge_records(g, rec);
  pose_records(d, N, X, ld, pose.data());
  const int L = edge_rec_doubles(d), RS = pose_rec_doubles(d), dof = d + d * (d - 1) / 2;
  for (int e = 0; e < m; e++) {
    const double *q = rec.data() + (size_t)e * L;
    int i, j;
    bool inter;
    edge_head(q, i, j, inter);
    const double *a = pose.data() + (size_t)i * RS, *b = pose.data() + (size_t)j * RS;
    double v[4], ri[12], rj[12];
    if (d == 2) {
      edge_lane<2>(q, a, b, inter, loss, loss_reg, v);
      robust_rows<2>(q, a, b, ri, rj);
    } else {
      edge_lane<3>(q, a, b, inter, loss, loss_reg, v);
      robust_rows<3>(q, a, b, ri, rj);
    }
    if (w) w[e] = v[3];
    if (c) c[e] = robust_curv(loss, loss_reg, v[0] + v[1], v[3], inter);
    if (rows) {
      std::copy(ri, ri + RS, rows + (size_t)2 * e * RS);
      std::copy(rj, rj + RS, rows + ((size_t)2 * e + 1) * RS);
    }
    if (ghat)
      for (int k = 0; k < dof; k++) {
        ghat[(size_t)2 * e * dof + k] = d == 2 ? robust_ghat_entry<2>(a, ri, k) : robust_ghat_entry<3>(a, ri, k);
        ghat[((size_t)2 * e + 1) * dof + k] = d == 2 ? robust_ghat_entry<2>(b, rj, k) : robust_ghat_entry<3>(b, rj, k);
      }
  }
  return 0;
}

}  // namespace dpgo
