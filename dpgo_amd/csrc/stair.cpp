// Host side of the Riemannian staircase (stair.h): the refusal, the truncated-Newton trust-region method at rank r (TNT.h /
// STPCG as oracle/tnt.py restates them, on the kernels of stair.hip and the certificate's products with M), verify on the
// Lambda of the lifted point, the escape along the certificate's direction, the rounding and the polish.  A handful of scalars
// is read back through the group's read-back flag; nothing here is captured in a graph.  The optimiser's state is not touched
// (cert_begin).
#include "stair.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

#include "cert_state.h"
#include "group.h"

namespace dpgo {

// one lifted point with what was computed at it
struct Group::StairPoint {
  DevBuf<double> Ya, Yb;                   // P0 + P1 rows
  DevBuf<double> MYa, MYb, Ga, Gb, Lam;    // P0 rows
  Lifted Y() { return {Ya.p, Yb.p}; }
  Lifted MY() { return {MYa.p, MYb.p}; }
  Lifted G() { return {Ga.p, Gb.p}; }
  void swap(StairPoint &o) {
    Ya.swap(o.Ya); Yb.swap(o.Yb); MYa.swap(o.MYa); MYb.swap(o.MYb); Ga.swap(o.Ga); Gb.swap(o.Gb); Lam.swap(o.Lam);
  }
};

struct Group::StairState {
  StairPoint cur, trial;
  DevBuf<double> pa, pb;                                            // P0 + P1 rows: the CG's direction, the escape's, a hook's V
  DevBuf<double> Hpa, Hpb, sa, sb, hsa, hsb, ra, rb, za, zb, MVa, MVb;   // P0 rows
  Lifted p() { return {pa.p, pb.p}; }
  Lifted Hp() { return {Hpa.p, Hpb.p}; }
  Lifted s() { return {sa.p, sb.p}; }
  Lifted hs() { return {hsa.p, hsb.p}; }
  Lifted r() { return {ra.p, rb.p}; }
  Lifted z() { return {za.p, zb.p}; }
  Lifted MV() { return {MVa.p, MVb.p}; }
};

void Group::stair_release() {
  delete stair_;
  stair_ = nullptr;
}

// The arguments, the certificate's buffers (cert_begin), the refusal, the lifted vectors (first call that is not refused)
int Group::stair_begin(const double *X, int ld, long long max_bytes, long long *bytes) {
  if (cert_begin(X, ld) != 0) return -1;
  const long long nall = (long long)(P0_ + P1_) * RS_, nown = (long long)P0_ * RS_;
  const long long total = 8ll * (2 * (2 * nall + 4 * nown + (long long)P0_ * d_ * d_) + 2 * nall + 12 * nown);
  if (bytes) *bytes = total;
  if (max_bytes > 0 && total > max_bytes) return 1;
  if (stair_) return 0;
  size_t free_b = 0, total_b = 0;
  HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
  if ((unsigned long long)total > free_b / 2) return 1;   // (nothing that cannot fit is asked of a shared device)
  stair_ = new StairState();
  StairState &s = *stair_;
  for (StairPoint *p : {&s.cur, &s.trial}) {
    for (DevBuf<double> *b : {&p->Ya, &p->Yb}) b->alloc((size_t)std::max<long long>(nall, 1));
    for (DevBuf<double> *b : {&p->MYa, &p->MYb, &p->Ga, &p->Gb}) b->alloc((size_t)std::max<long long>(nown, 1));
    p->Lam.alloc((size_t)std::max(P0_ * d_ * d_, 1));
  }
  for (DevBuf<double> *b : {&s.pa, &s.pb}) b->alloc((size_t)std::max<long long>(nall, 1));
  for (DevBuf<double> *b : {&s.Hpa, &s.Hpb, &s.sa, &s.sb, &s.hsa, &s.hsb, &s.ra, &s.rb, &s.za, &s.zb, &s.MVa, &s.MVb})
    b->alloc((size_t)std::max<long long>(nown, 1));
  return 0;
}

// a global (d+1)N x ncols matrix, d <= ncols <= 2d, into a lifted array over all rows: block B's missing columns are zero
void Group::stair_upload(const double *X, int ld, int ncols, const Lifted &dst) {
  cert_upload(X, ld, d_, dst.a);
  cert_upload(X + (size_t)d_ * ld, ld, ncols - d_, dst.b);
}
void Group::stair_download(const LiftedC &src, double *X, int ld) {
  cert_download(src.a, X, ld, d_);
  cert_download(src.b, X + (size_t)d_ * ld, ld, d_);
}

// out = M in, block by block; block B is skipped while the rank is d (it is zero, and so is its product)
void Group::stair_apply_M(const Lifted &in_all, const Lifted &out_own, int rank) {
  cert_apply_M(in_all.a, out_own.a);
  if (rank > d_) cert_apply_M(in_all.b, out_own.b);
  else HIP_CHECK(hipMemsetAsync(out_own.b, 0, sizeof(double) * (size_t)P0_ * RS_, st_));
}

// M Y, Lambda, the gradient (with store_grad), F and |grad| at the point
void Group::stair_eval_point(StairPoint &p, int rank, bool store_grad, double *F, double *gnorm) {
  CertState &c = *cert_;
  const NodeMask all{all_bits(), nullptr};
  stair_apply_M(p.Y(), p.MY(), rank);
  launch_stair_lambda(lc(all), p.Y(), p.MY(), p.Lam.p, store_grad ? p.G() : Lifted(), c.partials.p);
  launch_polish_reduce(st_, T_, 2, 0u, c.partials.p, c.h_sums, sched_.flag());
  wait_flag(sched_.last_seq());
  if (gnorm) *gnorm = std::sqrt(c.h_sums[0]);
  if (F) *F = c.h_sums[1];
}

// out = Hess[V] at the point (whose Lambda is in place); returns <V, out>, and |out|^2, |V|^2
double Group::stair_hess_product(StairPoint &p, int rank, const Lifted &V_all, const Lifted &MV, const Lifted &out, double *ww,
                                 double *vv) {
  CertState &c = *cert_;
  const NodeMask all{all_bits(), nullptr};
  stair_apply_M(V_all, MV, rank);
  launch_stair_hess(lc(all), p.Y(), p.Lam.p, V_all, MV, out, c.partials.p);
  launch_polish_reduce(st_, T_, 3, 0u, c.partials.p, c.h_sums, sched_.flag());
  wait_flag(sched_.last_seq());
  if (ww) *ww = c.h_sums[1];
  if (vv) *vv = c.h_sums[2];
  return c.h_sums[0];
}

// TNT (TNT.h:242-693) with STPCG (IterativeSolvers.h:166-426) from stair_->cur, which has been evaluated with its gradient;
// *F, *gnorm: at the point on entry and on return
int Group::stair_tnt(const StairOptions &o, int rank, double *F, double *gnorm, int *iters, int *products) {
  CertState &c = *cert_;
  StairState &s = *stair_;
  const NodeMask all{all_bits(), nullptr};
  const double *h = c.h_sums;
  const double *Tp = o.precondition ? c.Tp.p : nullptr;
  const int nseg = std::max(T_.nseg_own, 1);
  double fx = *F, gn = *gnorm, Delta = TntConst::Delta0;
  for (int iteration = 0; iteration < o.max_iterations; iteration++) {
    if (gn < o.grad_norm_tol) break;
    // ---- STPCG: s = hs = 0, r = g, z = P r, p = -z
    launch_stair_cg_update(lc(all), s.cur.Y(), Tp, true, false, 0.0, s.cur.G(), LiftedC(), LiftedC(), s.s(), s.hs(), s.r(), s.z(),
                           c.partials.p);
    launch_polish_reduce(st_, T_, 2, 0u, c.partials.p, c.h_sums, sched_.flag());
    HIP_CHECK(hipMemsetAsync(s.pa.p, 0, sizeof(double) * s.pa.n, st_));
    HIP_CHECK(hipMemsetAsync(s.pb.p, 0, sizeof(double) * s.pb.n, st_));
    launch_stair_cg_dir(lc(all), s.z(), 0.0, s.p());
    wait_flag(sched_.last_seq());
    double rz = h[0];
    if (std::sqrt(h[1]) < o.preconditioned_grad_norm_tol) break;
    double sk_M_pk = 0, sk_M_2 = 0, pk_M_2 = rz, h_M_norm = 0;
    const double Delta_2 = Delta * Delta, r0_norm = std::sqrt(rz);
    const double target = r0_norm * std::min(o.STPCG_kappa, std::pow(r0_norm, o.STPCG_theta));
    bool at_boundary = false;
    for (int it = 0; it < o.max_tCG_iterations; it++) {
      if (std::sqrt(rz) <= target) break;
      double hp2 = 0, pp = 0;
      const double kappa = stair_hess_product(s.cur, rank, s.p(), s.MV(), s.Hp(), &hp2, &pp);
      (*products)++;
      const bool flat = std::sqrt(hp2) / std::sqrt(pp) < 1e-8;   // :305-338; <p, r> = -<r, z> < 0 by conjugacy: p is flipped
      const double alpha = rz / kappa;
      const double skp1_M_2 = sk_M_2 + 2 * alpha * sk_M_pk + alpha * alpha * pk_M_2;
      if (flat || kappa <= 0 || skp1_M_2 > Delta_2) {             // :347-362: to the boundary along p
        const double b = flat ? -sk_M_pk : sk_M_pk;
        const double sigma = (-b + std::sqrt(b * b + pk_M_2 * (Delta_2 - sk_M_2))) / pk_M_2;
        launch_stair_cg_update(lc(all), s.cur.Y(), Tp, false, false, flat ? -sigma : sigma, LiftedC(), s.p(), s.Hp(), s.s(), s.hs(),
                               s.r(), s.z(), c.partials.p);
        at_boundary = true;
        break;
      }
      launch_stair_cg_update(lc(all), s.cur.Y(), Tp, false, true, alpha, LiftedC(), s.p(), s.Hp(), s.s(), s.hs(), s.r(), s.z(),
                             c.partials.p);
      launch_polish_reduce(st_, T_, 2, 0u, c.partials.p, c.h_sums, sched_.flag());
      wait_flag(sched_.last_seq());
      const double rz_new = h[0], beta = rz_new / (alpha * kappa);
      sk_M_2 = skp1_M_2;
      sk_M_pk = beta * (sk_M_pk + alpha * pk_M_2);
      pk_M_2 = rz_new + beta * beta * pk_M_2;
      launch_stair_cg_dir(lc(all), s.z(), beta, s.p());
      rz = rz_new;
    }
    h_M_norm = at_boundary ? Delta : std::sqrt(sk_M_2);
    // ---- the trial point, its value, the model's decrease: -<g, h> - 1/2 <h, H h> with H h accumulated by the CG
    launch_stair_retract(lc(all), s.cur.Y(), s.s(), 1.0, s.cur.G(), s.hs(), s.trial.Y(), c.partials.p);
    stair_apply_M(s.trial.Y(), s.trial.MY(), rank);
    launch_stair_lambda(lc(all), s.trial.Y(), s.trial.MY(), s.trial.Lam.p, s.trial.G(), c.partials.p + (size_t)3 * nseg);
    launch_polish_reduce(st_, T_, 5, 0u, c.partials.p, c.h_sums, sched_.flag());
    wait_flag(sched_.last_seq());
    (*iters)++;
    const double h_norm = std::sqrt(h[1]), dm = -h[0] - 0.5 * h[2], f_prop = h[4], gn_prop = std::sqrt(h[3]);
    const double df = fx - f_prop, rel_dec = df / (TntConst::sqrt_eps() + std::fabs(fx)), rho = df / dm;
    const bool accepted = !std::isnan(rho) && rho > TntConst::eta1;
    if (accepted) {
      s.cur.swap(s.trial);
      fx = f_prop;
      gn = gn_prop;
      if (rel_dec < o.rel_func_decrease_tol) break;
      if (h_norm < o.stepsize_tol) break;
    }
    if (!std::isnan(rho) && rho >= TntConst::eta2) {
      Delta = std::max(TntConst::alpha2 * h_M_norm, Delta);
    } else if (std::isnan(rho) || rho < TntConst::eta1) {
      Delta = TntConst::alpha1 * h_M_norm;
      if (Delta < TntConst::Delta_tol) break;
    }
  }
  *F = fx;
  *gnorm = gn;
  return 0;
}

// The rounding of stair_->cur: the Gram matrix, its eigenvectors on the host, X B, the vote, the projection
int Group::stair_round_point(int rank, double *Bout, double *sigma, double *Xhat, int ldx) {
  (void)rank;
  CertState &c = *cert_;
  StairState &s = *stair_;
  const NodeMask all{all_bits(), nullptr};
  const int n = 2 * d_, d = d_, ntri = n * (n + 1) / 2;
  launch_stair_gram(lc(all), s.cur.Y(), c.partials.p);
  launch_polish_reduce(st_, T_, ntri, 0u, c.partials.p, c.h_sums, sched_.flag());
  wait_flag(sched_.last_seq());
  double G[36], Z[36], w[6];
  for (int a = 0; a < n; a++)
    for (int b = a; b < n; b++) G[a * n + b] = G[b * n + a] = c.h_sums[cert_tri(n, a, b)];
  if (sym_eig(n, G, Z, w) != 0) return -1;
  int idx[6];
  for (int i = 0; i < n; i++) idx[i] = i;
  std::stable_sort(idx, idx + n, [&](int a, int b) { return w[a] > w[b]; });
  for (int i = 0; i < n; i++) sigma[i] = std::sqrt(std::max(w[idx[i]], 0.0));
  StairB B;
  std::memset(&B, 0, sizeof(B));
  for (int j = 0; j < d; j++) {
    int big = 0;
    for (int i = 1; i < n; i++)
      if (std::fabs(Z[i * n + idx[j]]) > std::fabs(Z[big * n + idx[j]])) big = i;
    const double sg = Z[big * n + idx[j]] < 0 ? -1.0 : 1.0;
    for (int i = 0; i < n; i++) B.v[i * d + j] = sg * Z[i * n + idx[j]];
  }
  double *W = s.Hpa.p, *out = s.trial.Ya.p;
  launch_stair_round(lc(all), s.cur.Y(), B, W, c.partials.p);
  launch_polish_reduce(st_, T_, 1, 0u, c.partials.p, c.h_sums, sched_.flag());
  wait_flag(sched_.last_seq());
  if (2.0 * c.h_sums[0] < (double)P0_) {   // most determinants are negative: the other orientation
    for (int i = 0; i < n; i++) B.v[i * d + d - 1] = -B.v[i * d + d - 1];
    launch_stair_round(lc(all), s.cur.Y(), B, W, c.partials.p);
  }
  HIP_CHECK(hipMemsetAsync(s.MVa.p, 0, sizeof(double) * (size_t)P0_ * RS_, st_));
  launch_retract_rot(lc(all), W, s.MVa.p, out);   // every Y_p B onto SO(d): det = +1 whatever the vote left
  launch_stair_copy_t(lc(all), W, out);
  cert_download(out, Xhat, ldx, d);
  if (Bout) std::copy(B.v, B.v + n * d, Bout);
  return 0;
}

int Group::staircase(const double *X, int ld, const StairOptions &oin, long long max_bytes, double *Xhat, int ldx, double *Yout,
                     int ldy, double *log, int log_cap, StairResult &out) {
  out = StairResult();
  const int N = num_poses_global_, rows = (d_ + 1) * N, d = d_;
  StairOptions o = oin;
  if (o.r_max == 0) o.r_max = 2 * d;
  if (!Xhat || ldx < rows || (Yout && ldy < rows) || log_cap < 0 || (log_cap > 0 && !log) || o.r_max < d || o.r_max > 2 * d ||
      o.max_iterations < 0 || o.max_tCG_iterations < 0 || !(o.grad_norm_tol >= 0) || !(o.preconditioned_grad_norm_tol >= 0) ||
      !(o.stepsize_tol >= 0) || !std::isfinite(o.rel_func_decrease_tol) || !(o.STPCG_kappa > 0) || !(o.STPCG_theta >= 0) ||
      !(o.min_eig_num_tol >= 0)) {
    fprintf(stderr, "[dpgo_amd] ERROR: staircase: bad options or inconsistent size of the output.\n");
    return -1;
  }
  const int ready = stair_begin(X, ld, max_bytes, &out.device_bytes);
  if (ready < 0) return -1;
  if (ready != 0) return 0;   // SKIPPED
  CertState &c = *cert_;
  StairState &s = *stair_;
  const NodeMask all{all_bits(), nullptr};
  typedef std::chrono::steady_clock Clock;
  auto ms_since = [](Clock::time_point t) { return 1e3 * std::chrono::duration<double>(Clock::now() - t).count(); };
  const auto t_start = Clock::now();
  if (o.precondition) cert_build_precon();
  CertOptions co;
  co.eta = o.min_eig_num_tol;
  co.precondition = o.precondition;
  const int nseg = std::max(T_.nseg_own, 1);
  std::vector<double> x(rows), E((size_t)rows * 2 * d);
  int rank = d;
  stair_upload(X, ld, d, s.cur.Y());
  double F = 0, gn = 0;
  stair_eval_point(s.cur, rank, true, &F, &gn);
  out.F_initial = F;
  out.outcome = STAIR_SADDLE;
  for (;;) {
    double *row = out.levels < log_cap ? log + (size_t)out.levels * STAIR_LOG_COLS : nullptr;
    out.levels++;
    auto t0 = Clock::now();
    const double F_in = F;
    int iters = 0, products = 0;
    if (stair_tnt(o, rank, &F, &gn, &iters, &products) != 0) return -1;
    out.tnt_iterations += iters;
    out.hess_products += products;
    out.optimise_ms += ms_since(t0);
    t0 = Clock::now();
    HIP_CHECK(hipMemcpyAsync(c.Lam.p, s.cur.Lam.p, sizeof(double) * (size_t)P0_ * d * d, hipMemcpyDeviceToDevice, st_));
    CertResult res;
    CertFactor fac;
    if (verify_lambda(co, o.max_factor_bytes, gn, res, x.data(), rows, fac) != 0) return -1;
    out.verify_ms += ms_since(t0);
    out.cert_status = res.status;
    out.theta = res.theta;
    out.stationarity = gn;
    out.final_rank = rank;
    out.F_sdp = F;
    if (row) {
      row[0] = rank; row[1] = F_in; row[2] = F; row[3] = gn; row[4] = iters; row[5] = products; row[6] = res.status;
      row[7] = res.theta; row[8] = 0.0; row[9] = 0.0;
    }
    if (res.status != CERT_NEGATIVE) {
      out.outcome = STAIR_SOLVED;
      break;
    }
    if (rank == o.r_max) {
      out.outcome = STAIR_MAX_RANK;
      break;
    }
    // the lift: column `rank` of Y is zero, the direction is x there
    t0 = Clock::now();
    std::fill(E.begin(), E.end(), 0.0);
    std::copy(x.begin(), x.end(), E.begin() + (size_t)rank * rows);
    stair_upload(E.data(), rows, 2 * d, s.p());
    double alpha = 1.0;
    int halvings = 0;
    bool accepted = false;
    for (int k = 0; k < 30 && !accepted; k++) {
      launch_stair_retract(lc(all), s.cur.Y(), s.p(), alpha, LiftedC(), LiftedC(), s.trial.Y(), c.partials.p);
      stair_apply_M(s.trial.Y(), s.trial.MY(), rank + 1);
      launch_stair_lambda(lc(all), s.trial.Y(), s.trial.MY(), s.trial.Lam.p, s.trial.G(), c.partials.p + (size_t)3 * nseg);
      launch_polish_reduce(st_, T_, 5, 0u, c.partials.p, c.h_sums, sched_.flag());
      wait_flag(sched_.last_seq());
      const double FZ = c.h_sums[4];
      if (FZ <= F + 0.25 * alpha * alpha * res.theta) {
        accepted = true;
        s.cur.swap(s.trial);
        F = FZ;
        gn = std::sqrt(c.h_sums[3]);
      } else {
        alpha *= 0.5;
        halvings++;
      }
    }
    out.optimise_ms += ms_since(t0);
    if (row) {
      row[8] = accepted ? alpha : 0.0;
      row[9] = halvings;
    }
    if (!accepted) {
      out.outcome = STAIR_SADDLE;
      break;
    }
    rank++;
  }
  if (Yout) stair_download(LiftedC(s.cur.Y()), Yout, ldy);
  // ---- the way back to SO(d)^N
  const auto t0 = Clock::now();
  std::vector<double> Xr((size_t)rows * d), Xp((size_t)rows * d);
  if (stair_round_point(rank, nullptr, out.sigma, Xr.data(), rows) != 0) return -1;
  if (rank == d) cert_download(s.cur.Ya.p, Xr.data(), rows, d);   // (on SO(d)^N already: taken as it is)
  auto value = [&](const std::vector<double> &Z) {
    double v = 0;
    stair_upload(Z.data(), rows, d, s.trial.Y());
    stair_eval_point(s.trial, d, false, &v, nullptr);
    return v;
  };
  out.F_rounded = out.F_final = value(Xr);
  if (o.polish) {
    PolishResult pr;
    if (polish(Xr.data(), rows, 0, PolishOptions(), 0, Xp.data(), rows, nullptr, 0, pr) != 0) return -1;
    out.polish_outcome = pr.outcome;
    if (pr.outcome != POLISH_SKIPPED) {
      Xr.swap(Xp);
      out.F_final = value(Xr);
    }
  }
  if (out.F_final > out.F_initial) {   // never worse than what was handed in
    out.replaced_by_input = 1;
    out.F_final = out.F_initial;
    for (int col = 0; col < d; col++) std::copy(X + (size_t)col * ld, X + (size_t)col * ld + rows, Xr.begin() + (size_t)col * rows);
  }
  for (int col = 0; col < d; col++) std::copy(Xr.begin() + (size_t)col * rows, Xr.begin() + (size_t)(col + 1) * rows, Xhat + (size_t)col * ldx);
  out.gap = out.F_final - out.F_sdp;
  out.round_ms = ms_since(t0);
  out.total_ms = ms_since(t_start);
  return 0;
}

// ---- operator hooks on a lifted point handed in as (d+1)N x 2d ----
int Group::stair_eval(const double *Y, int ldy, double *F, double *gnorm, double *Lambda, double *grad, int ldg) {
  const int rows = (d_ + 1) * num_poses_global_;
  if (!F || !gnorm || (grad && ldg < rows)) return -1;
  if (stair_begin(Y, ldy, 0, nullptr) != 0) return -1;
  StairState &s = *stair_;
  stair_upload(Y, ldy, 2 * d_, s.cur.Y());
  stair_eval_point(s.cur, 2 * d_, true, F, gnorm);
  if (Lambda) {
    std::vector<double> L((size_t)P0_ * d_ * d_);
    HIP_CHECK(hipMemcpy(L.data(), s.cur.Lam.p, sizeof(double) * L.size(), hipMemcpyDeviceToHost));
    for (int row = 0; row < P0_; row++)
      std::copy(&L[(size_t)row * d_ * d_], &L[(size_t)(row + 1) * d_ * d_], Lambda + (size_t)cert_->gid[row] * d_ * d_);
  }
  if (grad) stair_download(LiftedC(s.cur.G()), grad, ldg);
  return 0;
}

int Group::stair_hess(const double *Y, int ldy, const double *V, int ldv, double *out, int ldo) {
  const int rows = (d_ + 1) * num_poses_global_;
  if (!V || !out || ldv < rows || ldo < rows) return -1;
  if (stair_begin(Y, ldy, 0, nullptr) != 0) return -1;
  StairState &s = *stair_;
  stair_upload(Y, ldy, 2 * d_, s.cur.Y());
  stair_eval_point(s.cur, 2 * d_, false, nullptr, nullptr);
  stair_upload(V, ldv, 2 * d_, s.p());
  stair_hess_product(s.cur, 2 * d_, s.p(), s.MV(), s.Hp(), nullptr, nullptr);
  stair_download(LiftedC(s.Hp()), out, ldo);
  return 0;
}

int Group::stair_retract(const double *Y, int ldy, const double *V, int ldv, double *Z, int ldz) {
  const int rows = (d_ + 1) * num_poses_global_;
  if (!V || !Z || ldv < rows || ldz < rows) return -1;
  if (stair_begin(Y, ldy, 0, nullptr) != 0) return -1;
  StairState &s = *stair_;
  stair_upload(Y, ldy, 2 * d_, s.cur.Y());
  stair_upload(V, ldv, 2 * d_, s.p());
  launch_stair_retract(lc(NodeMask{all_bits(), nullptr}), s.cur.Y(), s.p(), 1.0, LiftedC(), LiftedC(), s.trial.Y(), cert_->partials.p);
  stair_download(LiftedC(s.trial.Y()), Z, ldz);
  return 0;
}

int Group::stair_round(const double *Y, int ldy, double *B, double *sigma, double *Xhat, int ldx) {
  const int rows = (d_ + 1) * num_poses_global_;
  if (!B || !sigma || !Xhat || ldx < rows) return -1;
  if (stair_begin(Y, ldy, 0, nullptr) != 0) return -1;
  stair_upload(Y, ldy, 2 * d_, stair_->cur.Y());
  return stair_round_point(2 * d_, B, sigma, Xhat, ldx);
}

}  // namespace dpgo
