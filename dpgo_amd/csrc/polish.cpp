// Host side of the Newton polish (polish.h): the parts of the refusal, and the loop -- the gradient, the Hessian and its shift
// written on the device, the factorisation (hess.cpp: hess_refactor), spd_vsolve_device, the retraction, one product with M for F(Z), and a handful of scalars read
// back per try through the group's read-back flag.  The matrix is the covariance's (cov.cpp): its pattern, its symbolic
// analysis and its numeric context are shared.  The optimiser's state is not touched (cert_begin).  The loop itself is
// polish_loop: what differs between the trivial loss and the robust objective (robust.cpp) is launched by three hooks.
#include "polish.h"

#include <algorithm>
#include <chrono>
#include <cmath>

#include "cert_state.h"
#include "cov_state.h"
#include "group.h"

namespace dpgo {

// The analysis and the refusal of polish, robust_polish and gnc, then what polish allocates (first call that is not refused):
// the numeric phase, the vector solve with the three vectors -- still to allocate where no earlier polish has left them -- and
// the caller's extra bytes (robust.cpp, gnc.cpp); not the blocks of the selected inversion.
int Group::polish_setup(long long max_bytes, HessAnalysis &out, HessPart extra) {
  if (cov_analyse(out) != 0) return -1;
  CovState &s = *cov_;
  const long long n = s.A.n, vectors = (long long)spd_vsolve_bytes(s.F) + 3ll * 8ll * n;
  const int ready = hess_reserve(max_bytes, "polish", {s.numeric_part(), {vectors, s.pol_g.p ? 0 : vectors}, extra}, out);
  if (ready == 0 && !s.pol_g.p)
    for (DevBuf<double> *b : {&s.pol_g, &s.pol_sol, &s.pol_hdiag}) b->alloc((size_t)std::max<long long>(n, 1));
  return ready;
}

int Group::polish(const double *X, int ld, int anchor, const PolishOptions &o, long long max_bytes, double *Xout, int ldout,
                  double *log, int log_cap, PolishResult &out) {
  out = PolishResult();
  const int rows = (d_ + 1) * num_poses_global_;
  if (!Xout || ldout < rows || o.max_steps < 0 || o.max_tries < 1 || !(o.rel_tol >= 0) || !(o.grad_tol >= 0) || log_cap < 0 ||
      (log_cap > 0 && !log)) {
    fprintf(stderr, "[dpgo_amd] ERROR: polish: bad options or inconsistent size of the output.\n");
    return -1;
  }
  if (cov_begin(X, ld, anchor) != 0) return -1;
  const int ready = polish_setup(max_bytes, out);
  if (ready < 0) return -1;
  if (ready != 0) return 0;   // SKIPPED, with what the analysis predicts
  CertState &c = *cert_;
  CovState &s = *cov_;
  const int arow = own_row(anchor);
  const NodeMask all{all_bits(), nullptr};
  PolishHooks hooks;
  hooks.point = [&] {
    cert_apply_M(c.X.p, c.MX.p);
    launch_cert_lambda(lc(all), c.X.p, c.MX.p, c.Lam.p, nullptr, c.partials.p);
    launch_polish_grad(lc(all), c.X.p, c.MX.p, arow, s.pol_g.p, 0, 1, c.partials.p);
  };
  hooks.hessian = [&] { launch_cov_hessian_at(arow); };
  hooks.trial = [&] {
    cert_apply_M(c.V.p, c.SV.p);
    launch_polish_grad(lc(all), c.V.p, c.SV.p, arow, nullptr, -1, 2, c.partials.p);
  };
  return polish_loop(X, ld, arow, o, hooks, Xout, ldout, log, log_cap, out);
}

int Group::polish_loop(const double *X, int ld, int arow, const PolishOptions &o, const PolishHooks &hooks, double *Xout, int ldout,
                       double *log, int log_cap, PolishResult &out) {
  CertState &c = *cert_;
  CovState &s = *cov_;
  const size_t n = (size_t)s.A.n;
  const NodeMask all{all_bits(), nullptr};
  typedef std::chrono::steady_clock Clock;
  auto ms_since = [](Clock::time_point t) { return 1e3 * std::chrono::duration<double>(Clock::now() - t).count(); };
  const auto t_start = Clock::now();
  const double *h = c.h_sums;
  cert_upload(X, ld, d_, c.X.p);
  double mu = 0;
  out.outcome = POLISH_STALLED;
  for (int k = 0; k <= o.max_steps; k++) {
    // g, |g|, F0, H and hmax at X; the first try's shift rides along
    hooks.point();
    HIP_CHECK(hipStreamSynchronize(st_));   // (the product and the gradient are other_ms: the clock of factor_ms starts behind them)
    auto t0 = Clock::now();
    hooks.hessian();
    launch_polish_shift(lc(all), c.bptr.p, c.diag_pose.p, arow, mu, true, s.pol_hdiag.p, spd_numeric_values(s.F), 2, c.partials.p);
    launch_polish_reduce(st_, T_, 3, 1u << 2, c.partials.p, c.h_sums, sched_.flag());
    wait_flag(sched_.last_seq());
    out.factor_ms += ms_since(t0);
    const double gn = std::sqrt(h[0]), F0 = h[1], hmax = std::isfinite(h[2]) ? h[2] : 0.0, mu_in = mu;
    if (k == 0) {
      out.F_initial = F0;
      out.grad_initial = gn;
    }
    out.F_final = F0;
    out.grad_final = gn;
    out.hmax = hmax;
    double *row = k < log_cap ? log + (size_t)k * POLISH_LOG_COLS : nullptr;
    if (row) {
      row[0] = F0; row[1] = gn; row[2] = mu_in; row[3] = 0.0; row[4] = 0.0;
    }
    if (gn <= (o.grad_tol > 0 ? o.grad_tol : o.rel_tol * hmax)) {
      out.outcome = POLISH_CONVERGED;
      break;
    }
    if (k == o.max_steps) {
      out.outcome = POLISH_MAX_STEPS;
      break;
    }
    bool accepted = false;
    int tries = 0;
    double rho = 0;
    for (int t = 0; t < o.max_tries && !accepted; t++) {
      tries++;
      t0 = Clock::now();
      if (t > 0) launch_polish_shift(lc(all), c.bptr.p, c.diag_pose.p, arow, mu, false, s.pol_hdiag.p, spd_numeric_values(s.F), 2, c.partials.p);
      const int rc = hess_refactor("polish", out);   // (the shift sits between the write and the factorisation: no hess_factor)
      out.factor_ms += ms_since(t0);
      out.factorisations++;
      if (rc < 0) return -1;
      if (rc != 0) {
        if (mu == 0) out.indefinite++;
        mu = std::max(10 * mu, 1e-3 * hmax);
        continue;
      }
      t0 = Clock::now();
      HIP_CHECK(hipMemcpyAsync(s.pol_sol.p, s.pol_g.p, sizeof(double) * n, hipMemcpyDeviceToDevice, st_));
      if (spd_vsolve_device(s.F, s.pol_sol.p, st_) != 0) {
        fprintf(stderr, "[dpgo_amd] ERROR: polish: the solve failed on the device.\n");
        return -1;
      }
      launch_polish_retract(lc(all), c.X.p, s.pol_sol.p, s.pol_g.p, arow, c.V.p, 0, 1, c.partials.p);
      hooks.trial();
      launch_polish_reduce(st_, T_, 3, 0u, c.partials.p, c.h_sums, sched_.flag());
      wait_flag(sched_.last_seq());
      out.solve_ms += ms_since(t0);
      const double gd = h[0], dd = h[1], F1 = h[2];
      const double pred = -0.5 * gd + 0.5 * mu * dd;
      rho = pred > 0 ? (F0 - F1) / pred : -1.0;
      if (rho >= 0.1 || std::fabs(F0 - F1) <= 1e-13 * std::fabs(F0)) {   // (at the rounding floor rho is noise)
        HIP_CHECK(hipMemcpyAsync(c.X.p, c.V.p, sizeof(double) * (size_t)P0_ * RS_, hipMemcpyDeviceToDevice, st_));
        accepted = true;
        out.steps++;
        if (rho > 0.75) {
          mu = mu / 10;
          if (mu < 1e-8 * hmax) mu = 0;
        }
      } else {
        mu = std::max(10 * mu, 1e-3 * hmax);
      }
    }
    if (row) {
      row[3] = accepted ? rho : 0.0;
      row[4] = tries;
    }
    if (!accepted) break;   // STALLED: X is the last accepted point
  }
  out.mu_final = mu;
  cert_download(c.X.p, Xout, ldout, d_);
  out.total_ms = ms_since(t_start);
  out.other_ms = out.total_ms - out.factor_ms - out.solve_ms;
  return 0;
}

}  // namespace dpgo
