// Host side of the candidate sets (cand.h): the pose list, the parts of the refusal, and the call -- H written on the device and
// factored (hess.cpp: hess_factor), Sigma_KK of the candidates' end poses by joint_marginal's batches (marg.cpp: marg_sigma), the
// joint innovation covariance (k_cand_innov), the joint test on marg.h's dense factor and the selection loop.  The matrix is the
// covariance's (cov.cpp).  The optimiser's state is not touched (cert_begin).
#include "cand.h"

#include <algorithm>
#include <chrono>
#include <cmath>

#include "cand_math.h"
#include "cert_state.h"
#include "cov.h"
#include "cov_state.h"
#include "group.h"
#include "pairs.h"

namespace dpgo {

void cand_pose_list(const int *pairs, int m, std::vector<int> &K, std::vector<int> &kpos) {
  K.clear();
  kpos.assign((size_t)2 * std::max(m, 0), 0);
  for (int k = 0; k < 2 * m; k++) {
    const auto it = std::find(K.begin(), K.end(), pairs[k]);
    kpos[k] = (int)(it - K.begin());
    if (it == K.end()) K.push_back(pairs[k]);
  }
}

// ---- the selection ----
namespace {
int steps_of(int m, int budget) { return std::max(0, std::min(budget, m)); }   // after m steps every candidate is taken
}  // namespace

long long cand_select_bytes(int dof, int m, int budget) {
  const long long n = (long long)dof * m, ns = steps_of(m, budget);
  return 8ll * (n * dof * ns + n * dof + n + 4ll * budget + 2 + dof * dof + dof) + 4ll * (3 + m + budget);
}

int cand_select_run(int d, hipStream_t st, int m, int budget, double d2_max, const double *d_S, const double *d_r, const double *d_winv,
                    int *selected, double *steps, double *sums, int *n_selected) {
  const int dof = cov_dof(d), ns = steps_of(m, budget);
  const size_t n = (size_t)dof * m;
  DevBuf<int> d_state, d_taken, d_sel;
  DevBuf<double> d_steps, d_sums, d_piv, d_P, d_C, d_rho;
  d_state.alloc(3);
  d_taken.alloc((size_t)m);
  d_sel.upload(std::vector<int>(selected, selected + budget));
  d_steps.upload(std::vector<double>(steps, steps + 4 * (size_t)budget));
  d_sums.alloc(2);
  d_piv.alloc((size_t)dof * dof + dof);
  d_P.alloc(std::max<size_t>(n * dof * ns, 1), false);
  d_C.alloc(n * dof, false);
  d_rho.alloc(n, false);
  const CandSelectBufs b = {d_state.p, d_taken.p, d_sel.p, d_steps.p, d_sums.p, d_piv.p, d_P.p, d_C.p, d_rho.p};
  launch_cand_select_init(d, st, m, d_S, d_r, b);
  for (int t = 0; t < ns; t++) {
    launch_cand_score(d, st, m, t, d2_max, d_winv, b);
    if (t + 1 < ns) launch_cand_update(d, st, m, t, d_S, b);   // (nothing reads the last step's panel)
  }
  HIP_CHECK(hipGetLastError());
  int state[3] = {0, 0, 0};
  HIP_CHECK(hipMemcpyAsync(selected, d_sel.p, sizeof(int) * (size_t)budget, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(steps, d_steps.p, sizeof(double) * 4 * (size_t)budget, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(sums, d_sums.p, sizeof(double) * 2, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(state, d_state.p, sizeof(int) * 3, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  *n_selected = state[2];
  return 0;
}

// ---- the call ----
int Group::candidate_set(const double *X, int ld, const int *pairs, int m, const double *candidates, int anchor, int budget,
                         double d2_max, bool want_joint, long long max_bytes, const CandOut &o, CandResult &out) {
  out = CandResult();
  if (m < 1 || !pairs || !candidates || budget < 0 || !o.residual || !o.scalars || !o.poses || (want_joint && !o.info) ||
      (budget > 0 && (!o.selected || !o.steps))) {
    fprintf(stderr, "[dpgo_amd] ERROR: candidate_set: missing output, pair or candidate arrays, or a negative budget.\n");
    return -1;
  }
  if (cov_begin(X, ld, anchor) != 0) return -1;
  const int d = d_, dof = cov_dof(d), N = P0_, ncand = d * d + d + 2;
  if (!pairs_args_ok("candidate_set", pairs, m)) return -1;
  if ((long long)dof * m > 46340) {
    fprintf(stderr, "[dpgo_amd] ERROR: candidate_set: a dense matrix of order %lld has more than 2^31 entries.\n", (long long)dof * m);
    return -1;
  }
  for (int k = 0; k < m; k++) {
    if (pairs[2 * k] == pairs[2 * k + 1]) {
      fprintf(stderr, "[dpgo_amd] ERROR: candidate_set: candidate %d joins pose %d to itself.\n", k, pairs[2 * k]);
      return -1;
    }
    const double kappa = candidates[(size_t)k * ncand + d * d + d], tau = candidates[(size_t)k * ncand + d * d + d + 1];
    if (!(kappa > 0) || !(tau > 0) || !std::isfinite(kappa) || !std::isfinite(tau)) {
      fprintf(stderr, "[dpgo_amd] ERROR: candidate_set: candidate %d has a weight that is not positive.\n", k);
      return -1;
    }
  }
  std::vector<int> K, kpos;
  cand_pose_list(pairs, m, K, kpos);
  const int nK = (int)K.size();
  const MargPlan pl = marg_plan(dof, anchor, K.data(), nK);
  const long long ns = (long long)dof * nK, n = (long long)dof * m, nh = (long long)dof * N;
  out.n = (int)n;
  out.poses = nK;
  out.columns = pl.columns;
  out.batches = pl.batches;
  std::copy(K.begin(), K.end(), o.poses);
  if (!marg_) marg_ = new MargCache();
  MargDense *D = want_joint ? marg_->get((int)n) : nullptr;   // (the symbolic analysis of the dense factor: nothing allocated)
  if (want_joint && !D) return -1;
  if (cov_analyse(out) != 0) return -1;
  CertState &c = *cert_;
  CovState &s = *cov_;
  // this call's buffers: the batch block, Sigma_KK, cov, S, r and the reciprocal weights, the candidates, the joint test's
  // inverse and two scalars, the selection's workspace, the lists (marg_sigma's and kpos)
  const long long own = 8ll * (nh * pl.kb + ns * ns + 2 * n * n + n + 2ll * m + (long long)m * ncand + (want_joint ? n * n + 2 : 0)) +
                        4ll * (2 * ns + pl.columns + nK + 2ll * m) + (budget > 0 ? cand_select_bytes(dof, m, budget) : 0);
  const long long solve = (long long)spd_msolve_bytes(s.F, pl.kb);
  const HessPart dense = {D ? D->bytes : 0, D && !D->F.numeric ? D->bytes : 0};
  const int ready = hess_reserve(max_bytes, "candidate_set", {s.numeric_part(), {solve, solve}, {own, own}, dense}, out);
  if (ready < 0) return -1;
  cert_prepare(X, ld, &out.stationarity);
  if (ready != 0) return 0;   // SKIPPED, with what the analyses and the plan predict
  if (o.cov) std::fill(o.cov, o.cov + (size_t)(n * n), 0.0);
  if (o.S) std::fill(o.S, o.S + (size_t)(n * n), 0.0);
  if (want_joint) std::fill(o.info, o.info + (size_t)(n * n), 0.0);
  std::fill(o.residual, o.residual + (size_t)n, 0.0);
  std::fill(o.scalars, o.scalars + 5, 0.0);
  if (budget > 0) {
    std::fill(o.selected, o.selected + budget, -1);
    std::fill(o.steps, o.steps + 4 * (size_t)budget, 0.0);
  }
  typedef std::chrono::steady_clock Clock;
  auto ms_since = [](Clock::time_point t) { return 1e3 * std::chrono::duration<double>(Clock::now() - t).count(); };
  const int rc = hess_factor("candidate_set", [&] { launch_cov_hessian_at(own_row(anchor)); }, out);
  if (rc < 0) return -1;
  out.outcome = rc != 0 ? CAND_NOT_PD : CAND_OK;
  if (rc != 0) return 0;
  auto t0 = Clock::now();
  if (D && marg_dense_prepare(*D) != 0) return -1;
  DevBuf<int> d_prow, d_kpos;
  DevBuf<double> d_sig, d_cov, d_S, d_r, d_winv, d_cand, d_info;
  d_kpos.upload(kpos);
  d_cand.upload(std::vector<double>(candidates, candidates + (size_t)m * ncand));
  d_sig.alloc((size_t)(ns * ns));   // (zeroed: the anchor's blocks)
  d_cov.alloc((size_t)(n * n), false);
  d_S.alloc((size_t)(n * n), false);
  d_r.alloc((size_t)n, false);
  d_winv.alloc((size_t)2 * m, false);
  if (want_joint) d_info.alloc((size_t)(n * n) + 2);
  if (marg_sigma(pl, K.data(), nK, d_sig.p, nullptr, d_prow, "candidate_set") != 0) return -1;
  launch_cand_resid(d, st_, m, d_prow.p, d_kpos.p, c.X.p, d_cand.p, d_r.p, d_winv.p);
  launch_cand_innov(d, st_, m, nK, d_prow.p, d_kpos.p, c.X.p, d_sig.p, d_winv.p, d_cov.p, d_S.p, D ? spd_numeric_values(D->F) : nullptr);
  HIP_CHECK(hipGetLastError());
  if (o.cov) HIP_CHECK(hipMemcpyAsync(o.cov, d_cov.p, sizeof(double) * (size_t)(n * n), hipMemcpyDeviceToHost, st_));
  if (o.S) HIP_CHECK(hipMemcpyAsync(o.S, d_S.p, sizeof(double) * (size_t)(n * n), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipMemcpyAsync(o.residual, d_r.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
  out.solve_ms = ms_since(t0);
  if (D) {
    t0 = Clock::now();
    double piv[2] = {0, 0};
    double *d_logdet = d_info.p + (size_t)(n * n), *d_quad = d_logdet + 1;
    const int drc = marg_dense_invert(*D, st_, d_info.p, d_logdet, piv);
    if (drc < 0) return -1;
    out.dense_pivot_min = piv[0];
    out.dense_pivot_max = piv[1];
    out.joint_not_pd = drc != 0;
    if (drc == 0) {
      launch_cand_quad(st_, (int)n, d_info.p, d_r.p, d_quad);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipMemcpyAsync(o.info, d_info.p, sizeof(double) * (size_t)(n * n), hipMemcpyDeviceToHost, st_));
      HIP_CHECK(hipMemcpyAsync(o.scalars, d_logdet, sizeof(double) * 2, hipMemcpyDeviceToHost, st_));
      HIP_CHECK(hipStreamSynchronize(st_));
      // gain_all = 1/2 (log det S - sum_i log det Omega_i^-1), the sum in candidate order from the reciprocals S's diagonal took
      double lw = 0.0;
      for (int k = 0; k < m; k++) {
        double w[2];
        cand_omega_inv(candidates[(size_t)k * ncand + d * d + d], candidates[(size_t)k * ncand + d * d + d + 1], w);
        lw += d * std::log(w[0]) + (dof - d) * std::log(w[1]);
      }
      o.scalars[2] = 0.5 * (o.scalars[0] - lw);
    }
    out.dense_ms = ms_since(t0);
  }
  if (budget > 0) {
    t0 = Clock::now();
    if (cand_select_run(d, st_, m, budget, d2_max, d_S.p, d_r.p, d_winv.p, o.selected, o.steps, o.scalars + 3, &out.n_selected) != 0)
      return -1;
    out.select_ms = ms_since(t0);
  }
  return 0;
}

// ---- the test hooks ----
namespace {
bool innov_args_ok(int d, int m, int nK, const int *kpos, const double *X, const double *sigma, const double *cand, const double *S,
                   const double *r) {
  if (!((d == 2 || d == 3) && m >= 1 && m <= 4096 && nK >= 2 && nK <= 8192 && kpos && X && sigma && cand && S && r)) return false;
  for (int k = 0; k < 2 * m; k++)
    if (kpos[k] < 0 || kpos[k] >= nK) return false;
  return true;
}

template <int D>
void innov_host(int m, int nK, const int *kpos, const double *X, const double *sig, const double *cand, double *cov, double *S, double *r) {
  typedef PairsDims<D> P;
  std::vector<double> winv((size_t)2 * m);
  for (int i = 0; i < m; i++) {
    const double *c = cand + (size_t)i * P::CAND;
    cand_residual<D>(X + (size_t)kpos[2 * i] * P::RS, X + (size_t)kpos[2 * i + 1] * P::RS, c, r + (size_t)i * P::DOF);
    cand_omega_inv(c[D * D + D], c[D * D + D + 1], &winv[2 * (size_t)i]);
  }
  for (int i = 0; i < m; i++)
    for (int j = 0; j <= i; j++) {
      const int kpi = kpos[2 * i], kqi = kpos[2 * i + 1], kpj = kpos[2 * j], kqj = kpos[2 * j + 1];
      cand_innov_block<D>(X + (size_t)kpi * P::RS, X + (size_t)kqi * P::RS, X + (size_t)kpj * P::RS, X + (size_t)kqj * P::RS, sig,
                          (long long)P::DOF * nK, kpi, kqi, kpj, kqj, i, j, &winv[2 * (size_t)i], cov, S, nullptr, (long long)P::DOF * m);
    }
}

// the selection's steps on the host, with cand_math.h's functions in the kernels' order
template <int D>
void select_host(int m, int budget, double d2_max, const double *S, const double *r, const double *winv, int *selected, double *steps,
                 double *sums, int *n_selected) {
  constexpr int DOF = PairsDims<D>::DOF;
  const long long n = (long long)DOF * m;
  const int ns = steps_of(m, budget);
  std::vector<double> C((size_t)n * DOF), rho(r, r + n), P((size_t)std::max<long long>(n * DOF * ns, 1)), piv(DOF * DOF + DOF, 0.0);
  std::vector<int> taken((size_t)m, 0);
  for (long long a = 0; a < n; a++)
    for (int c = 0; c < DOF; c++) C[(size_t)a * DOF + c] = S[a * n + (a / DOF) * DOF + c];
  sums[0] = sums[1] = 0.0;
  *n_selected = 0;
  for (int t = 0; t < ns; t++) {
    double bg = 0.0, bd = 0.0;
    int bi = -1, cnt = 0;
    for (int i = 0; i < m; i++) {
      if (taken[i]) continue;
      double g, d2;
      if (!cand_score_one<D>(&C[(size_t)i * DOF * DOF], &rho[(size_t)i * DOF], winv + 2 * (size_t)i, &g, &d2)) continue;
      if (d2_max > 0.0 && !(d2 <= d2_max)) continue;
      cnt++;
      if (cand_better(g, i, bg, bi)) {
        bg = g;
        bd = d2;
        bi = i;
      }
    }
    if (bi < 0) break;
    *n_selected = t + 1;
    taken[bi] = 1;
    selected[t] = bi;
    steps[4 * (size_t)t] = bi;
    steps[4 * (size_t)t + 1] = bg;
    steps[4 * (size_t)t + 2] = bd;
    steps[4 * (size_t)t + 3] = cnt;
    sums[0] += bg;
    sums[1] += bd;
    if (t + 1 == ns) break;
    double L[DOF * DOF] = {0}, z[DOF], lg, d2;
    (void)cand_chol<D>(&C[(size_t)bi * DOF * DOF], &rho[(size_t)bi * DOF], L, z, &lg, &d2);
    for (int a = 0; a < DOF; a++) {
      for (int cc = 0; cc < DOF; cc++) piv[a * DOF + cc] = cc <= a ? L[a * DOF + cc] : 0.0;
      piv[DOF * DOF + a] = z[a];
    }
    for (long long a = 0; a < n; a++) {
      double x[DOF];
      cand_panel_row<D>(S, P.data(), n, t, bi, a, piv.data(), x);
      for (int cc = 0; cc < DOF; cc++) P[(size_t)(((long long)DOF * t + cc) * n + a)] = x[cc];
    }
    for (long long a = 0; a < n; a++) {
      const long long a0 = (a / DOF) * DOF;
      for (int cc = 0; cc < DOF; cc++) {
        double v = C[(size_t)a * DOF + cc];
        for (int k = 0; k < DOF; k++) v = fma(-P[(size_t)(((long long)DOF * t + k) * n + a)], P[(size_t)(((long long)DOF * t + k) * n + a0 + cc)], v);
        C[(size_t)a * DOF + cc] = v;
      }
      double rh = rho[(size_t)a];
      for (int k = 0; k < DOF; k++) rh = fma(-P[(size_t)(((long long)DOF * t + k) * n + a)], piv[DOF * DOF + k], rh);
      rho[(size_t)a] = rh;
    }
  }
}

bool select_args_ok(int d, int m, int budget, const double *S, const double *r, const double *weights, const int *selected,
                    const double *steps, const double *sums, const int *n_selected) {
  if (!((d == 2 || d == 3) && m >= 1 && m <= 4096 && budget >= 0 && budget <= 1 << 20 && S && r && weights && sums && n_selected))
    return false;
  if (budget > 0 && (!selected || !steps)) return false;
  for (int k = 0; k < 2 * m; k++)
    if (!(weights[k] > 0) || !std::isfinite(weights[k])) return false;
  return true;
}

std::vector<double> winv_of(int m, const double *weights) {
  std::vector<double> w((size_t)2 * m);
  for (int i = 0; i < m; i++) cand_omega_inv(weights[2 * i], weights[2 * i + 1], &w[2 * (size_t)i]);
  return w;
}
}  // namespace

int cand_innov_host(int d, int m, int nK, const int *kpos, const double *X, const double *sigma, const double *cand, double *cov,
                    double *S, double *r) {
  if (!innov_args_ok(d, m, nK, kpos, X, sigma, cand, S, r)) return -1;
  if (d == 3) innov_host<3>(m, nK, kpos, X, sigma, cand, cov, S, r);
  else innov_host<2>(m, nK, kpos, X, sigma, cand, cov, S, r);
  return 0;
}

// the two kernels alone on the caller's arrays (host pointers), on the current device's null stream
int cand_innov_device(int d, int m, int nK, const int *kpos, const double *X, const double *sigma, const double *cand, double *cov,
                      double *S, double *r) {
  if (!innov_args_ok(d, m, nK, kpos, X, sigma, cand, S, r)) return -1;
  const size_t dof = (size_t)cov_dof(d), ns = dof * nK, n = dof * m, rs = (size_t)(d + 1) * d, ncand = (size_t)d * d + d + 2;
  std::vector<int> prow((size_t)nK);
  for (int i = 0; i < nK; i++) prow[i] = i;
  DevBuf<int> d_prow, d_kpos;
  DevBuf<double> d_X, d_sig, d_cand, d_cov, d_S, d_r, d_winv;
  d_prow.upload(prow);
  d_kpos.upload(std::vector<int>(kpos, kpos + 2 * (size_t)m));
  d_X.upload(std::vector<double>(X, X + rs * nK));
  d_sig.upload(std::vector<double>(sigma, sigma + ns * ns));
  d_cand.upload(std::vector<double>(cand, cand + ncand * m));
  d_cov.alloc(n * n);
  d_S.alloc(n * n);
  d_r.alloc(n);
  d_winv.alloc(2 * (size_t)m);
  launch_cand_resid(d, nullptr, m, d_prow.p, d_kpos.p, d_X.p, d_cand.p, d_r.p, d_winv.p);
  launch_cand_innov(d, nullptr, m, nK, d_prow.p, d_kpos.p, d_X.p, d_sig.p, d_winv.p, cov ? d_cov.p : nullptr, d_S.p, nullptr);
  HIP_CHECK(hipGetLastError());
  if (cov) HIP_CHECK(hipMemcpy(cov, d_cov.p, sizeof(double) * n * n, hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(S, d_S.p, sizeof(double) * n * n, hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(r, d_r.p, sizeof(double) * n, hipMemcpyDeviceToHost));
  return 0;
}

int cand_select_host(int d, int m, int budget, double d2_max, const double *S, const double *r, const double *weights, int *selected,
                     double *steps, double *sums, int *n_selected) {
  if (!select_args_ok(d, m, budget, S, r, weights, selected, steps, sums, n_selected)) return -1;
  const std::vector<double> w = winv_of(m, weights);
  if (d == 3) select_host<3>(m, budget, d2_max, S, r, w.data(), selected, steps, sums, n_selected);
  else select_host<2>(m, budget, d2_max, S, r, w.data(), selected, steps, sums, n_selected);
  return 0;
}

int cand_select_device(int d, int m, int budget, double d2_max, const double *S, const double *r, const double *weights, int *selected,
                       double *steps, double *sums, int *n_selected) {
  if (!select_args_ok(d, m, budget, S, r, weights, selected, steps, sums, n_selected)) return -1;
  const size_t n = (size_t)cov_dof(d) * m;
  sums[0] = sums[1] = 0.0;
  *n_selected = 0;
  if (budget == 0) return 0;
  DevBuf<double> d_S, d_r, d_w;
  d_S.upload(std::vector<double>(S, S + n * n));
  d_r.upload(std::vector<double>(r, r + n));
  d_w.upload(winv_of(m, weights));
  return cand_select_run(d, nullptr, m, budget, d2_max, d_S.p, d_r.p, d_w.p, selected, steps, sums, n_selected);
}

}  // namespace dpgo
