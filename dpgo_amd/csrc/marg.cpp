// Host side of the joint marginals (marg.h): the column plan, the dense factor of order n and its cache, the parts of the
// refusal, and the loop -- H written on the device (k_cov_hessian) and factored (hess.cpp: hess_factor), the unit columns of the
// kept poses solved batch by batch (spd_msolve_device), Sigma_KK gathered, the relative covariance, the dense inverse and the
// log-determinant.  The matrix is the covariance's (cov.cpp): its pattern, its symbolic analysis and its numeric context are
// shared.  The optimiser's state is not touched (cert_begin).
#include "marg.h"

#include <algorithm>
#include <chrono>
#include <cmath>

#include "cert_state.h"
#include "cov.h"
#include "cov_state.h"
#include "group.h"
#include "marg_math.h"
#include "pairs.h"

namespace dpgo {

MargPlan marg_plan(int dof, int anchor, const int *keep, int K) {
  MargPlan pl;
  pl.col.assign((size_t)std::max(K, 0), -1);
  for (int i = 0; i < K; i++)
    if (keep[i] != anchor) {
      pl.col[i] = dof * (int)pl.poses.size();
      pl.poses.push_back(keep[i]);
    }
  pl.columns = dof * (int)pl.poses.size();
  pairs_plan_sizes(pl.columns, &pl.batches, &pl.kb);
  return pl;
}

// ---- the dense factor ----
MargDense::~MargDense() {
  spd_release_numeric(F);
  spd_release_device(F);
}

// A dense pattern of order n is a clique, which no dissection can cut; with leaf = n it is not even tried.  What the rest of
// this file relies on is checked: one front, w = n, u = 0.
MargDense *MargCache::get(int n) {
  auto it = by_n.find(n);
  if (it != by_n.end()) return it->second.get();
  if (n < 1 || (long long)n * n > 0x7fffffffll) {
    fprintf(stderr, "[dpgo_amd] ERROR: joint_marginal: a dense matrix of order %d has more than 2^31 entries.\n", n);
    return nullptr;
  }
  std::unique_ptr<MargDense> D(new MargDense());
  D->A.n = n;
  D->A.ptr.resize((size_t)n + 1);
  D->A.col.resize((size_t)n * n);
  for (int i = 0; i <= n; i++) D->A.ptr[i] = i * n;
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) D->A.col[(size_t)i * n + j] = j;
  D->F.quiet = true;   // a non-positive pivot is a verdict here (info_not_pd)
  if (spd_symbolic(D->A, D->F, n, 1, 1) != 0 || D->F.nfronts != 1 || D->F.w[0] != n || D->F.u[0] != 0) {
    fprintf(stderr, "[dpgo_amd] ERROR: joint_marginal: the dense pattern of order %d is not one front.\n", n);
    return nullptr;
  }
  D->bytes = (long long)spd_numeric_bytes(D->F, (long long)n * n) + (long long)spd_selinv_bytes(D->F) + 4ll * n;
  MargDense *p = D.get();
  by_n[n] = std::move(D);
  return p;
}

int marg_dense_prepare(MargDense &D) {
  if (D.F.numeric) return 0;
  if (spd_prepare_device(D.A, D.F) != 0) {
    fprintf(stderr, "[dpgo_amd] ERROR: joint_marginal: the device state of the dense factorisation could not be set up.\n");
    return -1;
  }
  return 0;
}

int marg_dense_invert(MargDense &D, hipStream_t st, double *d_info, double *d_logdet, double *pivots) {
  SpdFactor &F = D.F;
  const int n = F.n;
  const int rc = spd_refactor_device(F, st, false);   // (returns with the verdict read)
  if (rc != 0 && !F.not_pd) {
    fprintf(stderr, "[dpgo_amd] ERROR: joint_marginal: the dense factorisation failed on the device.\n");
    return -1;
  }
  pivots[1] = F.pivot_max;
  pivots[0] = F.pivot_max > 0 ? F.pivot_min : 0.0;
  if (rc != 0) return 1;
  if (spd_selinv_device(F, st) != 0) {
    fprintf(stderr, "[dpgo_amd] ERROR: joint_marginal: the dense inversion failed on the device.\n");
    return -1;
  }
  // the root's block is (w x w, pivots in the factor's order): back through piv_idx.  The list travels with every call: it is n ints.
  DevBuf<int> d_piv;
  d_piv.upload(std::vector<int>(F.piv_idx.begin() + F.piv_ptr[0], F.piv_idx.begin() + F.piv_ptr[0] + n));
  launch_marg_scatter(st, n, d_piv.p, spd_selinv_values(F), d_info);
  launch_marg_logdet(st, n, F.dev_W + F.w_off[0], F.ldw[0], d_logdet);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(st));   // (d_piv is this function's)
  return 0;
}

// ---- the call ----
void Group::marg_release() {
  delete marg_;
  marg_ = nullptr;
}

// The batches of a column plan behind a factorisation that succeeded (joint_marginal, candidate_set): per batch the unit
// right-hand sides, the block solve and the gather of Sigma_KK's entries whose columns it holds, into g1 and (optional) g2 (device,
// (dof K)^2, the anchor's blocks zeroed by the caller).  d_prow <- the record of every kept pose; returns behind a synchronise.
int Group::marg_sigma(const MargPlan &pl, const int *keep, int K, double *g1, double *g2, DevBuf<int> &d_prow, const char *who) {
  CovState &s = *cov_;
  const int dof = cov_dof(d_);
  const long long ns = (long long)dof * K, nh = (long long)dof * P0_;
  // the lists: per row / column of Sigma_KK the unknown of H and the plan's column (-1: the anchor), per kept pose its record
  std::vector<int> row_unk((size_t)ns, -1), col_of((size_t)ns, -1), prow((size_t)K), col_unknown((size_t)std::max(pl.columns, 1), 0);
  for (int i = 0; i < K; i++) {
    prow[i] = own_row(keep[i]);
    if (pl.col[i] < 0) continue;
    for (int a = 0; a < dof; a++) {
      row_unk[(size_t)dof * i + a] = dof * prow[i] + a;
      col_of[(size_t)dof * i + a] = pl.col[i] + a;
      col_unknown[(size_t)pl.col[i] + a] = dof * prow[i] + a;
    }
  }
  DevBuf<int> d_row, d_colof, d_unk;
  DevBuf<double> d_Xb;
  d_row.upload(row_unk);
  d_colof.upload(col_of);
  d_prow.upload(prow);
  d_unk.upload(col_unknown);
  d_Xb.alloc((size_t)nh * pl.kb, false);
  for (int b = 0; b < pl.batches; b++) {
    const int c0 = b * PAIRS_BATCH, nc = std::min(PAIRS_BATCH, pl.columns - c0);
    HIP_CHECK(hipMemsetAsync(d_Xb.p, 0, sizeof(double) * (size_t)nh * pl.kb, st_));
    launch_pairs_rhs(st_, d_unk.p, c0, nc, d_Xb.p, pl.kb);
    if (spd_msolve_device(s.F, d_Xb.p, nc, pl.kb, st_) != 0) {
      fprintf(stderr, "[dpgo_amd] ERROR: %s: the solve failed on the device.\n", who);
      return -1;
    }
    launch_marg_gather(st_, (int)ns, d_row.p, d_colof.p, c0, nc, d_Xb.p, pl.kb, g1, g2);
  }
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(st_));   // (the batch block and the lists are this function's)
  return 0;
}

int Group::joint_marginal(const double *X, int ld, const int *keep, int K, int anchor, int base, bool want_info, long long max_bytes,
                          double *cov, double *info, double *logdet, MargResult &out) {
  out = MargResult();
  if (K < 1 || !keep || !cov || !logdet || (want_info && !info)) {
    fprintf(stderr, "[dpgo_amd] ERROR: joint_marginal: missing output or pose arrays.\n");
    return -1;
  }
  if (cov_begin(X, ld, anchor) != 0) return -1;
  const int d = d_, dof = cov_dof(d), N = P0_;
  int bpos = -1;
  {
    std::vector<int> sorted(keep, keep + K);
    std::sort(sorted.begin(), sorted.end());
    if (sorted.front() < 0 || sorted.back() >= N) {
      fprintf(stderr, "[dpgo_amd] ERROR: joint_marginal: a kept pose is not in the graph.\n");
      return -1;
    }
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) {
      fprintf(stderr, "[dpgo_amd] ERROR: joint_marginal: a pose is kept twice.\n");
      return -1;
    }
  }
  if (base < 0) {
    if (std::find(keep, keep + K, anchor) != keep + K) {
      fprintf(stderr, "[dpgo_amd] ERROR: joint_marginal: the anchor %d is kept in the absolute form: its block is exactly zero "
                      "and no information form exists (name a base for the relative form).\n", anchor);
      return -1;
    }
  } else {
    bpos = (int)(std::find(keep, keep + K, base) - keep);
    if (bpos == K || K < 2) {
      fprintf(stderr, "[dpgo_amd] ERROR: joint_marginal: the base %d must be one of at least two kept poses.\n", base);
      return -1;
    }
  }
  const bool relative = base >= 0;
  const MargPlan pl = marg_plan(dof, anchor, keep, K);
  const long long ns = (long long)dof * K, n = relative ? ns - dof : ns, nh = (long long)dof * N;
  out.n = (int)n;
  out.columns = pl.columns;
  out.batches = pl.batches;
  if (!marg_) marg_ = new MargCache();
  MargDense *D = want_info ? marg_->get((int)n) : nullptr;   // (the symbolic analysis of the dense factor: nothing allocated)
  if (want_info && !D) return -1;
  if (cov_analyse(out) != 0) return -1;
  CertState &c = *cert_;
  CovState &s = *cov_;
  // this call's buffers: the batch block, Sigma_KK (the relative form), cov, info and logdet, the lists
  const long long own = 8ll * (nh * pl.kb + (relative ? ns * ns : 0) + n * n + (want_info ? n * n + 1 : 0)) + 4ll * (2 * ns + pl.columns + K);
  const long long solve = (long long)spd_msolve_bytes(s.F, pl.kb);
  const HessPart dense = {D ? D->bytes : 0, D && !D->F.numeric ? D->bytes : 0};
  const int ready = hess_reserve(max_bytes, "joint_marginal", {s.numeric_part(), {solve, solve}, {own, own}, dense}, out);
  if (ready < 0) return -1;
  cert_prepare(X, ld, &out.stationarity);
  if (ready != 0) return 0;   // SKIPPED, with what the analyses and the plan predict
  std::fill(cov, cov + (size_t)(n * n), 0.0);
  if (want_info) std::fill(info, info + (size_t)(n * n), 0.0);
  *logdet = 0.0;
  typedef std::chrono::steady_clock Clock;
  auto ms_since = [](Clock::time_point t) { return 1e3 * std::chrono::duration<double>(Clock::now() - t).count(); };
  const int rc = hess_factor("joint_marginal", [&] { launch_cov_hessian_at(own_row(anchor)); }, out);
  if (rc < 0) return -1;
  out.outcome = rc != 0 ? MARG_NOT_PD : MARG_OK;
  if (rc != 0) return 0;
  auto t0 = Clock::now();
  if (D && marg_dense_prepare(*D) != 0) return -1;
  DevBuf<int> d_prow;
  DevBuf<double> d_sig, d_cov, d_info;
  d_cov.alloc((size_t)(n * n));
  if (relative) d_sig.alloc((size_t)(ns * ns));   // (zeroed: the anchor's blocks)
  if (want_info) d_info.alloc((size_t)(n * n) + 1);
  double *dense_val = D ? spd_numeric_values(D->F) : nullptr;
  // the absolute form gathers straight into the dense factor's value array (CSR order == row-major) and into cov
  double *g1 = relative ? d_sig.p : (dense_val ? dense_val : d_cov.p), *g2 = relative || !dense_val ? nullptr : d_cov.p;
  if (marg_sigma(pl, keep, K, g1, g2, d_prow, "joint_marginal") != 0) return -1;
  if (relative) launch_marg_rel(d, st_, K, bpos, d_prow.p, c.X.p, d_sig.p, d_cov.p, dense_val);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(cov, d_cov.p, sizeof(double) * (size_t)(n * n), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
  out.solve_ms = ms_since(t0);
  if (!D) return 0;
  t0 = Clock::now();
  double piv[2] = {0, 0};
  const int drc = marg_dense_invert(*D, st_, d_info.p, d_info.p + (size_t)(n * n), piv);
  if (drc < 0) return -1;
  out.dense_pivot_min = piv[0];
  out.dense_pivot_max = piv[1];
  out.info_not_pd = drc != 0;
  if (drc == 0) {
    HIP_CHECK(hipMemcpyAsync(info, d_info.p, sizeof(double) * (size_t)(n * n), hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipMemcpyAsync(logdet, d_info.p + (size_t)(n * n), sizeof(double), hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
  }
  out.dense_ms = ms_since(t0);
  return 0;
}

// ---- the test hooks ----
namespace {
template <int D>
void rel_host(int K, int b, const double *X, const double *sig, double *cov) {
  typedef PairsDims<D> P;
  const int m = K - 1;
  for (int ko = 0; ko < m; ko++)
    for (int lo = 0; lo <= ko; lo++) {
      const int k = ko + (ko >= b ? 1 : 0), l = lo + (lo >= b ? 1 : 0);
      marg_rel_block<D>(X + (size_t)b * P::RS, X + (size_t)k * P::RS, X + (size_t)l * P::RS, sig, (long long)P::DOF * K, b, k, l, ko,
                        lo, cov, nullptr, (long long)P::DOF * m);
    }
}
// a stream for the length of a hook (the dense factor's kernels and this file's run on one stream, in order)
struct HookStream {
  hipStream_t st = nullptr;
  HookStream() { HIP_CHECK(hipStreamCreate(&st)); }
  ~HookStream() { if (st) (void)hipStreamDestroy(st); }
};
bool rel_args_ok(int d, int K, int b, const double *X, const double *sig, const double *cov) {
  return (d == 2 || d == 3) && K >= 2 && K <= 4096 && b >= 0 && b < K && X && sig && cov;
}
}  // namespace

int marg_rel_host(int d, int K, int b, const double *X, const double *sig, double *cov) {
  if (!rel_args_ok(d, K, b, X, sig, cov)) return -1;
  if (d == 3) rel_host<3>(K, b, X, sig, cov);
  else rel_host<2>(K, b, X, sig, cov);
  return 0;
}

// k_marg_rel alone on the caller's arrays (host pointers), on the current device's null stream
int marg_rel_device(int d, int K, int b, const double *X, const double *sig, double *cov) {
  if (!rel_args_ok(d, K, b, X, sig, cov)) return -1;
  const size_t dof = (size_t)cov_dof(d), ns = dof * K, n = dof * (K - 1), rs = (size_t)(d + 1) * d;
  std::vector<int> prow((size_t)K);
  for (int i = 0; i < K; i++) prow[i] = i;
  DevBuf<int> d_prow;
  DevBuf<double> d_X, d_sig, d_cov;
  d_prow.upload(prow);
  d_X.upload(std::vector<double>(X, X + rs * K));
  d_sig.upload(std::vector<double>(sig, sig + ns * ns));
  d_cov.alloc(n * n);
  launch_marg_rel(d, nullptr, K, b, d_prow.p, d_X.p, d_sig.p, d_cov.p, nullptr);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpy(cov, d_cov.p, sizeof(double) * n * n, hipMemcpyDeviceToHost));
  return 0;
}

int marg_dense_device(int n, const double *A, double *cov, double *info, double *logdet, MargResult &out) {
  out = MargResult();
  if (n < 1 || !A || !cov || !info || !logdet) return -1;
  MargCache cache;
  MargDense *D = cache.get(n);
  if (!D) return -1;
  out.n = n;
  out.columns = n;
  int kb = 0;
  pairs_plan_sizes(n, &out.batches, &kb);
  out.device_bytes = D->bytes;
  out.fronts = D->F.nfronts;
  out.max_front = D->F.max_front;
  out.unknowns = n;
  out.levels = (int)D->F.by_height.size();
  const size_t nn = (size_t)n * n;
  std::fill(info, info + nn, 0.0);
  *logdet = 0.0;
  if (marg_dense_prepare(*D) != 0) return -1;
  HookStream hs;
  const auto t0 = std::chrono::steady_clock::now();
  // the matrix travels as the call's solved batches do: 64 columns at a time in a block of row length kb
  std::vector<int> ident((size_t)n);
  for (int i = 0; i < n; i++) ident[i] = i;
  std::vector<double> Xb((size_t)n * kb);
  DevBuf<int> d_id;
  DevBuf<double> d_Xb, d_cov, d_info;
  d_id.upload(ident);
  d_Xb.alloc(Xb.size(), false);
  d_cov.alloc(nn);
  d_info.alloc(nn + 1);
  for (int b = 0; b < out.batches; b++) {
    const int c0 = b * PAIRS_BATCH, nc = std::min(PAIRS_BATCH, n - c0);
    std::fill(Xb.begin(), Xb.end(), 0.0);
    for (int i = 0; i < n; i++)
      for (int j = 0; j < nc; j++) Xb[(size_t)i * kb + j] = A[(size_t)i * n + c0 + j];
    HIP_CHECK(hipMemcpy(d_Xb.p, Xb.data(), sizeof(double) * Xb.size(), hipMemcpyHostToDevice));
    launch_marg_gather(hs.st, n, d_id.p, d_id.p, c0, nc, d_Xb.p, kb, spd_numeric_values(D->F), d_cov.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(hs.st));
  }
  HIP_CHECK(hipMemcpy(cov, d_cov.p, sizeof(double) * nn, hipMemcpyDeviceToHost));
  double piv[2] = {0, 0};
  const int rc = marg_dense_invert(*D, hs.st, d_info.p, d_info.p + nn, piv);
  if (rc < 0) return -1;
  out.dense_pivot_min = piv[0];
  out.dense_pivot_max = piv[1];
  out.info_not_pd = rc != 0;
  if (rc == 0) {
    HIP_CHECK(hipMemcpy(info, d_info.p, sizeof(double) * nn, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(logdet, d_info.p + nn, sizeof(double), hipMemcpyDeviceToHost));
  }
  out.dense_ms = 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  out.outcome = MARG_OK;
  return 0;
}

}  // namespace dpgo
