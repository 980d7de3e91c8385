// Host side of the Hessian modes (modes.h): the host's small eigenproblem (modes_ritz), the parts of the refusal, the shift
// loop on polish.h's rule, the block iteration -- spd_msolve_device, the Gram matrices and the update on the device, one
// read-back behind each -- and the escape along the most negative mode.  The matrix is the covariance's (cov.cpp): its
// pattern, its symbolic analysis and its numeric context are shared; the verdict is hess_refactor's, as in polish_loop.  The
// optimiser's state is not touched (cert_begin).  What writes H and evaluates F is launched by two hooks, so that the robust
// objective can be put under the same loop as polish.cpp's was.
#include "modes.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

#include "cert_state.h"
#include "cov_state.h"
#include "group.h"

namespace dpgo {

// ---------------------------------------------------------------------------
// Rayleigh-Ritz on the host: order <= 64 (cert.cpp's rayleigh_ritz is written for orders up to 9 and keeps what it returns)
// ---------------------------------------------------------------------------
namespace {
constexpr int MR = MODES_MAX_B;

// cyclic Jacobi: A (n x n, symmetric, overwritten) = Z diag(w) Z^T
void jacobi_eig(int n, double (*A)[MR], double (*Z)[MR], double *w) {
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) Z[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 60; sweep++) {
    double off = 0, diag = 0;
    for (int i = 0; i < n; i++) {
      diag += A[i][i] * A[i][i];
      for (int j = i + 1; j < n; j++) off += A[i][j] * A[i][j];
    }
    if (off <= 1e-34 * (diag + off) || off == 0.0) break;
    for (int p = 0; p < n; p++)
      for (int q = p + 1; q < n; q++) {
        if (A[p][q] == 0.0) continue;
        const double th = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double t = (th >= 0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < n; k++) {   // A <- A J
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq;
          A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < n; k++) {   // A <- J^T A
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk;
          A[q][k] = s * apk + c * aqk;
        }
        A[p][q] = A[q][p] = 0.0;
        for (int k = 0; k < n; k++) {
          const double zkp = Z[k][p], zkq = Z[k][q];
          Z[k][p] = c * zkp - s * zkq;
          Z[k][q] = s * zkp + c * zkq;
        }
      }
  }
  for (int i = 0; i < n; i++) w[i] = A[i][i];
}

struct RitzWork {
  double L[MR][MR], As[MR][MR], Z[MR][MR], w[MR], dscale[MR], c[MR];
  int idx[MR];
};
}  // namespace

int modes_ritz(int b, const double *G, const double *T, double *theta, double *C, int *used_out) {
  if (b < 1 || b > MR || !G || !T || !theta || !C) return -1;
  std::vector<RitzWork> work(1);   // (130 KB: not on the stack)
  RitzWork &k = work[0];
  auto low = [b](const double *M, int i, int j) { return i >= j ? M[(size_t)i * b + j] : M[(size_t)j * b + i]; };
  std::fill(theta, theta + b, 0.0);
  std::fill(C, C + (size_t)b * b, 0.0);
  // the scaling, and the scaled Cholesky factor column by column up to the first pivot below 1e-12
  int n = 0;
  for (int j = 0; j < b; j++) {
    const double g = G[(size_t)j * b + j];
    k.dscale[j] = g > 0.0 && std::isfinite(g) ? 1.0 / std::sqrt(g) : 0.0;
  }
  for (int j = 0; j < b; j++, n++) {
    if (!(k.dscale[j] > 0.0)) break;
    double s = G[(size_t)j * b + j] * k.dscale[j] * k.dscale[j];
    for (int q = 0; q < j; q++) {
      double v = low(G, j, q) * k.dscale[j] * k.dscale[q];
      for (int r = 0; r < q; r++) v -= k.L[j][r] * k.L[q][r];
      k.L[j][q] = v / k.L[q][q];
      s -= k.L[j][q] * k.L[j][q];
    }
    if (!(s >= 1e-12)) break;
    k.L[j][j] = std::sqrt(s);
  }
  if (used_out) *used_out = n;
  for (int j = n; j < b; j++) C[(size_t)j * b + j] = k.dscale[j];
  if (n == 0) return -1;
  // As <- L^-1 (D T D) L^-T
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) k.As[i][j] = low(T, i, j) * k.dscale[i] * k.dscale[j];
  for (int c = 0; c < n; c++)       // columns: L Y = As
    for (int i = 0; i < n; i++) {
      double s = k.As[i][c];
      for (int q = 0; q < i; q++) s -= k.L[i][q] * k.As[q][c];
      k.As[i][c] = s / k.L[i][i];
    }
  for (int r = 0; r < n; r++)       // rows: Y L^-T
    for (int j = 0; j < n; j++) {
      double s = k.As[r][j];
      for (int q = 0; q < j; q++) s -= k.As[r][q] * k.L[j][q];
      k.As[r][j] = s / k.L[j][j];
    }
  for (int i = 0; i < n; i++)
    for (int j = i + 1; j < n; j++) k.As[i][j] = k.As[j][i] = 0.5 * (k.As[i][j] + k.As[j][i]);
  jacobi_eig(n, k.As, k.Z, k.w);
  for (int i = 0; i < n; i++) k.idx[i] = i;
  std::stable_sort(k.idx, k.idx + n, [&](int x, int y) { return k.w[x] < k.w[y]; });
  for (int j = 0; j < n; j++) {
    theta[j] = k.w[k.idx[j]];
    for (int i = n - 1; i >= 0; i--) {   // L^T c = z
      double s = k.Z[i][k.idx[j]];
      for (int q = i + 1; q < n; q++) s -= k.L[q][i] * k.c[q];
      k.c[i] = s / k.L[i][i];
    }
    for (int i = 0; i < n; i++) C[(size_t)i * b + j] = k.dscale[i] * k.c[i];
  }
  return 0;
}

void modes_unpack(int b, const double *packed, double *G, double *T) {
  const int L = b * (b + 1) / 2;
  for (int i = 0; i < b; i++)
    for (int j = 0; j <= i; j++) {
      G[(size_t)i * b + j] = G[(size_t)j * b + i] = packed[i * (i + 1) / 2 + j];
      T[(size_t)i * b + j] = T[(size_t)j * b + i] = packed[L + i * (i + 1) / 2 + j];
    }
}

// ---------------------------------------------------------------------------
// the call
// ---------------------------------------------------------------------------
namespace {
struct Pinned {   // the read-backs and the block the host hands the update: pinned for the length of one call
  double *p = nullptr;
  explicit Pinned(size_t n) {
    HIP_CHECK(hipHostMalloc((void **)&p, sizeof(double) * n, hipHostMallocDefault));
    std::memset(p, 0, sizeof(double) * n);
  }
  ~Pinned() { if (p) (void)hipHostFree(p); }
  Pinned(const Pinned &) = delete;
  Pinned &operator=(const Pinned &) = delete;
};
}  // namespace

int Group::hessian_modes(const double *X, int ld, int anchor, int k, const ModesOptions &o, long long max_bytes, double *values,
                         double *residuals, double *vectors, double *energy, double *X_escape, ModesResult &out) {
  out = ModesResult();
  if (!values || !residuals || !vectors || !energy || (o.want_escape && !X_escape) || o.guard < 4 || o.max_iters < 1 ||
      o.max_tries < 1 || !(o.rel_tol >= 0) || !(o.shift >= 0) || !std::isfinite(o.shift)) {
    fprintf(stderr, "[dpgo_amd] ERROR: hessian_modes: bad options or missing output arrays.\n");
    return -1;
  }
  if (cov_begin(X, ld, anchor) != 0) return -1;
  const int dof = cov_dof(d_), N = P0_;
  const long long n = (long long)dof * N;
  if (k < 1 || k > MODES_MAX_K || k > n - dof || modes_block(k, o.guard) > MODES_MAX_B) {
    fprintf(stderr, "[dpgo_amd] ERROR: hessian_modes: k = %d with guard %d is outside 1 ... min(%d, n - dof = %lld) or its block is "
                    "wider than %d columns.\n", k, o.guard, MODES_MAX_K, n - dof, MODES_MAX_B);
    return -1;
  }
  ModesHooks hooks;
  hooks.hessian = [&](int arow) { launch_cov_hessian_at(arow); };
  hooks.trial = [&](int arow) {
    CertState &c = *cert_;
    cert_apply_M(c.V.p, c.SV.p);
    launch_polish_grad(lc(NodeMask{all_bits(), nullptr}), c.V.p, c.SV.p, arow, nullptr, -1, 2, c.partials.p);
  };
  return modes_loop(X, ld, anchor, k, o, max_bytes, hooks, values, residuals, vectors, energy, X_escape, out);
}

// Behind cov_begin: the analysis, the refusal, the point (X, M X, Lambda, g and F through the certificate's path), then the
// shift loop and the iteration.  hooks.hessian writes H at c.X into the factorisation's values; hooks.trial leaves F(c.V) in
// slot 2 of the certificate's partials; both are handed the anchor's own row, which exists only behind the analysis
// (own_row reads the maps cert_build_pattern fills).
int Group::modes_loop(const double *X, int ld, int anchor, int k, const ModesOptions &o, long long max_bytes, const ModesHooks &hooks,
                      double *values, double *residuals, double *vectors, double *energy, double *X_escape, ModesResult &out) {
  if (cov_analyse(out) != 0) return -1;
  CertState &c = *cert_;
  CovState &s = *cov_;
  const int arow = own_row(anchor);
  const int dof = cov_dof(d_), N = P0_, b = modes_block(k, o.guard), lb = b, nwg = modes_workgroups((long long)dof * N);
  const long long n = (long long)dof * N;
  const size_t nb = (size_t)n * lb;
  out.block = b;
  // the refusal: the numeric phase, one batch of the block solve, the two blocks, the partials with C and Theta and the gid map,
  // and polish's three vectors (g for the escape, the unshifted diagonal for the shift) where no polish has left them
  const long long solve = (long long)spd_msolve_bytes(s.F, b), blocks = 2ll * 8ll * n * lb,
                  small = 8ll * (modes_partials(n, b) + (long long)b * b + b) + 4ll * N, vectors3 = 3ll * 8ll * n;
  const int ready = hess_reserve(max_bytes, "hessian_modes",
                                 {s.numeric_part(), {solve, solve}, {blocks, blocks}, {small, small}, {vectors3, s.pol_g.p ? 0 : vectors3}},
                                 out);
  if (ready < 0) return -1;
  cert_prepare(X, ld, &out.stationarity);
  if (ready != 0) return 0;   // SKIPPED, with what the analysis predicts
  if (!s.pol_g.p)
    for (DevBuf<double> *buf : {&s.pol_g, &s.pol_sol, &s.pol_hdiag}) buf->alloc((size_t)std::max<long long>(n, 1));
  typedef std::chrono::steady_clock Clock;
  auto ms_since = [](Clock::time_point t) { return 1e3 * std::chrono::duration<double>(Clock::now() - t).count(); };
  const auto t_start = Clock::now();
  const NodeMask all{all_bits(), nullptr};
  const double *h = c.h_sums;
  DevBuf<double> V, W, part, Cdev;
  DevBuf<int> gid;
  V.alloc(nb, false);
  W.alloc(nb, false);
  part.alloc((size_t)modes_partials(n, b), false);
  Cdev.alloc((size_t)b * b + b, false);
  gid.upload(c.gid);
  const int L = b * (b + 1) / 2;
  Pinned pin((size_t)2 * L + 2 * b + (size_t)b * b + b);
  double *h_gram = pin.p, *h_sums = pin.p + 2 * L, *h_C = h_sums + 2 * b, *h_theta = h_C + (size_t)b * b;
  std::vector<double> G((size_t)b * b), T((size_t)b * b);
  std::fill(values, values + k, 0.0);
  std::fill(residuals, residuals + k, 0.0);
  std::fill(vectors, vectors + (size_t)k * n, 0.0);
  std::fill(energy, energy + (size_t)k * N, 0.0);

  // ---- g, F, H and hmax at X; the shift on polish.h's rule until the factorisation succeeds
  launch_polish_grad(lc(all), c.X.p, c.MX.p, arow, s.pol_g.p, 0, 1, c.partials.p);
  HIP_CHECK(hipStreamSynchronize(st_));
  auto t0 = Clock::now();
  double mu = o.shift > 0 ? o.shift : 0.0;
  hooks.hessian(arow);
  launch_polish_shift(lc(all), c.bptr.p, c.diag_pose.p, arow, mu, true, s.pol_hdiag.p, spd_numeric_values(s.F), 2, c.partials.p);
  launch_polish_reduce(st_, T_, 3, 1u << 2, c.partials.p, c.h_sums, sched_.flag());
  wait_flag(sched_.last_seq());
  const double F0 = h[1], hmax = std::isfinite(h[2]) ? h[2] : 0.0;
  out.F = out.F_escape = F0;
  out.hmax = hmax;
  if (o.want_escape) cert_download(c.X.p, X_escape, ld, d_);   // (X itself unless a lower point is found)
  bool factored = false;
  for (int t = 0; t < o.max_tries && !factored; t++) {
    if (t > 0) launch_polish_shift(lc(all), c.bptr.p, c.diag_pose.p, arow, mu, false, s.pol_hdiag.p, spd_numeric_values(s.F), 2, c.partials.p);
    const int rc = hess_refactor("hessian_modes", out);
    out.factorisations++;
    if (rc < 0) return -1;
    if (rc != 0) {
      out.shift_tries++;
      mu = std::max(10 * mu, 1e-3 * hmax);
      if (!(mu > 0)) break;   // (hmax = 0: nothing to shift by)
      continue;
    }
    factored = true;
  }
  out.factor_ms = ms_since(t0);
  out.mu = mu;
  out.outcome = MODES_STALLED;
  if (!factored) {
    out.total_ms = ms_since(t_start);
    return 0;
  }

  // ---- the iteration
  const int a0 = dof * arow;
  launch_modes_init(st_, n, b, lb, a0, dof, o.seed, gid.p, dof, V.p);
  std::vector<double> theta(b, 0.0), rnorm(b, 0.0), vnorm(b, 1.0);
  bool converged = false, have_pairs = false, stalled = false;
  for (int it = 1; it <= o.max_iters && !converged; it++) {
    t0 = Clock::now();
    HIP_CHECK(hipMemcpyAsync(W.p, V.p, sizeof(double) * nb, hipMemcpyDeviceToDevice, st_));
    if (spd_msolve_device(s.F, W.p, b, lb, st_) != 0) {
      fprintf(stderr, "[dpgo_amd] ERROR: hessian_modes: the solve failed on the device.\n");
      return -1;
    }
    out.solve_ms += ms_since(t0);
    t0 = Clock::now();
    launch_modes_gram(st_, n, b, lb, W.p, V.p, part.p);
    launch_modes_reduce_gram(st_, nwg, b, part.p, h_gram, sched_.flag());
    wait_flag(sched_.last_seq());
    out.gram_ms += ms_since(t0);
    out.iterations = it;
    t0 = Clock::now();
    modes_unpack(b, h_gram, G.data(), T.data());
    int used = 0;
    const int rr = modes_ritz(b, G.data(), T.data(), h_theta, h_C, &used);
    out.ritz_ms += ms_since(t0);
    if (rr != 0 || used < k) {   // STALLED, with the pairs of the iteration before (if any)
      stalled = true;
      break;
    }
    t0 = Clock::now();
    HIP_CHECK(hipMemcpyAsync(Cdev.p, h_C, sizeof(double) * ((size_t)b * b + b), hipMemcpyHostToDevice, st_));
    launch_modes_update(st_, n, b, lb, a0, dof, W.p, V.p, Cdev.p, Cdev.p + (size_t)b * b, part.p);
    launch_modes_reduce(st_, nwg, 2 * b, 2 * b, part.p, h_sums, sched_.flag());
    wait_flag(sched_.last_seq());
    out.update_ms += ms_since(t0);
    converged = true;
    for (int j = 0; j < b; j++) {
      theta[j] = h_theta[j];
      rnorm[j] = std::sqrt(h_sums[j]);
      vnorm[j] = std::sqrt(h_sums[b + j]);
      if (j < k && !(rnorm[j] <= o.rel_tol * hmax)) converged = false;
    }
    have_pairs = true;
  }
  if (have_pairs) out.outcome = converged ? MODES_CONVERGED : (stalled ? MODES_STALLED : MODES_MAX_ITERS);

  // ---- the pairs to the host: row j of `vectors` the unit vector v_j by global pose, where it lives, lambda_j = theta_j - mu
  std::vector<double> Vh(nb), v0own;
  if (have_pairs) {
    HIP_CHECK(hipMemcpyAsync(Vh.data(), V.p, sizeof(double) * nb, hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
    for (int j = 0; j < k; j++) {
      values[j] = theta[j] - mu;
      residuals[j] = rnorm[j];
      if (converged && values[j] < 0) out.negative++;
      double nn = 0;
      for (long long i = 0; i < n; i++) nn += Vh[(size_t)i * lb + j] * Vh[(size_t)i * lb + j];
      const double inv = nn > 0 ? 1.0 / std::sqrt(nn) : 0.0;
      for (int p = 0; p < N; p++) {
        const int g = c.gid[p];
        double e = 0;
        for (int a = 0; a < dof; a++) {
          const double v = Vh[((size_t)dof * p + a) * lb + j] * inv;
          vectors[(size_t)j * n + (size_t)dof * g + a] = v;
          e += v * v;
        }
        energy[(size_t)j * N + g] = e;
      }
    }
  }

  // ---- the escape along v_0
  if (o.want_escape && have_pairs && values[0] < 0) {
    std::vector<double> gh((size_t)n);
    HIP_CHECK(hipMemcpyAsync(gh.data(), s.pol_g.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
    double nn = 0, gv = 0, vinf = 0;
    for (long long i = 0; i < n; i++) nn += Vh[(size_t)i * lb] * Vh[(size_t)i * lb];
    const double inv = nn > 0 ? 1.0 / std::sqrt(nn) : 0.0;
    for (long long i = 0; i < n; i++) {
      const double v = Vh[(size_t)i * lb] * inv;
      gv += gh[i] * v;
      vinf = std::max(vinf, std::fabs(v));
    }
    const double sgn = gv > 0 ? -1.0 : 1.0;
    double alpha = vinf > 0 ? 0.5 / vinf : 0.0;
    for (int t = 0; t <= 30 && alpha > 0; t++, alpha *= 0.5) {
      // sol = -alpha s v_0: launch_polish_retract moves by -sol
      launch_modes_column(st_, n, lb, 0, -alpha * sgn * inv, V.p, s.pol_sol.p);
      launch_polish_retract(lc(all), c.X.p, s.pol_sol.p, s.pol_g.p, arow, c.V.p, 0, 1, c.partials.p);
      hooks.trial(arow);
      launch_polish_reduce(st_, T_, 3, 0u, c.partials.p, c.h_sums, sched_.flag());
      wait_flag(sched_.last_seq());
      const double F1 = h[2], pred = alpha * std::fabs(gv) + 0.5 * alpha * alpha * std::fabs(values[0]);
      if (F1 <= F0 - 0.1 * pred) {
        out.escaped = 1;
        out.escape_alpha = alpha;
        out.F_escape = F1;
        cert_download(c.V.p, X_escape, ld, d_);
        break;
      }
    }
  }
  out.total_ms = ms_since(t_start);
  return 0;
}

}  // namespace dpgo
