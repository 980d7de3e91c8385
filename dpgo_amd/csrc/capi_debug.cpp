// The test hooks of the C ABI (include/dpgo_amd.h): every dpgo_debug_* and dpgo_group_debug_* entry point.  Only tests/ and
// the tools call them; what a user of the library links against is in capi.cpp.  The hooks that take a CSR matrix read it
// with read_csr, and those that factor it do so through one SpdDebugSession.
#include "capi_util.h"

#include <algorithm>
#include <memory>
#include <string>
#include <utility>

#include "cert.h"
#include "comm.h"
#include "ml_rely.h"
#include "pairs_math.h"

// A CSR matrix handed over the C ABI, checked and copied into A: n > 0, no null array, ptr from 0 and monotone, every column
// in [0, n), and the ordering parameters of spd_factor (a hook without them leaves the defaults, which pass).
// false: malformed, A is not to be used.
static bool read_csr(int n, const int *ptr, const int *col, const double *val, dpgo::CsrMatrix &A, int leaf = 1, int collapse = 0,
                     int block = 1) {
  if (n <= 0 || !ptr || !col || !val || ptr[0] != 0 || leaf < 1 || block < 1 || collapse < 0 || n % block != 0) return false;
  for (int i = 0; i < n; i++)
    if (ptr[i + 1] < ptr[i]) return false;
  for (int e = 0; e < ptr[n]; e++)
    if (col[e] < 0 || col[e] >= n) return false;
  A.n = n;
  A.ptr.assign(ptr, ptr + n + 1);
  A.col.assign(col, col + ptr[n]);
  A.val.assign(val, val + ptr[n]);
  return true;
}

namespace {
bool spd_debug_device_numeric() {
  int ndev = 0;
  return !dpgo::settings().spd_host_factor && hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
}
// W / WT of F to the host: the host vectors where the numeric phase filled them, else the device copies
int spd_debug_fetch(const dpgo::SpdFactor &F, std::vector<double> &W, std::vector<double> &WT) {
  const int nt = F.nfronts;
  if (!F.dev_W) { W = F.W; WT = F.WT; return 0; }
  W.assign(F.w_off[nt], 0.0);
  WT.assign(F.wt_off[nt], 0.0);
  if (!W.empty() && hipMemcpy(W.data(), F.dev_W, sizeof(double) * W.size(), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (!WT.empty() && hipMemcpy(WT.data(), F.dev_WT, sizeof(double) * WT.size(), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return 0;
}

// One matrix, its factor and what the factor keeps on the device, for the length of a hook.  It decides where the numeric
// phase runs, factors, factors again from new values -- through the kept context on the device, from scratch on the host --
// and writes the verdict of numeric phase k to status[k stride] (0 factored, 1 not positive definite, -1 error), its pivot
// range to pivots[2k], pivots[2k + 1] and, where asked for, the failing front to fail_front[k].  (A factor does not release
// what it owns by itself: spd.h.)
struct SpdDebugSession {
  dpgo::CsrMatrix A;
  dpgo::SpdFactor F;
  const bool on_device;
  double *d_x = nullptr;   // the array a solve hook works in, n doubles times its columns
  int *const status;
  const int stride;
  double *const pivots;
  int *const fail_front;

  SpdDebugSession(dpgo::CsrMatrix &&A_, bool host, int *status_, double *pivots_, int stride_ = 1, int *fail_front_ = nullptr)
      : A(std::move(A_)), on_device(!host && spd_debug_device_numeric()), status(status_), stride(stride_), pivots(pivots_),
        fail_front(fail_front_) {
    F.quiet = true;
    for (int k = 0; k < 2; k++) {
      status[k * stride] = -1;
      if (fail_front) fail_front[k] = -1;
    }
    std::fill(pivots, pivots + 4, 0.0);
  }
  SpdDebugSession(const SpdDebugSession &) = delete;
  ~SpdDebugSession() {
    if (d_x) (void)hipFree(d_x);
    dpgo::spd_release_device(F);
    dpgo::spd_release_numeric(F);
  }

  // rc of spd_factor / spd_refactor / spd_refactor_device -> the verdict of numeric phase k, written and returned
  int record(int k, int rc) {
    const int s = rc == 0 ? 0 : (F.not_pd ? 1 : -1);
    status[k * stride] = s;
    if (fail_front) fail_front[k] = F.not_pd ? F.fail_front : -1;
    pivots[2 * k] = F.pivot_min;
    pivots[2 * k + 1] = F.pivot_max;
    return s;
  }
  // numeric phase 0.  keep: W / WT and the numeric context stay on the device (keep_device + keep_numeric)
  int factor(int leaf, int collapse, int block, bool keep) {
    F.keep_numeric = keep;
    const int s = record(0, dpgo::spd_factor(A, F, leaf, collapse, block, /*keep_device=*/keep));
    return keep && !F.numeric ? -1 : s;
  }
  // numeric phase k from new values of the same pattern: on the device through the kept context, the kernels again (also
  // behind a non-positive pivot: the context does not depend on the values); without one, spd_refactor redoes the
  // factorisation on the host.  k < 0: nothing is recorded and the rc of the numeric phase comes back
  int refactor(int k, const double *val) {
    int rc;
    if (F.numeric) {
      if (hipMemcpy(dpgo::spd_numeric_values(F), val, sizeof(double) * A.val.size(), hipMemcpyHostToDevice) != hipSuccess) return -1;
      rc = dpgo::spd_refactor_device(F);
    } else {
      A.val.assign(val, val + A.val.size());
      rc = dpgo::spd_refactor(A, F);
    }
    return k < 0 ? rc : record(k, rc);
  }
  // what vsolve and msolve do with a session: factor, solve into slots 0 and 1, factor refactor_val (if any), solve into
  // slot 2.  solve(j): slot j <- A^-1 rhs, 0 / -1; refuses(): the device solve on a factor that failed, true where it
  // returned its -1.  Returns 1 (ran on the device), 0 (on the host) or -1
  template <class Solve, class Refuses>
  int solve_course(int leaf, int collapse, int block, const double *refactor_val, Solve solve, Refuses refuses) {
    const int s = factor(leaf, collapse, block, on_device);
    if (s < 0) return -1;
    if (s == 0 && (solve(0) != 0 || solve(1) != 0)) return -1;
    if (s != 0 && on_device && !refuses()) return -1;   // (a failed factorisation solves nothing)
    if (refactor_val) {
      const int s2 = refactor(1, refactor_val);
      if (s2 < 0 || (s2 == 0 && solve(2) != 0)) return -1;
    }
    return on_device ? 1 : 0;
  }
};
}  // namespace

// ---- assembled operators of one node ----
static int ref_row(int d, int n0, int n1, int p, int slot) {
  if (p < n0) return slot == 0 ? p : n0 + p * d + slot - 1;
  const int k = p - n0;
  return slot == 0 ? (d + 1) * n0 + k : (d + 1) * n0 + n1 + k * d + slot - 1;
}

extern "C" {

int dpgo_debug_node_matrix(const dpgo_graph_t *g, int node, const dpgo_options_t *opt, const char *name, int *rows,
                           int *cols, double *vals) {
  dpgo::DataInfo info;
  if (node_info(g, node, info) != 0) return -1;
  dpgo::NodeOperators ops;
  const bool trivial = opt->loss == 0;
  if (dpgo::assemble_node(info, opt->regularizer, trivial, ops) != 0) return -1;
  const int d = info.d, B = d + 1, n0 = info.n[0], n1 = info.n[1];
  const std::string nm(name);
  int cnt = 0;
  auto emit = [&](int p, int q, const double *blk) {
    for (int r = 0; r < B; r++)
      for (int c = 0; c < B; c++) {
        if (blk[r * B + c] == 0.0) continue;
        if (rows) { rows[cnt] = ref_row(d, n0, n1, p, r); cols[cnt] = ref_row(d, n0, n1, q, c); vals[cnt] = blk[r * B + c]; }
        cnt++;
      }
  };
  if (nm == "D") {
    for (int p = 0; p < n0; p++) emit(p, p, &ops.D[(size_t)p * B * B]);
    return cnt;
  }
  const dpgo::BsrMatrix *M = nm == "G" ? &ops.G : nm == "S" ? &ops.S : nm == "P" ? &ops.P : nm == "P0" ? &ops.P0
                                                                                    : nm == "Q" ? &ops.Q : nullptr;
  if (!M || M->B == 0) return -1;
  for (int p = 0; p < M->nrows; p++)
    for (int k = M->ptr[p]; k < M->ptr[p + 1]; k++) emit(p, M->col[k], &M->val[(size_t)k * B * B]);
  return cnt;
}

int dpgo_debug_node_proximal(const dpgo_graph_t *g, int node, const dpgo_options_t *opt, double *T, double *N,
                             double *V) {
  dpgo::DataInfo info;
  if (node_info(g, node, info) != 0) return -1;
  dpgo::NodeOperators ops;
  if (dpgo::assemble_node(info, opt->regularizer, opt->loss == 0, ops) != 0) return -1;
  std::copy(ops.Tinv.begin(), ops.Tinv.end(), T);
  std::copy(ops.N.begin(), ops.N.end(), N);
  std::copy(ops.V.begin(), ops.V.end(), V);
  return 0;
}

// ---- the host factor and solve of a given matrix ----
int dpgo_debug_spd_solve(int n, const int *ptr, const int *col, const double *val, double *X, int ncols, int leaf) {
  return guarded([&] {
    dpgo::CsrMatrix A;
    dpgo::SpdFactor F;
    if (!read_csr(n, ptr, col, val, A, leaf) || dpgo::spd_factor(A, F, leaf) != 0) return -1;
    dpgo::spd_solve_host(F, X, ncols);
    return 0;
  });
}

int dpgo_debug_spd_stats(int n, const int *ptr, const int *col, const double *val, int leaf, long *nnz, int *levels,
                         int *max_front) {
  return guarded([&] {
    dpgo::CsrMatrix A;
    dpgo::SpdFactor F;
    if (!read_csr(n, ptr, col, val, A, leaf) || dpgo::spd_factor(A, F, leaf) != 0) return -1;
    if (!dpgo::settings().spd_dump_fronts.empty()) {   // analysis hook: w u height depth per front
      if (FILE *fp = fopen(dpgo::settings().spd_dump_fronts.c_str(), "w")) {
        for (int f = 0; f < F.nfronts; f++) fprintf(fp, "%d %d %d %d\n", F.w[f], F.u[f], F.height[f], F.depth[f]);
        fclose(fp);
      }
    }
    *nnz = (long)F.nnz();
    *levels = (int)F.by_height.size();
    *max_front = F.max_front;
    return 0;
  });
}

}  // extern "C"

// ---- test hook: the factor itself, front by front ----
struct dpgo_spd_debug {
  int status[2], fail_front[2];   // [0] the factorisation, [1] the one through the kept context
  double pivots[4];
  SpdDebugSession S;
  bool has_second = false, factor_only = false;
  std::vector<int> height;
  std::vector<double> W, WT, W2, WT2;
  explicit dpgo_spd_debug(dpgo::CsrMatrix &&A) : S(std::move(A), /*host=*/false, status, pivots, 1, fail_front) {}
};

// ---- test hook: selected inversion, front by front ----
struct dpgo_spd_selinv_debug {
  int status[4] = {-1, -1, -1, -1};   // factorisation, inversion, and the two behind refactor_val
  double pivots[4];
  SpdDebugSession S;
  std::vector<int> depth;
  std::vector<double> sigma, sigma_again, sigma2, W_before, W_after;
  dpgo_spd_selinv_debug(dpgo::CsrMatrix &&A, bool host) : S(std::move(A), host, status, pivots, 2) {}
};

extern "C" {

int dpgo_debug_spd_factor(int n, const int *ptr, const int *col, const double *val, const double *refactor_val, int leaf,
                          int collapse, int block, int factor_only, dpgo_spd_debug_t **out) {
  if (!out) return -1;
  *out = nullptr;
  return guarded([&] {
    dpgo::CsrMatrix A;
    if (!read_csr(n, ptr, col, val, A, leaf, collapse, block)) return -1;
    std::unique_ptr<dpgo_spd_debug> h(new dpgo_spd_debug(std::move(A)));
    SpdDebugSession &S = h->S;
    dpgo::SpdFactor &F = S.F;
    h->factor_only = factor_only != 0;
    h->has_second = refactor_val != nullptr;
    if (h->factor_only && S.on_device) {
      // the certificate's route (cert.cpp): analysis, context, values written on the device, numeric phase from them
      F.factor_only = true;
      if (dpgo::spd_symbolic(S.A, F, leaf, collapse, block) != 0 || dpgo::spd_prepare_device(S.A, F) != 0) return -1;
      if (S.refactor(0, val) < 0 || (refactor_val && S.refactor(1, refactor_val) < 0)) return -1;
    } else {
      // (keep: Group::factor_tt for a Dynamic rescale)
      const int s = S.factor(leaf, collapse, block, /*keep=*/refactor_val != nullptr && S.on_device);
      if (s < 0 || (s == 0 && !h->factor_only && spd_debug_fetch(F, h->W, h->WT) != 0)) return -1;
      if (refactor_val) {
        const int s2 = S.refactor(1, refactor_val);
        if (s2 < 0 || (s2 == 0 && !h->factor_only && spd_debug_fetch(F, h->W2, h->WT2) != 0)) return -1;
      }
    }
    h->height.assign(F.nfronts, 0);
    for (int f = 0; f < F.nfronts; f++)
      if (F.parent[f] >= 0) h->height[F.parent[f]] = std::max(h->height[F.parent[f]], h->height[f] + 1);
    *out = h.release();
    return 0;
  });
}

int dpgo_debug_spd_factor_get(const dpgo_spd_debug_t *h, long long *sizes, int *status, double *pivots, int *fronts,
                              long long *offsets, int *piv_idx, int *upd_idx, double *W, double *WT, double *W2, double *WT2) {
  if (!h) return -1;
  const dpgo::SpdFactor &F = h->S.F;
  const int nt = F.nfronts;
  if (sizes) {
    sizes[0] = nt; sizes[1] = F.upd_ptr[nt]; sizes[2] = F.w_off[nt]; sizes[3] = F.wt_off[nt];
    sizes[4] = (long long)h->W.size(); sizes[5] = (long long)h->W2.size(); sizes[6] = h->has_second; sizes[7] = h->S.on_device;
  }
  if (status) { status[0] = h->status[0]; status[1] = h->fail_front[0]; status[2] = h->status[1]; status[3] = h->fail_front[1]; }
  if (pivots) std::copy(h->pivots, h->pivots + 4, pivots);
  for (int f = 0; f < nt; f++) {
    if (fronts) {
      int *q = fronts + 6 * f;
      q[0] = F.w[f]; q[1] = F.u[f]; q[2] = F.parent[f]; q[3] = h->height[f]; q[4] = F.ldw[f]; q[5] = F.ldm[f];
    }
    if (offsets) { offsets[2 * f] = F.w_off[f]; offsets[2 * f + 1] = F.wt_off[f]; }
  }
  if (piv_idx) std::copy(F.piv_idx.begin(), F.piv_idx.end(), piv_idx);
  if (upd_idx) std::copy(F.upd_idx.begin(), F.upd_idx.end(), upd_idx);
  if (W) std::copy(h->W.begin(), h->W.end(), W);
  if (WT) std::copy(h->WT.begin(), h->WT.end(), WT);
  if (W2) std::copy(h->W2.begin(), h->W2.end(), W2);
  if (WT2) std::copy(h->WT2.begin(), h->WT2.end(), WT2);
  return 0;
}

void dpgo_debug_spd_factor_free(dpgo_spd_debug_t *h) { delete h; }

int dpgo_debug_spd_selinv(int n, const int *ptr, const int *col, const double *val, const double *refactor_val, int leaf,
                          int collapse, int block, int host, dpgo_spd_selinv_debug_t **out) {
  if (!out) return -1;
  *out = nullptr;
  return guarded([&] {
    dpgo::CsrMatrix A;
    if (!read_csr(n, ptr, col, val, A, leaf, collapse, block)) return -1;
    std::unique_ptr<dpgo_spd_selinv_debug> h(new dpgo_spd_selinv_debug(std::move(A), host != 0));
    SpdDebugSession &S = h->S;
    dpgo::SpdFactor &F = S.F;
    std::vector<double> WT;
    // the blocks the device holds, to the host
    auto fetch_sigma = [&](std::vector<double> &Sig) -> int {
      Sig.assign(dpgo::spd_selinv_offsets(F).back(), 0.0);
      if (hipDeviceSynchronize() != hipSuccess) return -1;
      if (!Sig.empty() && hipMemcpy(Sig.data(), dpgo::spd_selinv_values(F), sizeof(double) * Sig.size(), hipMemcpyDeviceToHost) != hipSuccess) return -1;
      return 0;
    };
    // (with a device and host != 0 the numeric phase still runs where spd_factor puts it; W comes to the host)
    const int s = S.factor(leaf, collapse, block, /*keep=*/S.on_device);
    if (s < 0) return -1;
    if (S.on_device) {
      if (s == 0 && spd_debug_fetch(F, h->W_before, WT) != 0) return -1;
      const int si = dpgo::spd_selinv_device(F);
      h->status[1] = si == 0 ? 0 : (F.not_pd ? 1 : -1);
      if (h->status[1] < 0) return -1;
      if (si == 0) {
        if (fetch_sigma(h->sigma) != 0 || dpgo::spd_selinv_device(F) != 0 || fetch_sigma(h->sigma_again) != 0) return -1;
        // the same values through the kept context, behind the inversion
        if (S.refactor(-1, val) != 0 || spd_debug_fetch(F, h->W_after, WT) != 0) return -1;
      }
      if (refactor_val) {
        if (S.refactor(1, refactor_val) < 0) return -1;
        const int si2 = dpgo::spd_selinv_device(F);
        h->status[3] = si2 == 0 ? 0 : (F.not_pd ? 1 : -1);
        if (h->status[3] < 0) return -1;
        if (si2 == 0 && fetch_sigma(h->sigma2) != 0) return -1;
      }
    } else {
      h->status[1] = s;
      if (s == 0) {
        h->W_before = F.W;
        if (dpgo::spd_selinv_host(F, F.W.data(), h->sigma) != 0 || dpgo::spd_selinv_host(F, F.W.data(), h->sigma_again) != 0) return -1;
        h->W_after = F.W;
      }
      if (refactor_val) {
        const int s2 = S.refactor(1, refactor_val);
        if (s2 < 0) return -1;
        h->status[3] = s2;
        if (s2 == 0 && dpgo::spd_selinv_host(F, F.W.data(), h->sigma2) != 0) return -1;
      }
    }
    h->depth.assign(F.nfronts, 0);
    for (int f = F.nfronts - 1; f >= 0; f--)
      if (F.parent[f] >= 0) h->depth[f] = h->depth[F.parent[f]] + 1;
    *out = h.release();
    return 0;
  });
}

int dpgo_debug_spd_selinv_get(const dpgo_spd_selinv_debug_t *h, long long *sizes, int *status, double *pivots, int *fronts,
                              int *piv_idx, int *upd_idx, double *sigma, double *sigma_again, double *sigma2,
                              double *W_before, double *W_after) {
  if (!h) return -1;
  const dpgo::SpdFactor &F = h->S.F;
  const int nt = F.nfronts;
  if (sizes) {
    sizes[0] = nt; sizes[1] = F.upd_ptr[nt]; sizes[2] = dpgo::spd_selinv_offsets(F).back();
    sizes[3] = (long long)h->sigma.size(); sizes[4] = (long long)h->sigma_again.size(); sizes[5] = (long long)h->sigma2.size();
    sizes[6] = (long long)std::min(h->W_before.size(), h->W_after.size()); sizes[7] = h->S.on_device;
  }
  if (status) std::copy(h->status, h->status + 4, status);
  if (pivots) std::copy(h->pivots, h->pivots + 4, pivots);
  if (fronts)
    for (int f = 0; f < nt; f++) {
      int *q = fronts + 4 * f;
      q[0] = F.w[f]; q[1] = F.u[f]; q[2] = F.parent[f]; q[3] = h->depth[f];
    }
  if (piv_idx) std::copy(F.piv_idx.begin(), F.piv_idx.end(), piv_idx);
  if (upd_idx) std::copy(F.upd_idx.begin(), F.upd_idx.end(), upd_idx);
  if (sigma) std::copy(h->sigma.begin(), h->sigma.end(), sigma);
  if (sigma_again) std::copy(h->sigma_again.begin(), h->sigma_again.end(), sigma_again);
  if (sigma2) std::copy(h->sigma2.begin(), h->sigma2.end(), sigma2);
  if (W_before) std::copy(h->W_before.begin(), h->W_before.end(), W_before);
  if (W_after) std::copy(h->W_after.begin(), h->W_after.end(), W_after);
  return 0;
}

void dpgo_debug_spd_selinv_free(dpgo_spd_selinv_debug_t *h) { delete h; }

// ---- test hook: the device solve for one plain vector (spd.h: spd_vsolve_*) ----
int dpgo_debug_spd_vsolve_chunk(int chunk) { return dpgo::spd_vsolve_chunk(chunk); }

int dpgo_debug_spd_vsolve(int n, const int *ptr, const int *col, const double *val, const double *refactor_val, int leaf,
                          int collapse, int block, int host, const double *rhs, double *out, int *status, double *pivots) {
  if (!rhs || !out || !status || !pivots) return -1;
  return guarded([&] {
    dpgo::CsrMatrix A;
    if (!read_csr(n, ptr, col, val, A, leaf, collapse, block)) return -1;
    SpdDebugSession S(std::move(A), host != 0, status, pivots);
    dpgo::SpdFactor &F = S.F;
    const size_t nb = sizeof(double) * (size_t)n;
    if (S.on_device && hipMalloc((void **)&S.d_x, nb) != hipSuccess) return -1;
    // out + j n <- A^-1 rhs, through spd_vsolve_device or spd_solve_host
    auto solve = [&](int j) -> int {
      double *x = out + (size_t)j * n;
      if (!S.on_device) {
        std::copy(rhs, rhs + n, x);
        dpgo::spd_solve_host(F, x, 1);
        return 0;
      }
      if (hipMemcpy(S.d_x, rhs, nb, hipMemcpyHostToDevice) != hipSuccess) return -1;
      if (dpgo::spd_vsolve_device(F, S.d_x) != 0 || hipDeviceSynchronize() != hipSuccess) return -1;
      return hipMemcpy(x, S.d_x, nb, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
    };
    return S.solve_course(leaf, collapse, block, refactor_val, solve, [&] { return dpgo::spd_vsolve_device(F, S.d_x) == -1; });
  });
}

// ---- test hook: the device solve for a block of plain vectors (spd.h: spd_msolve_*) ----
int dpgo_debug_spd_msolve(int n, const int *ptr, const int *col, const double *val, const double *refactor_val, int leaf,
                          int collapse, int block, int host, int chunk, const double *rhs, int k, int ldx, double *out,
                          int *status, double *pivots) {
  if (!rhs || !out || !status || !pivots || k < 1 || ldx < k) return -1;
  return guarded([&] {
    dpgo::CsrMatrix A;
    if (!read_csr(n, ptr, col, val, A, leaf, collapse, block)) return -1;
    SpdDebugSession S(std::move(A), host != 0, status, pivots);
    dpgo::SpdFactor &F = S.F;
    struct ChunkRestore {   // the caller's chunk is back on every way out
      int before = 0;
      bool set = false;
      ~ChunkRestore() { if (set) dpgo::spd_msolve_chunk(before); }
    } restore;
    const size_t cnt = (size_t)n * ldx, nb = sizeof(double) * cnt;
    if (S.on_device) {
      if (chunk > 0) { restore.before = dpgo::spd_msolve_chunk(chunk); restore.set = true; }
      if (hipMalloc((void **)&S.d_x, nb) != hipSuccess) return -1;
    }
    // part j of out <- A^-1 rhs.  On the device the solve is handed the n x ldx array the caller filled, with rhs in its
    // first k columns; on the host spd_solve_host works on n x k and only those columns of out are written
    auto solve = [&](int j) -> int {
      if (!S.on_device) {
        std::vector<double> X(rhs, rhs + (size_t)n * k);
        dpgo::spd_solve_host(F, X.data(), k);
        for (int i = 0; i < n; i++) std::copy(X.begin() + (size_t)i * k, X.begin() + (size_t)(i + 1) * k, out + j * cnt + (size_t)i * ldx);
        return 0;
      }
      std::vector<double> X(out + j * cnt, out + (j + 1) * cnt);
      for (int i = 0; i < n; i++) std::copy(rhs + (size_t)i * k, rhs + (size_t)(i + 1) * k, X.begin() + (size_t)i * ldx);
      if (hipMemcpy(S.d_x, X.data(), nb, hipMemcpyHostToDevice) != hipSuccess) return -1;
      if (dpgo::spd_msolve_device(F, S.d_x, k, ldx) != 0 || hipDeviceSynchronize() != hipSuccess) return -1;
      return hipMemcpy(out + j * cnt, S.d_x, nb, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
    };
    return S.solve_course(leaf, collapse, block, refactor_val, solve,
                          [&] { return dpgo::spd_msolve_device(F, S.d_x, k, ldx) == -1; });
  });
}

}  // extern "C"

// ---- test hook: the device solve (spd_solve.cpp) on a given matrix ----
using dpgo::DeviceError;   // (what HIP_CHECK throws)
struct dpgo_spd_solver_debug {
  dpgo::SpdSolverDev S;
  int n = 0, d = 0, dof = 0, nnodes = 1;
  size_t nval = 0, len = 0;   // stored entries of A; doubles of a record array
  std::vector<int> height;
  hipStream_t st = nullptr;
  dpgo::DevBuf<double> in, out;
  dpgo::DevBuf<dpgo::NodeBits> word;
  ~dpgo_spd_solver_debug() { if (st) (void)hipStreamDestroy(st); }
};

extern "C" {

int dpgo_debug_spd_solver_create(int n, const int *ptr, const int *col, const double *val, int leaf, int collapse, int block,
                                 int d, int dof, const int *node_of_unknown, int keep_numeric, dpgo_spd_solver_debug_t **out) {
  if (!out) return -1;
  *out = nullptr;
  if (!ptr || !col || !val || !node_of_unknown || n <= 0 || (d != 2 && d != 3) || (dof != 1 && dof != d)) return -1;
  for (int i = 0; i < n; i++)
    if (node_of_unknown[i] < 0 || node_of_unknown[i] >= dpgo::MAX_LOCAL_NODES) return -1;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return -2;   // the solve has no host form
  const dpgo::Settings &s = dpgo::settings();
  if (keep_numeric && (!s.spd_device_panels || s.spd_host_factor)) return -1;   // (Group::refactor_tt keeps the context under the same condition)
  return guarded([&] {
    dpgo::CsrMatrix A;
    if (!read_csr(n, ptr, col, val, A, leaf, collapse, block)) return -1;
    std::unique_ptr<dpgo_spd_solver_debug> h(new dpgo_spd_solver_debug());
    h->n = n; h->d = d; h->dof = dof; h->nval = A.val.size();
    h->len = (size_t)((n + dof - 1) / dof) * (d + 1) * d;   // (a last record may hold fewer than dof unknowns)
    std::vector<int> node(node_of_unknown, node_of_unknown + n);
    for (int a : node) h->nnodes = std::max(h->nnodes, a + 1);
    dpgo::SpdFactor &F = h->S.F;
    F.keep_numeric = keep_numeric != 0;
    if (dpgo::spd_factor(A, F, leaf, collapse, block, s.spd_device_panels) != 0) return -1;
    h->height.assign(F.nfronts, 0);
    for (int f = 0; f < F.nfronts; f++)
      if (F.parent[f] >= 0) h->height[F.parent[f]] = std::max(h->height[F.parent[f]], h->height[f] + 1);
    h->S.upload(dof, d, node);
    HIP_CHECK(hipStreamCreate(&h->st));
    h->in.alloc(h->len);
    h->out.alloc(h->len);
    h->word.alloc(1);
    *out = h.release();
    return 0;
  });
}

int dpgo_debug_spd_solver_plan(const dpgo_spd_solver_debug_t *h, long long *sizes, int *flags, int *levels, int *node_counts,
                               int *fronts, int *piv_idx, int *upd_idx) {
  if (!h) return -1;
  const dpgo::SpdFactor &F = h->S.F;
  const dpgo::SpdPlanInfo I = h->S.plan_info();
  const int nt = F.nfronts, nn = h->nnodes;
  if (sizes) {
    sizes[0] = nt; sizes[1] = F.upd_ptr[nt]; sizes[2] = (long long)I.fwd.size(); sizes[3] = (long long)I.bwd.size();
    sizes[4] = nn; sizes[5] = h->n; sizes[6] = (long long)h->len; sizes[7] = (long long)h->nval;
  }
  if (flags) {
    flags[0] = I.fused_root; flags[1] = I.root_sym; flags[2] = I.root.rows; flags[3] = I.root_fine_rows;
    flags[4] = I.root_fine_below; flags[5] = I.stream_once; flags[6] = h->dof; flags[7] = h->d;
  }
  std::vector<const dpgo::SpdPlanInfo::Level *> all;
  for (const auto &v : I.fwd) all.push_back(&v);
  for (const auto &v : I.bwd) all.push_back(&v);
  all.push_back(&I.root); all.push_back(&I.root_fine); all.push_back(&I.root_rows);
  for (size_t l = 0; l < all.size(); l++) {
    const dpgo::SpdPlanInfo::Level &v = *all[l];
    if (levels) { levels[3 * l] = v.rows; levels[3 * l + 1] = v.nwide; levels[3 * l + 2] = v.nnarrow; }
    if (node_counts)
      for (int a = 0; a < nn; a++) {   // (a level nobody built -- no fused root, no finer class -- has no nodes: zeros)
        node_counts[(l * nn + a) * 2] = a < (int)v.wcount.size() ? v.wcount[a] : 0;
        node_counts[(l * nn + a) * 2 + 1] = a < (int)v.ncount.size() ? v.ncount[a] : 0;
      }
  }
  if (fronts)
    for (int f = 0; f < nt; f++) { fronts[4 * f] = F.w[f]; fronts[4 * f + 1] = F.u[f]; fronts[4 * f + 2] = F.parent[f]; fronts[4 * f + 3] = h->height[f]; }
  if (piv_idx) std::copy(F.piv_idx.begin(), F.piv_idx.end(), piv_idx);
  if (upd_idx) std::copy(F.upd_idx.begin(), F.upd_idx.end(), upd_idx);
  return 0;
}

int dpgo_debug_spd_solver_fine_root(const dpgo_spd_solver_debug_t *h, unsigned long long nodes) {
  if (!h) return -1;
  return h->S.fine_root_for(nodes) ? 1 : 0;
}

int dpgo_debug_spd_solver_run(dpgo_spd_solver_debug_t *h, unsigned long long mask_v, const unsigned long long *mask_word,
                              const unsigned long long *class_of, double scale, int in_place, const double *in, double *out) {
  if (!h || !in || !out || (scale != 1.0 && scale != -1.0)) return -1;
  return guarded([&] {
    // the out array first: what the solve leaves alone is what the caller put there (in place: the in array is both)
    HIP_CHECK(hipMemcpy(h->in.p, in, sizeof(double) * h->len, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(h->out.p, out, sizeof(double) * h->len, hipMemcpyHostToDevice));
    dpgo::NodeMask mask{mask_v, nullptr};
    if (mask_word) {
      HIP_CHECK(hipMemcpy(h->word.p, mask_word, sizeof(dpgo::NodeBits), hipMemcpyHostToDevice));
      mask.p = h->word.p;
    }
    const dpgo::NodeBits cls = class_of ? *class_of : 0;
    double *res = in_place ? h->in.p : h->out.p;
    try {
      dpgo::spd_run(h->d, h->st, h->S, mask, h->in.p, res, scale, class_of ? &cls : nullptr);
    } catch (const dpgo::DeviceError &) {
      return -2;   // spd_run's own refusal (in == out with fused roots); nothing was launched
    }
    HIP_CHECK(hipStreamSynchronize(h->st));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpy(out, res, sizeof(double) * h->len, hipMemcpyDeviceToHost));
    return 0;
  });
}

int dpgo_debug_spd_solver_refactor(dpgo_spd_solver_debug_t *h, const double *val) {
  if (!h || !val) return -1;
  return guarded([&] {
    dpgo::SpdFactor &F = h->S.F;
    double *dst = dpgo::spd_numeric_values(F);
    if (!dst) return -1;   // (not created with keep_numeric)
    // what Group::rescale_device does behind k_rescale_apply: the new values are on the device, the numeric phase and the
    // panels follow on the same stream
    HIP_CHECK(hipMemcpyAsync(dst, val, sizeof(double) * h->nval, hipMemcpyHostToDevice, h->st));
    if (dpgo::spd_refactor_device(F, (void *)h->st, true) != 0) return -1;
    if (h->S.repack(h->st) != 0) return -1;
    if (dpgo::spd_refactor_finish(F, true) != 0) return F.not_pd ? 1 : -1;
    HIP_CHECK(hipStreamSynchronize(h->st));
    return 0;
  });
}

void dpgo_debug_spd_solver_free(dpgo_spd_solver_debug_t *h) { delete h; }

int dpgo_debug_spd_panel_pack(int rows, int count, int len, int pairs, long long mat_off, const double *src, int src_ld,
                              double *panel, long long cap, long long *info) {
  if ((rows != 64 && rows != 16 && rows != 8) || count < 1 || count > rows || len < 1 || mat_off < 0 || !info) return -1;
  const dpgo::SpdItem it = dpgo::spd_panel_item(rows, count, pairs != 0, mat_off);
  info[0] = it.ld; info[1] = it.pair_kq; info[2] = it.mat_off; info[3] = dpgo::spd_panel_doubles(it, len);
  if (!panel) return 0;
  if (!src || src_ld < count || cap < mat_off + info[3]) return -1;
  dpgo::spd_pack_panel_host(it, dpgo::PanelSrc{0, src_ld, len}, src, panel);
  return 0;
}

// ---- the group's hooks (group.h: debug_*; debug_inter.cpp, debug_cert.cpp) ----
int dpgo_group_debug_apply(dpgo_group_t *h, int local, const char *op, const double *in, int ld_in, double *out,
                           int ld_out) {
  return guarded([&] { return h->grp->debug_apply(local, op, in, ld_in, out, ld_out); });
}

int dpgo_group_debug_inter_update(dpgo_group_t *h, const dpgo_inter_update_debug_t *q) {
  if (!h || !q) return -1;
  return guarded([&] {
    dpgo::Group::InterUpdateDebug a;
    a.local = q->local; a.whole = q->whole; a.quad = q->quad; a.with_Df = q->with_Df; a.nrecv = q->nrecv;
    a.Z = q->Z; a.Zprev = q->Zprev; a.DfE_old = q->DfE_old; a.GX = q->GX; a.X = q->X; a.Znbr = q->Znbr; a.recv = q->recv; a.nsrc = q->nsrc;
    a.DfE = q->DfE; a.g = q->g; a.w = q->w; a.sums = q->sums; a.Df = q->Df; a.Z_after = q->Z_after; a.Znbr_after = q->Znbr_after;
    return h->grp->debug_inter_update(a);
  });
}

int dpgo_group_debug_inter_iterate(dpgo_group_t *h, const dpgo_inter_iterate_debug_t *q) {
  if (!h || !q) return -1;
  return guarded([&] {
    dpgo::Group::InterIterateDebug a;
    a.local = q->local; a.whole = q->whole; a.fused = q->fused; a.prox = q->prox; a.gamma_dev = q->gamma_dev;
    a.Zc = q->Zc; a.Zp = q->Zp; a.GXc = q->GXc; a.GXp = q->GXp; a.Xref = q->Xref; a.gamma = q->gamma;
    a.Y = q->Y; a.g = q->g; a.Df = q->Df; a.Xout = q->Xout; a.Xref_after = q->Xref_after; a.sums = q->sums;
    return h->grp->debug_inter_iterate(a);
  });
}

int dpgo_group_debug_cost(dpgo_group_t *h, int local, int whole, int eform, const double *Z, double *sums) {
  if (!h) return -1;
  return guarded([&] { return h->grp->debug_cost(local, whole, eform, Z, sums); });
}

int dpgo_group_debug_edge_offsets(const dpgo_group_t *h, int *edge_offsets) {
  if (!h || !edge_offsets) return -1;
  const std::vector<int> &o = h->grp->debug_edge_offsets();
  for (size_t k = 0; k < o.size(); k++) edge_offsets[k] = o[k];
  return 0;
}

int dpgo_group_debug_rescale(dpgo_group_t *h, const double *w, const double *scale, const int *count, int max_rescale_count,
                             const int *nodes, int n, int *flags, double *host_flags, double *scale_out, int *count_out) {
  if (!h) return -1;
  return guarded([&] {
    return h->grp->debug_rescale(w, scale, count, max_rescale_count, nodes, n, flags, host_flags, scale_out, count_out);
  });
}

int dpgo_group_debug_cert_gram(dpgo_group_t *h, const double *X, const double *V, const double *W, const double *P,
                               const double *SV, const double *SP, const double *MW, int ld, double *sums, double *SW) {
  if (!h || !h->grp || !X) return -1;
  return guarded([&] { return h->grp->debug_cert_gram(X, V, W, P, SV, SP, MW, ld, sums, SW); });
}

int dpgo_group_debug_cert_update(dpgo_group_t *h, const dpgo_cert_update_debug_t *q) {
  if (!h || !h->grp || !q) return -1;
  return guarded([&] {
    dpgo::Group::CertUpdateDebug a;
    a.C = q->C; a.theta = q->theta; a.V = q->V; a.W = q->W; a.P = q->P; a.SV = q->SV; a.SW = q->SW; a.SP = q->SP;
    a.ld = q->ld; a.precondition = q->precondition; a.nbr_fill = q->nbr_fill;
    a.out[0] = q->V_out; a.out[1] = q->W_out; a.out[2] = q->P_out; a.out[3] = q->SV_out; a.out[4] = q->SW_out; a.out[5] = q->SP_out;
    a.sums = q->sums; a.nbr = q->nbr;
    return h->grp->debug_cert_update(a);
  });
}

int dpgo_group_debug_cert_nbr_rows(const dpgo_group_t *h) { return h && h->grp ? h->grp->debug_cert_nbr_rows() : -1; }

int dpgo_group_debug_cert_precon(dpgo_group_t *h, double *T) {
  if (!h || !h->grp || !T) return -1;
  return guarded([&] { return h->grp->debug_cert_precon(T); });
}

int dpgo_group_debug_cert_trace(dpgo_group_t *h, int on) {
  if (!h || !h->grp) return -1;
  h->grp->debug_cert_trace(on != 0);
  return 0;
}

int dpgo_group_debug_cert_trace_get(const dpgo_group_t *h, double *records, long long cap, int *record_len, long long *count) {
  if (!h || !h->grp || !record_len || !count) return -1;
  const std::vector<double> &t = h->grp->debug_cert_trace_records();
  *record_len = h->grp->cert_trace_len();
  *count = (long long)t.size() / *record_len;
  if (!records) return 0;   // (the sizes alone)
  if (cap < (long long)t.size()) return -1;
  std::copy(t.begin(), t.end(), records);
  return 0;
}

int dpgo_group_debug_seg_layout(dpgo_group_t *h, int *nseg_all, int *own_ptr, int *nbr_ptr) {
  if (!h) return -1;
  return guarded([&] { return h->grp->debug_seg_layout(nseg_all, own_ptr, nbr_ptr); });
}

int dpgo_group_debug_stpcg(dpgo_group_t *h, const int *locals, int n, const double *in, int ld_in, const double *Delta,
                           int device_start, double fill, double *out, int ld_out, double *scalars) {
  if (!h || !locals || n <= 0) return -1;
  return guarded([&] {
    return h->grp->debug_stpcg(std::vector<int>(locals, locals + n), in, ld_in, Delta, device_start != 0, fill, out, ld_out, scalars);
  });
}

int dpgo_group_debug_cg_scalars(dpgo_group_t *h, const dpgo_cg_debug_launch_t *script, int n, double *records,
                                unsigned long long *masks, double *cg_summary, double *tnt_summary, double *dev_tnt,
                                unsigned long long *seq, unsigned *arrived, double *gate_sums, unsigned long long *gate_words) {
  if (!h || (n > 0 && !script)) return -1;
  return guarded([&] {
    std::vector<dpgo::Group::CgDebugLaunch> sc(n);
    std::vector<dpgo::Group::GateDebug> gates(n);
    for (int i = 0; i < n; i++) {
      const dpgo_cg_debug_launch_t &q = script[i];
      if (const dpgo_gate_debug_t *g = q.gate) {
        dpgo::Group::GateDebug &o = gates[i];
        o.nslots = g->nslots; o.max_it = g->max_it; o.max_acc = g->max_acc; o.max_hits0 = g->max_hits0; o.max_hits1 = g->max_hits1;
        o.rel_tol = g->rel_tol; o.step_tol = g->step_tol; o.psi = g->psi; o.phi = g->phi;
        o.f = g->f; o.Fk0 = g->Fk0; o.Fk1 = g->Fk1; o.fobj = g->fobj; o.hits0 = g->hits0; o.hits1 = g->hits1;
        sc[i].gate = &o;
      }
      sc[i].kind = q.kind; sc[i].bits = q.bits; sc[i].use_precon = q.use_precon; sc[i].max_it = q.max_it;
      sc[i].grad_tol = q.grad_tol; sc[i].pgrad_tol = q.pgrad_tol; sc[i].kappa = q.kappa; sc[i].theta = q.theta;
      sc[i].rv = q.rv; sc[i].Delta = q.Delta; sc[i].target = q.target; sc[i].partials = q.partials; sc[i].slots = q.slots;
    }
    return h->grp->debug_cg_scalars(sc.data(), n, records, masks, cg_summary, tnt_summary, dev_tnt, seq, arrived, gate_sums, gate_words);
  });
}

int dpgo_group_debug_star_sums(dpgo_group_t *h, const double *partials, unsigned valid, double *out, unsigned long long *seq) {
  if (!h || !h->grp || !partials || !out || !seq || (valid & ~0x3fu)) return -1;
  return guarded([&] { return h->grp->debug_star_sums(partials, valid, out, seq); });
}

int dpgo_group_debug_gated_update(dpgo_group_t *h, unsigned long long go_word, int *report) {
  if (!h || !h->grp || !report || (go_word != 0 && go_word != ~0ull)) return -1;
  return guarded([&] { return h->grp->debug_gated_update(go_word, report); });
}

// ---- the exchange (comm.cpp) ----
// The neighbour-to-neighbour exchange plan of rank `rank` (comm.cpp: p2p_plan) from every rank's exported and
// needed keys.  exp_counts / need_counts: keys per rank; *_nodes / *_poses: the keys, rank after rank.
// Out (may be null to query sizes): npeers; per peer 5 ints (rank, send_off, send_cnt, recv_off, recv_cnt); the send and
// the receive keys (node, pose interleaved).  sizes[0..2] = npeers, send keys, recv keys.
int dpgo_debug_p2p_plan(int rank, int nranks, const int *exp_counts, const int *exp_nodes, const int *exp_poses,
                        const int *need_counts, const int *need_nodes, const int *need_poses, int *peers, int *send_keys,
                        int *recv_keys, int *sizes) {
  if (nranks < 1 || rank < 0 || rank >= nranks || !exp_counts || !need_counts || !sizes) return -1;
  return guarded([&] {
    std::vector<std::vector<dpgo::PoseKey>> ex(nranks), nd(nranks);
    size_t a = 0, b = 0;
    for (int r = 0; r < nranks; r++) {
      for (int k = 0; k < exp_counts[r]; k++, a++) ex[r].push_back({exp_nodes[a], exp_poses[a]});
      for (int k = 0; k < need_counts[r]; k++, b++) nd[r].push_back({need_nodes[b], need_poses[b]});
    }
    const dpgo::P2PPlan P = dpgo::p2p_plan(rank, ex, nd);
    sizes[0] = (int)P.peers.size(); sizes[1] = (int)P.send_keys.size(); sizes[2] = (int)P.recv_keys.size();
    if (peers)
      for (size_t i = 0; i < P.peers.size(); i++) {
        const auto &q = P.peers[i];
        const int v[5] = {q.rank, q.send_off, q.send_cnt, q.recv_off, q.recv_cnt};
        std::copy(v, v + 5, peers + 5 * i);
      }
    if (send_keys) for (size_t i = 0; i < P.send_keys.size(); i++) { send_keys[2 * i] = P.send_keys[i].first; send_keys[2 * i + 1] = P.send_keys[i].second; }
    if (recv_keys) for (size_t i = 0; i < P.recv_keys.size(); i++) { recv_keys[2 * i] = P.recv_keys[i].first; recv_keys[2 * i + 1] = P.recv_keys[i].second; }
    return 0;
  });
}

int dpgo_debug_comm_p2p_self(dpgo_group_t *h) {
  if (!h) return -1;
  return guarded([&] {
    unsigned char id[128];
    if (dpgo::Comm::unique_id(id) != 0) return -1;
    dpgo::Comm c(h->grp, 0, 1, id, /*layout=*/false);   // a communicator of one rank: the group's neighbours need no host
    return c.p2p_self_check();
  });
}

// ---- host forms of device arithmetic, and the pieces of pair_covariance (edges.h, robust.h, pairs.h, sens.h, cert.h) ----
int dpgo_debug_edge_eval_host(const dpgo_graph_t *g, const double *X, int ld, int loss, double loss_reg, double *s_rot,
                              double *s_trans, double *rho, double *weight, dpgo_edge_summary_t *sum) {
  if (!g) return -1;
  return guarded([&] {
    dpgo::EdgeSummary s;
    const int rc = dpgo::edge_eval_host(g->g, X, ld, loss, loss_reg, s_rot, s_trans, rho, weight, &s);
    if (rc == 0 && sum) to_c(s, sum);
    return rc;
  });
}

int dpgo_debug_robust_edge_host(const dpgo_graph_t *g, const double *X, int ld, int loss, double loss_reg, double *w, double *c,
                                double *rows, double *ghat) {
  if (!g) return -1;
  return guarded([&] { return dpgo::robust_edge_host(g->g, X, ld, loss, loss_reg, w, c, rows, ghat); });
}

int dpgo_group_debug_ml_hessian_guarded(dpgo_group_t *h, const dpgo_graph_t *g, const double *X, int ld, int anchor, int pad,
                                        double sentinel, double *guards, double *val, long long cap) {
  if (!h || !h->grp || !g || !X || !guards || !val) return -1;
  return guarded([&] { return h->grp->ml_hessian_guarded(g->g, X, ld, anchor, pad, sentinel, guards, val, cap); });
}

int dpgo_debug_ml_edge_host(const dpgo_graph_t *g, const double *X, int ld, double *r, double *wr, double *chi2, double *Ji,
                            double *Jj, double *grad, double *blocks, long long *near_pi) {
  if (!g) return -1;
  return guarded([&] { return dpgo::ml_edge_host(g->g, X, ld, r, wr, chi2, Ji, Jj, grad, blocks, near_pi); });
}

int dpgo_group_gnc_eval(dpgo_group_t *h, const dpgo_graph_t *g, const double *X, int ld, int kind, double mu, double barc2,
                        const int *robust_set, const double *w_in, double *s_rot, double *s_trans, double *w, double *sums) {
  if (!h || !h->grp || !g || !X || !s_rot || !s_trans || !w || !sums) return -1;
  return guarded([&] { return h->grp->gnc_eval(g->g, X, ld, kind, mu, barc2, robust_set, w_in, s_rot, s_trans, w, sums); });
}

int dpgo_debug_gnc_weight_host(int kind, double mu, double barc2, const double *s, int n, double *w, double *rho) {
  return guarded([&] { return dpgo::gnc_weight_host(kind, mu, barc2, s, n, w, rho); });
}

int dpgo_group_ml_gnc_eval(dpgo_group_t *h, const dpgo_graph_t *g, const double *X, int ld, int kind, double mu, double barc2,
                           const int *robust_set, const double *w_in, int full, double *chi2, double *w, double *sums, double *r,
                           double *wr, double *grad, double *jw) {
  if (!h || !h->grp || !g || !X || !chi2 || !w || !sums) return -1;
  return guarded([&] {
    return h->grp->ml_gnc_eval(g->g, X, ld, kind, mu, barc2, robust_set, w_in, full != 0, chi2, w, sums, r, wr, grad, jw);
  });
}

int dpgo_group_debug_ml_gnc_hessian(dpgo_group_t *h, const dpgo_graph_t *g, const double *X, int ld, int anchor, const int *robust_set,
                                    const double *w_in, int *ptr, int *col, double *val, long long cap, long long *nnz, double *grad) {
  if (!h || !h->grp || !g || !X || !w_in || !nnz) return -1;
  return guarded([&] { return h->grp->ml_gnc_hessian(g->g, X, ld, anchor, robust_set, w_in, ptr, col, val, cap, nnz, grad); });
}

int dpgo_debug_ml_gnc_edge_host(const dpgo_graph_t *g, const double *X, int ld, const double *w, double *r, double *wr, double *chi2,
                                double *grad, double *jw, long long *near_pi, long long *near_pi_all) {
  if (!g) return -1;
  return guarded([&] { return dpgo::ml_gnc_edge_host(g->g, X, ld, w, r, wr, chi2, grad, jw, near_pi, near_pi_all); });
}

int dpgo_debug_pairs_vsolve_baseline(dpgo_group_t *h, const double *X, int ld, int anchor, int ncols, double *ms) {
  if (!h || !h->grp || !X || !ms || ncols < 1) return -1;
  return guarded([&] { return h->grp->pairs_vsolve_baseline(X, ld, anchor, ncols, ms); });
}

int dpgo_debug_pairs_plan(int dof, int anchor, const int *pairs, int npairs, int *poses, int *pair_col, int *sizes) {
  if (dof < 1 || npairs < 0 || (npairs > 0 && (!pairs || !poses || !pair_col)) || !sizes) return -1;
  return guarded([&] {
    const dpgo::PairsPlan pl = dpgo::pairs_plan(dof, anchor, pairs, npairs);
    std::copy(pl.poses.begin(), pl.poses.end(), poses);
    std::copy(pl.pair_col.begin(), pl.pair_col.end(), pair_col);
    sizes[0] = (int)pl.poses.size(); sizes[1] = pl.columns; sizes[2] = pl.batches; sizes[3] = pl.kb;
    return 0;
  });
}

int dpgo_debug_pairs_gate(int d, const double *recp, const double *recq, const double *joint, const double *cand, double *rel,
                          double *gate) {
  if ((d != 2 && d != 3) || !recp || !recq || !joint || !rel || (cand && !gate)) return -1;
  if (cand && (!(cand[d * d + d] > 0) || !(cand[d * d + d + 1] > 0))) return -1;
  const int DD = d == 3 ? 36 : 9;
  if (d == 3) dpgo::pairs_one<3>(recp, recq, joint, joint + DD, joint + 2 * DD, cand, rel, gate);
  else dpgo::pairs_one<2>(recp, recq, joint, joint + DD, joint + 2 * DD, cand, rel, gate);
  return 0;
}

int dpgo_debug_marg_plan(int dof, int anchor, const int *keep, int nkeep, int *poses, int *col, int *sizes) {
  if (dof < 1 || nkeep < 1 || !keep || !poses || !col || !sizes) return -1;
  return guarded([&] {
    const dpgo::MargPlan pl = dpgo::marg_plan(dof, anchor, keep, nkeep);
    std::copy(pl.poses.begin(), pl.poses.end(), poses);
    std::copy(pl.col.begin(), pl.col.end(), col);
    sizes[0] = (int)pl.poses.size(); sizes[1] = pl.columns; sizes[2] = pl.batches; sizes[3] = pl.kb;
    return 0;
  });
}

int dpgo_debug_marg_rel_host(int d, int nkeep, int base_pos, const double *X, const double *sigma, double *cov) {
  return guarded([&] { return dpgo::marg_rel_host(d, nkeep, base_pos, X, sigma, cov); });
}

int dpgo_debug_marg_rel(int device, int d, int nkeep, int base_pos, const double *X, const double *sigma, double *cov) {
  return guarded([&] {
    if (hipSetDevice(device) != hipSuccess) return -1;
    return dpgo::marg_rel_device(d, nkeep, base_pos, X, sigma, cov);
  });
}

int dpgo_debug_marg_dense(int device, int n, const double *A, double *cov, double *info, double *logdet, dpgo_marg_result_t *result) {
  if (n < 1 || !A || !cov || !info || !logdet || !result) return -1;
  return guarded([&] {
    if (hipSetDevice(device) != hipSuccess) return -1;
    dpgo::MargResult r;
    const int rc = dpgo::marg_dense_device(n, A, cov, info, logdet, r);
    to_c(r, result);
    return rc;
  });
}

int dpgo_debug_cand_innov_host(int d, int ncand, int nposes, const int *kpos, const double *X, const double *sigma,
                               const double *candidates, double *cov, double *S, double *residual) {
  return guarded([&] { return dpgo::cand_innov_host(d, ncand, nposes, kpos, X, sigma, candidates, cov, S, residual); });
}

int dpgo_debug_cand_innov(int device, int d, int ncand, int nposes, const int *kpos, const double *X, const double *sigma,
                          const double *candidates, double *cov, double *S, double *residual) {
  return guarded([&] {
    if (hipSetDevice(device) != hipSuccess) return -1;
    return dpgo::cand_innov_device(d, ncand, nposes, kpos, X, sigma, candidates, cov, S, residual);
  });
}

int dpgo_debug_cand_select_host(int d, int ncand, int budget, double d2_max, const double *S, const double *r, const double *weights,
                                int *selected, double *steps, double *sums, int *n_selected) {
  return guarded([&] { return dpgo::cand_select_host(d, ncand, budget, d2_max, S, r, weights, selected, steps, sums, n_selected); });
}

int dpgo_debug_cand_select(int device, int d, int ncand, int budget, double d2_max, const double *S, const double *r,
                           const double *weights, int *selected, double *steps, double *sums, int *n_selected) {
  return guarded([&] {
    if (hipSetDevice(device) != hipSuccess) return -1;
    return dpgo::cand_select_device(d, ncand, budget, d2_max, S, r, weights, selected, steps, sums, n_selected);
  });
}

// ---- the kernels of the Hessian modes on the caller's arrays (modes.h).  The device copies stand between two guard runs of
// MODES_GUARD doubles that must come back untouched (-2 otherwise) ----
namespace {
constexpr size_t MODES_GUARD = 64;
const double MODES_SENTINEL = -7.25e300;
struct GuardedBlock {
  dpgo::DevBuf<double> buf;
  size_t n = 0;
  void put(const double *src, size_t count) {
    n = count;
    std::vector<double> h(count + 2 * MODES_GUARD, MODES_SENTINEL);
    std::copy(src, src + count, h.begin() + MODES_GUARD);
    buf.upload(h);
  }
  double *p() { return buf.p + MODES_GUARD; }
  bool get(double *dst) {   // false: a guard was written
    std::vector<double> h;
    buf.download(h);
    bool ok = true;
    for (size_t i = 0; i < MODES_GUARD; i++) ok = ok && h[i] == MODES_SENTINEL && h[MODES_GUARD + n + i] == MODES_SENTINEL;
    if (dst) std::copy(h.begin() + MODES_GUARD, h.begin() + MODES_GUARD + n, dst);
    return ok;
  }
};
static bool modes_shape_ok(long long n, int b, int ld) { return n >= 1 && n <= (1ll << 40) && b >= 16 && b <= dpgo::MODES_MAX_B && b % 16 == 0 && ld >= b; }
}  // namespace

int dpgo_debug_modes_init(int device, long long n, int b, int ld, int anchor_row0, int dof, unsigned long long seed, double *V) {
  if (!modes_shape_ok(n, b, ld) || !V) return -1;
  return guarded([&] {
    if (hipSetDevice(device) != hipSuccess) return -1;
    GuardedBlock v;
    v.put(V, (size_t)n * ld);
    dpgo::launch_modes_init(nullptr, n, b, ld, anchor_row0, dof, seed, nullptr, 1, v.p());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    return v.get(V) ? 0 : -2;
  });
}

int dpgo_debug_modes_gram(int device, long long n, int b, int ld, const double *W, const double *V, double *G, double *T) {
  if (!modes_shape_ok(n, b, ld) || !W || !V || !G || !T) return -1;
  return guarded([&] {
    if (hipSetDevice(device) != hipSuccess) return -1;
    GuardedBlock w, v;
    w.put(W, (size_t)n * ld);
    v.put(V, (size_t)n * ld);
    dpgo::DevBuf<double> part, packed;
    part.alloc((size_t)dpgo::modes_partials(n, b), false);
    packed.alloc((size_t)b * (b + 1));
    dpgo::launch_modes_gram(nullptr, n, b, ld, w.p(), v.p(), part.p);
    dpgo::launch_modes_reduce_gram(nullptr, dpgo::modes_workgroups(n), b, part.p, packed.p, dpgo::ReadbackFlag{nullptr, nullptr, 0, nullptr});
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    std::vector<double> h;
    packed.download(h);
    dpgo::modes_unpack(b, h.data(), G, T);
    return w.get(nullptr) && v.get(nullptr) ? 0 : -2;
  });
}

int dpgo_debug_modes_update(int device, long long n, int b, int ld, int anchor_row0, int dof, const double *W, double *V,
                            const double *C, const double *theta, double *rr, double *vv) {
  if (!modes_shape_ok(n, b, ld) || !W || !V || !C || !theta || !rr || !vv) return -1;
  return guarded([&] {
    if (hipSetDevice(device) != hipSuccess) return -1;
    GuardedBlock w, v;
    w.put(W, (size_t)n * ld);
    v.put(V, (size_t)n * ld);
    std::vector<double> ct(C, C + (size_t)b * b);
    ct.insert(ct.end(), theta, theta + b);
    dpgo::DevBuf<double> cdev, part, sums;
    cdev.upload(ct);
    part.alloc((size_t)dpgo::modes_partials(n, b), false);
    sums.alloc((size_t)2 * b);
    dpgo::launch_modes_update(nullptr, n, b, ld, anchor_row0, dof, w.p(), v.p(), cdev.p, cdev.p + (size_t)b * b, part.p);
    dpgo::launch_modes_reduce(nullptr, dpgo::modes_workgroups(n), 2 * b, 2 * b, part.p, sums.p, dpgo::ReadbackFlag{nullptr, nullptr, 0, nullptr});
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    std::vector<double> h;
    sums.download(h);
    std::copy(h.begin(), h.begin() + b, rr);
    std::copy(h.begin() + b, h.end(), vv);
    const bool ok_w = w.get(nullptr);
    return v.get(V) && ok_w ? 0 : -2;
  });
}

int dpgo_debug_modes_ritz_host(int b, const double *G, const double *T, double *theta, double *C, int *used) {
  return guarded([&] { return dpgo::modes_ritz(b, G, T, theta, C, used); });
}

int dpgo_debug_modes_ritz(int device, long long n, int b, int ld, const double *W, const double *V, double *theta, double *C, int *used) {
  if (!theta || !C || !used) return -1;
  std::vector<double> G((size_t)std::max(b, 1) * std::max(b, 1)), T(G.size());
  const int rc = dpgo_debug_modes_gram(device, n, b, ld, W, V, G.data(), T.data());
  if (rc != 0) return rc;
  return guarded([&] { return dpgo::modes_ritz(b, G.data(), T.data(), theta, C, used); });
}

int dpgo_debug_sens_edge_host(const dpgo_graph_t *g, const double *X, int ld, const double *lambda, double *sens, double *phi) {
  if (!g) return -1;
  return guarded([&] { return dpgo::sens_edge_host(g->g, X, ld, lambda, sens, phi); });
}

int dpgo_debug_rely_edge_host(int d, int n, const double *rel, const double *r, const double *kappa, const double *tau,
                              double *records) {
  return guarded([&] { return dpgo::rely_edge_host(d, n, rel, r, kappa, tau, records); });
}

int dpgo_debug_rely_edge(int device, int d, int n, const double *rel, const double *r, const double *kappa, const double *tau,
                         double *records) {
  return guarded([&] {
    if (hipSetDevice(device) != hipSuccess) return -1;
    return dpgo::rely_edge_device(d, n, rel, r, kappa, tau, records);
  });
}

int dpgo_debug_ml_rely_edge_host(int d, int n, int sign, const double *J, const double *joint, const double *omega, const double *r,
                                 double *rel, double *records) {
  return guarded([&] { return dpgo::ml_rely_edge_host(d, n, sign, J, joint, omega, r, rel, records); });
}

int dpgo_debug_ml_rely_edge(int device, int d, int n, int sign, const double *J, const double *joint, const double *omega,
                            const double *r, double *rel, double *records) {
  return guarded([&] {
    if (hipSetDevice(device) != hipSuccess) {
      (void)hipGetLastError();   // (the refusal is this call's: no later launch check may find it)
      return -1;
    }
    return dpgo::ml_rely_edge_device(d, n, sign, J, joint, omega, r, rel, records);
  });
}

int dpgo_debug_robust_sens_edge_host(const dpgo_graph_t *g, const double *X, int ld, int loss, double loss_reg, const double *lambda,
                                     double *sens, double *phi) {
  if (!g) return -1;
  return guarded([&] { return dpgo::robust_sens_edge_host(g->g, X, ld, loss, loss_reg, lambda, sens, phi); });
}

int dpgo_debug_rayleigh_ritz(int ns, int nblk, const double *A, const double *B, double *theta, double *C, int *used) {
  if (!A || !B || !theta || !C || !used) return -1;
  return guarded([&] { return dpgo::rayleigh_ritz(ns, nblk, A, B, theta, C, used); });
}

}  // extern "C"
