// Host side of the solution certificate (cert.h): the Rayleigh-Ritz step, the block-Jacobi preconditioner and the
// LOBPCG loop of Group::certify (fast_verification STEP 2, C++/SESync/src/SESync_utils.cpp:765-826;
// C++/Optimization/include/Optimization/LinearAlgebra/LOBPCG.h:131-337), and STEP 1 (:731-754): the pattern of S on
// pose-major unknowns, its multifrontal analysis, and the calls that factor S + eta I on the device (Group::cert_factor,
// Group::verify).
#include "cert.h"

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstring>

#include "cert_state.h"
#include "group.h"

namespace dpgo {

// ---------------------------------------------------------------------------
// Rayleigh-Ritz on the host: n <= 9
// ---------------------------------------------------------------------------
namespace {
constexpr int RR_MAX = 9;

// cyclic Jacobi: A (n x n, symmetric, overwritten) = Z diag(w) Z^T
void jacobi_eig(int n, double A[RR_MAX][RR_MAX], double Z[RR_MAX][RR_MAX], double *w) {
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
}  // namespace

int sym_eig(int n, const double *A, double *Z, double *w) {
  if (n < 1 || n > RR_MAX || !A || !Z || !w) return -1;
  double As[RR_MAX][RR_MAX], Zv[RR_MAX][RR_MAX];
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) As[i][j] = 0.5 * (A[(size_t)i * n + j] + A[(size_t)j * n + i]);
  jacobi_eig(n, As, Zv, w);
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) Z[(size_t)i * n + j] = Zv[i][j];
  return 0;
}

int rayleigh_ritz(int ns, int nblk, const double *A, const double *B, double *theta, double *C, int *used_out) {
  const int nfull = ns * nblk;
  if (ns < 1 || nblk < 1 || nfull > RR_MAX || !A || !B || !theta || !C) return -1;
  for (int used = nblk; used >= 1; used--) {
    const int n = ns * used;
    double dscale[RR_MAX], L[RR_MAX][RR_MAX], As[RR_MAX][RR_MAX], Zv[RR_MAX][RR_MAX], w[RR_MAX];
    bool ok = true;
    for (int i = 0; i < n; i++) {
      const double b = B[(size_t)i * nfull + i];
      if (!(b > 0.0) || !std::isfinite(b)) { ok = false; break; }
      dscale[i] = 1.0 / std::sqrt(b);
    }
    if (!ok) continue;
    // Cholesky of the scaled mass matrix (both triangles of the input are averaged)
    for (int j = 0; j < n && ok; j++) {
      for (int i = j; i < n; i++) {
        double s = 0.5 * (B[(size_t)i * nfull + j] + B[(size_t)j * nfull + i]) * dscale[i] * dscale[j];
        for (int k = 0; k < j; k++) s -= L[i][k] * L[j][k];
        if (i == j) {
          if (!(s >= 1e-12)) { ok = false; break; }
          L[j][j] = std::sqrt(s);
        } else {
          L[i][j] = s / L[j][j];
        }
      }
    }
    if (!ok) continue;
    // As <- L^-1 (D A D) L^-T
    for (int i = 0; i < n; i++)
      for (int j = 0; j < n; j++) As[i][j] = 0.5 * (A[(size_t)i * nfull + j] + A[(size_t)j * nfull + i]) * dscale[i] * dscale[j];
    for (int c = 0; c < n; c++)       // columns: L Y = As
      for (int i = 0; i < n; i++) {
        double s = As[i][c];
        for (int k = 0; k < i; k++) s -= L[i][k] * As[k][c];
        As[i][c] = s / L[i][i];
      }
    for (int r = 0; r < n; r++)       // rows: Y L^-T
      for (int j = 0; j < n; j++) {
        double s = As[r][j];
        for (int k = 0; k < j; k++) s -= As[r][k] * L[j][k];
        As[r][j] = s / L[j][j];
      }
    for (int i = 0; i < n; i++)
      for (int j = i + 1; j < n; j++) As[i][j] = As[j][i] = 0.5 * (As[i][j] + As[j][i]);
    jacobi_eig(n, As, Zv, w);
    int idx[RR_MAX];
    for (int i = 0; i < n; i++) idx[i] = i;
    std::stable_sort(idx, idx + n, [&](int a, int b) { return w[a] < w[b]; });
    std::fill(C, C + (size_t)nfull * ns, 0.0);
    for (int j = 0; j < ns; j++) {
      theta[j] = w[idx[j]];
      double c[RR_MAX];
      for (int i = n - 1; i >= 0; i--) {   // L^T c = z
        double s = Zv[i][idx[j]];
        for (int k = i + 1; k < n; k++) s -= L[k][i] * c[k];
        c[i] = s / L[i][i];
      }
      for (int i = 0; i < n; i++) C[(size_t)i * ns + j] = dscale[i] * c[i];
    }
    if (used_out) *used_out = used;
    return 0;
  }
  return -1;
}

// ---------------------------------------------------------------------------
// the group's certificate state
// ---------------------------------------------------------------------------
void Group::cert_release() {
  delete cert_;
  cert_ = nullptr;
}

namespace {
// standard Gaussians from a seeded host generator: splitmix64 + Box-Muller
struct Gauss {
  unsigned long long s;
  explicit Gauss(unsigned long long seed) : s(seed) {}
  unsigned long long next() {
    unsigned long long z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  }
  double uniform() { return ((double)(next() >> 11) + 0.5) * (1.0 / 9007199254740992.0); }   // (0, 1)
  void fill(std::vector<double> &v) {
    for (size_t i = 0; i < v.size(); i += 2) {
      const double r = std::sqrt(-2.0 * std::log(uniform())), a = 6.283185307179586476925 * uniform();
      v[i] = r * std::cos(a);
      if (i + 1 < v.size()) v[i + 1] = r * std::sin(a);
    }
  }
};
}  // namespace

// What every entry needs: the arguments checked, the optimiser's pending work taken, the buffers there.
int Group::cert_begin(const double *X, int ld) {
  const int N = num_poses_global_;
  if (!X || ld < (d_ + 1) * N) {
    fprintf(stderr, "[dpgo_amd] ERROR: certificate: inconsistent size of X.\n");
    return -1;
  }
  return cert_ready();
}

// ... and the part of it that does not depend on X
int Group::cert_ready() {
  const int N = num_poses_global_;
  if (opt_.loss != 0) {
    fprintf(stderr, "[dpgo_amd] ERROR: certificate: the group was created with a robust loss; the certificate is that of the "
                    "trivial loss (create a group with LOSS_NONE and max_iterations = 0).\n");
    return -1;
  }
  if (num_local() != num_nodes_total_ || (int)gather_dst_.n != P1_ || P0_ != N) {
    fprintf(stderr, "[dpgo_amd] ERROR: certificate: the group must host every node of the graph.\n");
    return -1;
  }
  // the optimiser's deferred read-back and a pending exchange first: nothing of its state is touched below (own buffers, own
  // partial sums, own pinned block; launches on the group's stream, eagerly, with the schedule's flag like any read-back)
  finish_update();
  join_exchange();
  sync();
  if (!cert_) {
    cert_ = new CertState();
    CertState &c = *cert_;
    const size_t nall = (size_t)(P0_ + P1_) * RS_, nown = (size_t)P0_ * RS_;
    for (DevBuf<double> *b : {&c.X, &c.V, &c.W, &c.P}) b->alloc(nall);
    for (DevBuf<double> *b : {&c.MX, &c.SV, &c.SW, &c.SP, &c.tmp}) b->alloc(nown);
    c.Lam.alloc((size_t)P0_ * d_ * d_);
    c.partials.alloc((size_t)cert_nsums(d_) * std::max(T_.nseg_own, 1));
    HIP_CHECK(hipHostMalloc((void **)&c.h_sums, sizeof(double) * cert_nsums(d_), hipHostMallocDefault));
    std::memset(c.h_sums, 0, sizeof(double) * cert_nsums(d_));
    c.gid.resize(P0_);
    for (int a = 0; a < num_local(); a++)
      for (int k = 0; k < info_[a].n[0]; k++) c.gid[own_off_[a] + k] = g_index_[a].at(info_[a].own_pose[k]);
  }
  return 0;
}

// a global (d+1)N x d matrix (reference layout) into the own rows of a record array; the neighbour rows (zeroed here unless
// the array has none: with_nbr = false) follow by the halo copy
void Group::cert_upload(const double *M, int ld, int ncols, double *dev_all, bool with_nbr) {
  const int N = num_poses_global_;
  std::vector<double> rec((size_t)(P0_ + (with_nbr ? P1_ : 0)) * RS_, 0.0);
  for (int row = 0; row < P0_; row++) {
    const int g = cert_->gid[row];
    double *r = &rec[(size_t)row * RS_];
    for (int c = 0; c < ncols; c++) {
      r[c] = M[(size_t)c * ld + g];
      for (int k = 0; k < d_; k++) r[d_ + k * d_ + c] = M[(size_t)c * ld + N + g * d_ + k];
    }
  }
  HIP_CHECK(hipMemcpyAsync(dev_all, rec.data(), sizeof(double) * rec.size(), hipMemcpyHostToDevice, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
}

void Group::cert_download(const double *dev_own, double *M, int ld, int ncols) {
  const int N = num_poses_global_;
  std::vector<double> rec((size_t)P0_ * RS_);
  HIP_CHECK(hipMemcpyAsync(rec.data(), dev_own, sizeof(double) * rec.size(), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
  for (int row = 0; row < P0_; row++) {
    const int g = cert_->gid[row];
    const double *r = &rec[(size_t)row * RS_];
    for (int c = 0; c < ncols; c++) {
      M[(size_t)c * ld + g] = r[c];
      for (int k = 0; k < d_; k++) M[(size_t)c * ld + N + g * d_ + k] = r[d_ + k * d_ + c];
    }
  }
}

// out (own rows) = M in: the halo copy inside the group, then the two block-sparse passes evaluate_global makes for the
// gradient of the trivial loss (S, then G with the first product added)
void Group::cert_apply_M(double *in_all, double *out_own) {
  const NodeMask all{all_bits(), nullptr};
  if (gather_dst_.n) launch_copy_indexed(d_, st_, (int)gather_dst_.n, gather_dst_.p, gather_src_.p, in_all, in_all);
  launch_bsr(lc(all), S_.dev, {.x = in_all, .y = cert_->tmp.p});
  launch_bsr(lc(all), G_.dev, {.x = in_all, .addv = cert_->tmp.p, .y = out_own});
}
void Group::cert_apply_S(double *in_all, double *out_own) {
  cert_apply_M(in_all, out_own);
  launch_cert_apply(lc(NodeMask{all_bits(), nullptr}), cert_->Lam.p, in_all, out_own, out_own);
}

// X on the device, M X, the Lambda blocks and |S X|_F
int Group::cert_prepare(const double *X, int ld, double *stationarity) {
  CertState &c = *cert_;
  cert_upload(X, ld, d_, c.X.p);
  cert_apply_M(c.X.p, c.MX.p);
  launch_cert_lambda(lc(NodeMask{all_bits(), nullptr}), c.X.p, c.MX.p, c.Lam.p, nullptr, c.partials.p);
  launch_cert_reduce(st_, T_, 1, c.partials.p, c.h_sums, sched_.flag());
  wait_flag(sched_.last_seq());
  if (stationarity) *stationarity = std::sqrt(c.h_sums[0]);
  return 0;
}

int Group::cert_lambda(const double *X, int ld, double *Lambda) {
  if (!Lambda || cert_begin(X, ld) != 0) return -1;
  cert_prepare(X, ld, nullptr);
  std::vector<double> L((size_t)P0_ * d_ * d_);
  HIP_CHECK(hipMemcpy(L.data(), cert_->Lam.p, sizeof(double) * L.size(), hipMemcpyDeviceToHost));
  for (int row = 0; row < P0_; row++)
    std::copy(&L[(size_t)row * d_ * d_], &L[(size_t)(row + 1) * d_ * d_], Lambda + (size_t)cert_->gid[row] * d_ * d_);
  return 0;
}

int Group::cert_apply(const double *X, int ld, const double *V, int ldv, double *SV, int ldsv) {
  const int rows = (d_ + 1) * num_poses_global_;
  if (!V || !SV || ldv < rows || ldsv < rows) {
    fprintf(stderr, "[dpgo_amd] ERROR: certificate: inconsistent size of V.\n");
    return -1;
  }
  if (cert_begin(X, ld) != 0) return -1;
  CertState &c = *cert_;
  cert_prepare(X, ld, nullptr);
  cert_upload(V, ldv, d_, c.V.p);
  cert_apply_S(c.V.p, c.SV.p);
  cert_download(c.SV.p, SV, ldsv, d_);
  return 0;
}

// T_p = (M_pp)^-1, M_pp the pose's diagonal block of M = G + S (the inter-node terms and the regulariser cancel between the two);
// the identity for a pose without an edge (or a block that is not positive definite).  Independent of X: built once.
void Group::cert_build_precon() {
  CertState &c = *cert_;
  if (c.have_Tp) return;
  const int B = B_, BB = B * B;
  std::vector<double> Tp((size_t)P0_ * BB, 0.0);
  for (int a = 0; a < num_local(); a++)
    for (int r = 0; r < info_[a].n[0]; r++) {
      double M[16] = {0}, L[16] = {0}, Li[16] = {0};
      for (const BsrMatrix *A : {&ops_[a].G, &ops_[a].S})
        for (int k = A->ptr[r]; k < A->ptr[r + 1]; k++)
          if (A->col[k] == r)
            for (int e = 0; e < BB; e++) M[e] += A->val[(size_t)k * BB + e];
      double scale = 0;
      for (int i = 0; i < B; i++) scale = std::max(scale, std::fabs(M[i * B + i]));
      bool ok = scale > 0;
      for (int j = 0; j < B && ok; j++)
        for (int i = j; i < B; i++) {
          double s = 0.5 * (M[i * B + j] + M[j * B + i]);
          for (int k = 0; k < j; k++) s -= L[i * B + k] * L[j * B + k];
          if (i == j) {
            if (!(s > 1e-12 * scale)) { ok = false; break; }
            L[j * B + j] = std::sqrt(s);
          } else {
            L[i * B + j] = s / L[j * B + j];
          }
        }
      double *T = &Tp[(size_t)(own_off_[a] + r) * BB];
      if (!ok) {
        for (int i = 0; i < B; i++) T[i * B + i] = 1.0;
        continue;
      }
      for (int cidx = 0; cidx < B; cidx++)   // Li = L^-1
        for (int i = 0; i < B; i++) {
          double s = i == cidx ? 1.0 : 0.0;
          for (int k = 0; k < i; k++) s -= L[i * B + k] * Li[k * B + cidx];
          Li[i * B + cidx] = s / L[i * B + i];
        }
      for (int i = 0; i < B; i++)            // T = Li^T Li
        for (int j = 0; j < B; j++) {
          double s = 0;
          for (int k = 0; k < B; k++) s += Li[k * B + i] * Li[k * B + j];
          T[i * B + j] = s;
        }
    }
  c.Tp.upload(Tp);
  c.have_Tp = true;
}

// ---------------------------------------------------------------------------
// STEP 1: the Cholesky factorisation of S + eta I (SESync_utils.cpp:731-754)
// ---------------------------------------------------------------------------
// The pattern of M = G + S on pose-major unknowns, once per group: one dense B x B block per pair (p, q) that has a block
// in a node's G or S (the walk of cert_build_precon over every block, the neighbour columns of S at their unified own
// rows; the inter-node and xi terms cancel between the two), the diagonal block always, and the transposed pair of every
// pair, so that the pattern is symmetric whatever the assembly stored.  Structural zeros are explicit: the quotient
// graph of B consecutive unknowns is then exactly the pose graph.
void Group::cert_build_pattern() {
  CertState &c = *cert_;
  if (c.have_pattern) return;
  const int B = B_, BB = B * B, N = P0_;
  c.row_of.resize(N);
  for (int p = 0; p < N; p++) c.row_of[c.gid[p]] = p;
  std::vector<int> nbr_row(std::max(P1_, 1), -1);   // neighbour record -> the unified own row of the pose it copies
  for (int a = 0; a < num_local(); a++)
    for (int k = 0; k < info_[a].n[1]; k++) {
      const auto key = info_[a].nbr_key[k];
      const int b = local_of_node_.at(key.first);
      nbr_row[nbr_off_[a] + k] = own_off_[b] + info_[b].index.at(key);
    }
  typedef std::pair<int, std::array<double, 16>> Blk;
  std::vector<std::vector<Blk>> rows(N);
  auto at = [&](int p, int q) -> std::array<double, 16> & {
    for (Blk &b : rows[p])
      if (b.first == q) return b.second;
    rows[p].push_back({q, {}});
    rows[p].back().second.fill(0.0);
    return rows[p].back().second;
  };
  for (int a = 0; a < num_local(); a++) {
    const int n0 = info_[a].n[0];
    for (int r = 0; r < n0; r++) {
      const int p = own_off_[a] + r;
      at(p, p);
      for (const BsrMatrix *A : {&ops_[a].G, &ops_[a].S})
        for (int k = A->ptr[r]; k < A->ptr[r + 1]; k++) {
          const int cl = A->col[k], q = cl < n0 ? own_off_[a] + cl : nbr_row[nbr_off_[a] + cl - n0];
          std::array<double, 16> &m = at(p, q);
          for (int e = 0; e < BB; e++) m[e] += A->val[(size_t)k * BB + e];
        }
    }
  }
  for (int p = 0; p < N; p++)
    for (size_t k = 0; k < rows[p].size(); k++) at(rows[p][k].first, p);
  c.bptr_h.assign(N + 1, 0);
  for (int p = 0; p < N; p++) {
    std::sort(rows[p].begin(), rows[p].end(), [](const Blk &x, const Blk &y) { return x.first < y.first; });
    c.bptr_h[p + 1] = c.bptr_h[p] + (int)rows[p].size();
  }
  const size_t nblk = c.bptr_h[N], nnz = nblk * BB;
  if (nnz > (size_t)0x7fffffff) throw DeviceError("certificate: the matrix has more than 2^31 entries");
  std::vector<int> diag(nblk, -1);
  std::vector<double> Mval(nnz);
  c.A.n = B * N;
  c.A.ptr.assign((size_t)B * N + 1, 0);
  c.A.col.resize(nnz);
  for (int p = 0; p < N; p++) {
    const int nb = (int)rows[p].size();
    const size_t base = (size_t)BB * c.bptr_h[p];
    for (int r = 0; r < B; r++) {
      c.A.ptr[(size_t)B * p + r + 1] = (int)(base + (size_t)(r + 1) * B * nb);
      for (int j = 0; j < nb; j++)
        for (int cc = 0; cc < B; cc++) {
          const size_t e = base + (size_t)r * B * nb + (size_t)j * B + cc;
          c.A.col[e] = B * rows[p][j].first + cc;
          Mval[e] = rows[p][j].second[r * B + cc];
        }
    }
    for (int j = 0; j < nb; j++)
      if (rows[p][j].first == p) diag[c.bptr_h[p] + j] = p;
  }
  c.bptr.upload(c.bptr_h);
  c.diag_pose.upload(diag);
  c.Mval.upload(Mval);
  c.have_pattern = true;
}

int Group::own_row(int global_pose) const { return cert_->row_of[global_pose]; }

// the block of the pattern that holds (p, q), unified own rows; -1: none
int Group::cert_block_of(int p, int q) const {
  const CertState &c = *cert_;
  const int B = B_, b0 = c.bptr_h[p], nb = c.bptr_h[p + 1] - b0;
  for (int j = 0; j < nb; j++)
    if (c.A.col[(size_t)B * B * b0 + (size_t)j * B] / B == q) return b0 + j;
  return -1;
}

// The analysis (first call), the prediction, the refusal, the numeric context (first call that is not refused).
int Group::cert_factor_setup(long long max_factor_bytes, CertFactor &out) {
  CertState &c = *cert_;
  cert_build_pattern();
  if (!c.have_symbolic) {
    const auto t0 = std::chrono::steady_clock::now();
    // collapse = 1: the merge model of spd_factor prices solves, and nothing is solved here.  leaf: 64 unknowns, 16 poses
    // at d = 3 -- the 125 poses of smallGrid3D come apart into four levels, the 9 of tinyGrid3D stay one front -- and more
    // where that many leaves would not fit the 65535 fronts a level's launch can index (two leaves per `leaf` unknowns
    // at the worst)
    const long long n = c.A.n;
    const int leaf = (int)std::max<long long>(64, B_ * ((2 * n / B_ + 59999) / 60000));
    c.F.quiet = true;         // a non-positive pivot is a verdict here
    c.F.factor_only = true;   // no W / WT: nothing is solved with this factor
    if (spd_symbolic(c.A, c.F, leaf, 1, B_) != 0) {
      fprintf(stderr, "[dpgo_amd] ERROR: certificate: the symbolic analysis of S failed.\n");
      return -1;
    }
    c.factor_bytes = (long long)spd_numeric_bytes(c.F, (long long)c.A.col.size());
    c.symbolic_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    out.symbolic_s = c.symbolic_s;
    c.have_symbolic = true;
  }
  out.fronts = c.F.nfronts;
  out.levels = (int)c.F.by_height.size();
  out.max_front = c.F.max_front;
  out.factor_entries = c.F.entries;
  out.factor_bytes = c.factor_bytes;
  out.outcome = CERT_FACTOR_SKIPPED;
  if (max_factor_bytes > 0 && c.factor_bytes > max_factor_bytes) return 1;
  if (!c.F.numeric) {
    size_t free_b = 0, total_b = 0;
    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    if ((unsigned long long)c.factor_bytes > free_b / 2) return 1;   // (nothing that cannot fit is asked of a shared device)
    if (spd_prepare_device(c.A, c.F) != 0) {
      fprintf(stderr, "[dpgo_amd] ERROR: certificate: the device state of the factorisation could not be set up.\n");
      return -1;
    }
  }
  return 0;
}

int Group::cert_factor(const double *X, int ld, double eta, long long max_factor_bytes, CertFactor &out) {
  out = CertFactor();
  out.eta = eta;
  if (!std::isfinite(eta)) {
    fprintf(stderr, "[dpgo_amd] ERROR: certificate: eta is not finite.\n");
    return -1;
  }
  if (cert_begin(X, ld) != 0) return -1;
  const int ready = cert_factor_setup(max_factor_bytes, out);
  if (ready < 0) return -1;
  cert_prepare(X, ld, &out.stationarity);
  if (ready != 0) return 0;   // SKIPPED, with what the analysis predicts
  return cert_factor_numeric(eta, out);
}

// S + eta I from the Lambda in CertState, factored: the verdict
int Group::cert_factor_numeric(double eta, CertFactor &out) {
  CertState &c = *cert_;
  const auto t0 = std::chrono::steady_clock::now();
  launch_cert_matrix(d_, st_, P0_, c.bptr.p, c.diag_pose.p, c.Mval.p, c.Lam.p, eta, spd_numeric_values(c.F));
  const int rc = spd_refactor_device(c.F, st_, false);   // (returns with the verdict read: the stream has drained)
  out.numeric_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (rc != 0 && !c.F.not_pd) {
    fprintf(stderr, "[dpgo_amd] ERROR: certificate: the factorisation failed on the device.\n");
    return -1;
  }
  out.outcome = rc == 0 ? CERT_FACTOR_PD : CERT_FACTOR_NOT_PD;
  out.pivot_max = c.F.pivot_max;
  out.pivot_min = c.F.pivot_max > 0 ? c.F.pivot_min : 0.0;   // (no front factored: nothing recorded)
  return 0;
}

int Group::cert_matrix(const double *X, int ld, double eta, int *ptr, int *col, double *val, long long cap, long long *nnz) {
  if (!nnz || !std::isfinite(eta) || cert_begin(X, ld) != 0) return -1;
  CertState &c = *cert_;
  cert_build_pattern();
  *nnz = (long long)c.A.col.size();
  if (!ptr && !col && !val) return 0;   // (the size alone)
  if (!ptr || !col || !val || cap < *nnz) {
    fprintf(stderr, "[dpgo_amd] ERROR: certificate: cert_matrix needs room for %lld entries.\n", *nnz);
    return -1;
  }
  CertFactor f;
  if (cert_factor_setup(0, f) != 0) {
    fprintf(stderr, "[dpgo_amd] ERROR: certificate: the value array of the factorisation does not fit the device.\n");
    return -1;
  }
  cert_prepare(X, ld, nullptr);
  launch_cert_matrix(d_, st_, P0_, c.bptr.p, c.diag_pose.p, c.Mval.p, c.Lam.p, eta, spd_numeric_values(c.F));
  std::vector<double> v(c.A.col.size());
  HIP_CHECK(hipMemcpyAsync(v.data(), spd_numeric_values(c.F), sizeof(double) * v.size(), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
  cert_csr_out(v, ptr, col, val);
  return 0;
}

// handed out on GLOBAL poses -- unknown (d+1) g + r, g = gid[p] -- rows in that order, a row's blocks by ascending pose
void Group::cert_csr_out(const std::vector<double> &v, int *ptr, int *col, double *val) {
  CertState &c = *cert_;
  const int B = B_, BB = B * B, N = P0_;
  std::vector<int> order;
  size_t e = 0;
  ptr[0] = 0;
  for (int g = 0; g < N; g++) {
    const int p = own_row(g), b0 = c.bptr_h[p], nb = c.bptr_h[p + 1] - b0;
    const size_t base = (size_t)BB * b0;
    auto pose_of = [&](int j) { return c.gid[c.A.col[base + (size_t)j * B] / B]; };
    order.resize(nb);
    for (int j = 0; j < nb; j++) order[j] = j;
    std::sort(order.begin(), order.end(), [&](int x, int y) { return pose_of(x) < pose_of(y); });
    for (int r = 0; r < B; r++) {
      for (int j : order)
        for (int cc = 0; cc < B; cc++, e++) {
          col[e] = B * pose_of(j) + cc;
          val[e] = v[base + (size_t)r * B * nb + (size_t)j * B + cc];
        }
      ptr[(size_t)B * g + r + 1] = (int)e;
    }
  }
}

static bool cert_options_ok(const CertOptions &o, int rows, const double *V0, int ldv0, const double *x_out, int ldx) {
  return o.eta >= 0 && o.tau > 0 && o.max_iters >= 0 && o.refresh_every >= 0 && !(V0 && ldv0 < rows) && !(x_out && ldx < rows);
}

// fast_verification (SESync_utils.cpp:721-830): STEP 1, and STEP 2 only when it did not succeed
int Group::verify(const double *X, int ld, const CertOptions &o, long long max_factor_bytes, const double *V0, int ldv0,
                  CertResult &res, double *x_out, int ldx, CertFactor &fac) {
  res = CertResult();
  fac = CertFactor();
  if (!cert_options_ok(o, (d_ + 1) * num_poses_global_, V0, ldv0, x_out, ldx)) {
    fprintf(stderr, "[dpgo_amd] ERROR: verify: bad options or inconsistent size of V0 / x.\n");
    return -1;
  }
  if (cert_factor(X, ld, o.eta, max_factor_bytes, fac) != 0) return -1;
  if (fac.outcome == CERT_FACTOR_PD) {
    res.status = CERT_PROVEN;
    res.stationarity = fac.stationarity;
    return 0;
  }
  const int rc = certify(X, ld, o, V0, ldv0, res, x_out, ldx);
  // a search that converged to a Ritz value >= -eta / 2 has just been refuted by the factorisation
  if (rc == 0 && fac.outcome == CERT_FACTOR_NOT_PD && res.status == CERT_NONNEGATIVE) res.status = CERT_UNDECIDED;
  return rc;
}

// verify on the Lambda in CertState (the staircase's: Lambda of a lifted point); cert_begin has run
int Group::verify_lambda(const CertOptions &o, long long max_factor_bytes, double stationarity, CertResult &res, double *x_out,
                         int ldx, CertFactor &fac) {
  res = CertResult();
  fac = CertFactor();
  fac.eta = o.eta;
  if (!cert_options_ok(o, (d_ + 1) * num_poses_global_, nullptr, 0, x_out, ldx)) return -1;
  const int ready = cert_factor_setup(max_factor_bytes, fac);
  if (ready < 0) return -1;
  fac.stationarity = res.stationarity = stationarity;
  if (ready == 0 && cert_factor_numeric(o.eta, fac) != 0) return -1;
  if (fac.outcome == CERT_FACTOR_PD) {
    res.status = CERT_PROVEN;
    return 0;
  }
  if (o.precondition) cert_build_precon();
  const int rc = cert_search(o, nullptr, 0, res, x_out, ldx);
  if (rc == 0 && fac.outcome == CERT_FACTOR_NOT_PD && res.status == CERT_NONNEGATIVE) res.status = CERT_UNDECIDED;
  return rc;
}

int Group::certify(const double *X, int ld, const CertOptions &o, const double *V0, int ldv0, CertResult &res, double *x_out, int ldx) {
  const int rows = (d_ + 1) * num_poses_global_;
  res = CertResult();
  if (!(o.eta >= 0) || !(o.tau > 0) || o.max_iters < 0 || o.refresh_every < 0 || (V0 && ldv0 < rows) || (x_out && ldx < rows)) {
    fprintf(stderr, "[dpgo_amd] ERROR: certify: bad options or inconsistent size of V0 / x.\n");
    return -1;
  }
  if (cert_begin(X, ld) != 0) return -1;
  if (o.precondition) cert_build_precon();
  cert_prepare(X, ld, &res.stationarity);
  return cert_search(o, V0, ldv0, res, x_out, ldx);
}

// The search on S = M - Lambda with the Lambda in CertState (res.stationarity is the caller's)
int Group::cert_search(const CertOptions &o, const double *V0, int ldv0, CertResult &res, double *x_out, int ldx) {
  const int N = num_poses_global_, rows = (d_ + 1) * N, d = d_;
  CertState &c = *cert_;
  const NodeMask all{all_bits(), nullptr};
  const int NT = cert_ntri(d), n3 = 3 * d, nsums = cert_nsums(d);

  // |S| ~ |S Omega|_F / |Omega|_F on a Gaussian block (LOBPCG.h:199-214)
  std::vector<double> blk((size_t)rows * d), tmp((size_t)rows * d);
  {
    Gauss g(o.seed ^ 0x5eedc0de5eedc0deull);
    g.fill(blk);
    cert_upload(blk.data(), rows, d, c.V.p);
    cert_apply_S(c.V.p, c.SV.p);
    cert_download(c.SV.p, tmp.data(), rows, d);
    double a = 0, b = 0;
    for (size_t i = 0; i < blk.size(); i++) {
      a += tmp[i] * tmp[i];
      b += blk[i] * blk[i];
    }
    res.S_norm_est = std::sqrt(a / b);
  }
  // the initial block: the caller's, or seeded Gaussians
  if (V0) {
    cert_upload(V0, ldv0, d, c.V.p);
  } else {
    Gauss g(o.seed);
    g.fill(blk);
    cert_upload(blk.data(), rows, d, c.V.p);
  }
  cert_apply_S(c.V.p, c.SV.p);
  HIP_CHECK(hipMemsetAsync(c.W.p, 0, sizeof(double) * c.W.n, st_));
  HIP_CHECK(hipMemsetAsync(c.P.p, 0, sizeof(double) * c.P.n, st_));
  HIP_CHECK(hipMemsetAsync(c.SW.p, 0, sizeof(double) * c.SW.n, st_));
  HIP_CHECK(hipMemsetAsync(c.SP.p, 0, sizeof(double) * c.SP.n, st_));

  const double *h = c.h_sums;
  if (cert_trace_on_) cert_trace_.clear();
  double theta0 = 0;
  bool have_norms = false, have_W = false, drop_P = true;   // (the first Rayleigh-Ritz step sees V alone, the second [V W])
  std::vector<double> xg(rows), sx(rows);
  for (;;) {
    while (res.iterations < o.max_iters) {
      if (have_W) cert_apply_M(c.W.p, c.SW.p);   // (S W is finished by k_cert_gram)
      launch_cert_gram(lc(all), c.Lam.p, c.V.p, c.W.p, c.P.p, c.SV.p, c.SW.p, c.SP.p, c.partials.p);
      launch_cert_reduce(st_, T_, nsums, c.partials.p, c.h_sums, sched_.flag());
      wait_flag(sched_.last_seq());
      // the stopping test of the LAST update, one product late (LOBPCG.h:298-307)
      if (have_norms) {
        const double r0 = std::sqrt(h[2 * NT]), x0 = std::sqrt(h[2 * NT + d]);
        if (r0 <= o.tau * (res.S_norm_est + std::fabs(theta0)) * x0) break;
      }
      const int nblk = !have_W ? 1 : drop_P ? 2 : 3, n = d * nblk;
      double A[81], Bm[81], th[3], C[27];
      for (int a = 0; a < n; a++)
        for (int b = a; b < n; b++) {
          Bm[a * n + b] = Bm[b * n + a] = h[cert_tri(n3, a, b)];
          A[a * n + b] = A[b * n + a] = h[NT + cert_tri(n3, a, b)];
        }
      int used = 0;
      if (rayleigh_ritz(d, nblk, A, Bm, th, C, &used) != 0) {
        fprintf(stderr, "[dpgo_amd] ERROR: certify: the block has lost its rank (V^T V is not positive definite).\n");
        return -1;
      }
      if (used < nblk) res.restarts++;
      CertCoef K;
      std::memset(&K, 0, sizeof(K));
      for (int i = 0; i < n; i++)
        for (int j = 0; j < d; j++) K.C[i * d + j] = C[i * d + j];
      for (int j = 0; j < d; j++) K.theta[j] = th[j];
      launch_cert_update(lc(all), K, o.precondition ? c.Tp.p : nullptr, c.V.p, c.W.p, c.P.p, c.SV.p, c.SW.p, c.SP.p,
                         c.partials.p);
      if (cert_trace_on_) cert_trace_pass(h, nblk, used, K);
      res.iterations++;
      theta0 = th[0];
      have_norms = true;
      drop_P = !have_W;   // (P' = 0 after the step that had no W)
      have_W = true;
      if (o.stop_on_negative && theta0 < -0.5 * o.eta) break;   // SESync_utils.cpp:775-793
      if (o.refresh_every > 0 && res.iterations % o.refresh_every == 0) {
        cert_apply_S(c.V.p, c.SV.p);
        cert_apply_S(c.P.p, c.SP.p);
        if (cert_trace_on_) cert_trace_.back() = 1.0;
      }
    }
    // the returned vector: column 0 of V, normalised; theta and the residual from one fresh product S x
    {
      std::vector<double> Vh((size_t)rows * d);
      cert_download(c.V.p, Vh.data(), rows, d);
      double nrm = 0;
      for (int i = 0; i < rows; i++) nrm += Vh[i] * Vh[i];
      nrm = std::sqrt(nrm);
      if (!(nrm > 0) || !std::isfinite(nrm)) {
        fprintf(stderr, "[dpgo_amd] ERROR: certify: the iterate is not finite.\n");
        return -1;
      }
      for (int i = 0; i < rows; i++) xg[i] = Vh[i] / nrm;
      double n2 = 0;   // (once more: the division's rounding)
      for (int i = 0; i < rows; i++) n2 += xg[i] * xg[i];
      n2 = std::sqrt(n2);
      for (int i = 0; i < rows; i++) xg[i] /= n2;
      cert_upload(xg.data(), rows, 1, c.X.p);   // (X itself is no longer needed: Lambda is there)
      cert_apply_S(c.X.p, c.MX.p);
      cert_download(c.MX.p, sx.data(), rows, 1);
      double th = 0, r2 = 0;
      for (int i = 0; i < rows; i++) th += xg[i] * sx[i];
      for (int i = 0; i < rows; i++) {
        const double e = sx[i] - th * xg[i];
        r2 += e * e;
      }
      res.theta = th;
      res.residual = std::sqrt(r2);
    }
    if (res.theta < -0.5 * o.eta) res.status = CERT_NEGATIVE;
    else if (res.residual <= o.tau * (res.S_norm_est + std::fabs(res.theta))) res.status = CERT_NONNEGATIVE;
    else res.status = CERT_UNDECIDED;
    if (res.status != CERT_UNDECIDED || res.iterations >= o.max_iters) break;
    // the recurrences said "done", the fresh product does not: real products, and on
    cert_apply_S(c.V.p, c.SV.p);
    cert_apply_S(c.P.p, c.SP.p);
    have_norms = false;
  }
  if (x_out) std::copy(xg.begin(), xg.end(), x_out);
  return 0;
}

}  // namespace dpgo
