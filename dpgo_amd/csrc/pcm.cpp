// PCM host side: the measurement records of PCM::update (C++/DPGO/src/PCM.cpp:5-193), the device buffers, and the two
// max-clique solvers of C++/DPGO/include/DPGO/PCM.h:49-51 written from Pattabiraman et al. 2015 on bit rows.
#include "pcm.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <stdexcept>

namespace dpgo {

#define PCM_HIP(x)                                                                                         \
  do {                                                                                                     \
    hipError_t e_ = (x);                                                                                   \
    if (e_ != hipSuccess) {                                                                                \
      fprintf(stderr, "[dpgo_amd] ERROR: HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
      throw std::runtime_error(hipGetErrorString(e_));                                                     \
    }                                                                                                      \
  } while (0)

int pcm_records(const Graph &g, int alpha, int beta, const double *X, int ld, std::vector<int> &edge_ids,
                std::vector<double> &rec) {
  edge_ids.clear();
  rec.clear();
  if (alpha == beta || alpha < 0 || beta < 0 || alpha >= g.num_nodes || beta >= g.num_nodes) {
    fprintf(stderr, "[dpgo_amd] ERROR: PCM needs two distinct nodes in [0, %d), got %d and %d.\n", g.num_nodes, alpha, beta);
    return -1;
  }
  const int d = g.d, N = g.num_poses;
  if (!X || ld < (d + 1) * N) {
    fprintf(stderr, "[dpgo_amd] ERROR: PCM needs the global X ((d+1)N x d, ld >= %d).\n", (d + 1) * N);
    return -1;
  }
  std::vector<int> node_of(N, -1);
  for (int a = 0; a < g.num_nodes; a++)
    for (const auto &kv : g.g_index[a]) node_of[kv.second] = a;
  const int RT = d * d + d, L = pcm_rec_len(d);
  // pose i of the global X: t_i = row i, R_i(r, c) = X(N + d i + c, r)  (PCM.cpp:128-129, :165-166)
  auto pose = [&](int i, double *R, double *t) {
    for (int c = 0; c < d; c++) {
      t[c] = X[(size_t)c * ld + i];
      for (int r = 0; r < d; r++) R[r * d + c] = X[(size_t)r * ld + N + (size_t)d * i + c];
    }
  };
  // (R, t) as given, and (R^T, -R^T t) computed from the measurement (:115-116, :156-157)
  auto plain = [&](const Measurement &mm, double *R, double *t) {
    for (int k = 0; k < d * d; k++) R[k] = mm.R[k];
    for (int k = 0; k < d; k++) t[k] = mm.t[k];
  };
  auto inverse = [&](const Measurement &mm, double *R, double *t) {
    for (int r = 0; r < d; r++)
      for (int c = 0; c < d; c++) R[r * d + c] = mm.R[c * d + r];
    for (int r = 0; r < d; r++) {
      double s = 0;
      for (int k = 0; k < d; k++) s += mm.R[k * d + r] * mm.t[k];
      t[r] = -s;
    }
  };
  for (size_t e = 0; e < g.all.size(); e++) {
    const Measurement &mm = g.all[e];
    const int ni = node_of[mm.ipose], nj = node_of[mm.jpose];
    const bool fwd = ni == alpha && nj == beta, bwd = ni == beta && nj == alpha;
    if (!fwd && !bwd) continue;
    edge_ids.push_back((int)e);
    rec.resize(rec.size() + L);
    double *r = rec.data() + rec.size() - L;
    pose(fwd ? mm.ipose : mm.jpose, r, r + d * d);             // alpha pose
    pose(fwd ? mm.jpose : mm.ipose, r + RT, r + RT + d * d);   // beta pose
    if (fwd) {
      plain(mm, r + 2 * RT, r + 2 * RT + d * d);     // R_ij, t_ij   (:91-92)
      inverse(mm, r + 3 * RT, r + 3 * RT + d * d);   // R_ji, t_ji   (:156-157)
    } else {
      inverse(mm, r + 2 * RT, r + 2 * RT + d * d);   // (:115-116)
      plain(mm, r + 3 * RT, r + 3 * RT + d * d);     // (:181-182)
    }
    r[4 * RT] = mm.kappa;
    r[4 * RT + 1] = mm.tau;
  }
  return 0;
}

Pcm::Pcm(int dev) : device(dev) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) throw std::runtime_error("PCM: no HIP device");
  if (dev < 0 || dev >= ndev) throw std::runtime_error("PCM: device out of range");
  PCM_HIP(hipSetDevice(device));
  hipStream_t st;
  PCM_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  stream = (void *)st;
}

Pcm::~Pcm() {
  (void)hipSetDevice(device);
  if (rec_dev) (void)hipFree(rec_dev);
  if (bits_dev) (void)hipFree(bits_dev);
  if (err_dev) (void)hipFree(err_dev);
  if (stream) (void)hipStreamDestroy((hipStream_t)stream);
}

template <class T>
static void grow(T *&p, size_t &cap, size_t n) {
  if (n <= cap) return;
  if (p) PCM_HIP(hipFree(p));
  p = nullptr;
  cap = 0;
  PCM_HIP(hipMalloc((void **)&p, n * sizeof(T)));
  cap = n;
}

int Pcm::update(const Graph &g, int alpha, int beta, const double *X, int ld, double tol, bool w) {
  m = 0;
  edge_ids.clear();
  bits.clear();
  if (pcm_records(g, alpha, beta, X, ld, edge_ids, rec) != 0) return -1;
  const int mm = (int)edge_ids.size();
  if (mm > PCM_MAX_M) {
    fprintf(stderr, "[dpgo_amd] ERROR: PCM: %d measurements between nodes %d and %d exceed the limit %d.\n", mm, alpha,
            beta, PCM_MAX_M);
    edge_ids.clear();
    return -1;
  }
  d = g.d;
  tolerance = tol;
  weighted = w;
  m = mm;
  if (m == 0) return 0;
  const size_t W = (size_t)(m + 63) / 64;
  PCM_HIP(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  grow(rec_dev, rec_cap, rec.size());
  grow(bits_dev, bits_cap, (size_t)m * W);
  PCM_HIP(hipMemcpyAsync(rec_dev, rec.data(), rec.size() * sizeof(double), hipMemcpyHostToDevice, st));
  if (pcm_pairs_launch(d, m, rec_dev, tolerance, weighted, bits_dev, nullptr, stream) != 0) return -1;
  bits.resize((size_t)m * W);
  PCM_HIP(hipMemcpyAsync(bits.data(), bits_dev, bits.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  PCM_HIP(hipStreamSynchronize(st));
  return m;
}

int Pcm::errors(double *E) {
  if (!E) return -1;
  if (m > PCM_MAX_M_ERRORS) {
    fprintf(stderr, "[dpgo_amd] ERROR: PCM: the error matrix is a debug output for m <= %d (m = %d).\n", PCM_MAX_M_ERRORS, m);
    return -1;
  }
  if (m == 0) return 0;
  PCM_HIP(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  grow(err_dev, err_cap, (size_t)m * m);
  // the debug variant rewrites the same bit rows (same formula) next to the error matrix
  if (pcm_pairs_launch(d, m, rec_dev, tolerance, weighted, bits_dev, err_dev, stream) != 0) return -1;
  PCM_HIP(hipMemcpyAsync(E, err_dev, (size_t)m * m * sizeof(double), hipMemcpyDeviceToHost, st));
  PCM_HIP(hipStreamSynchronize(st));
  return 0;
}

// ---- max clique on bit rows (Pattabiraman, Patwary, Gebremedhin, Liao, Choudhary 2015) ----------------------------

namespace {

struct BitGraph {
  int m, W;
  const uint64_t *rows;
  std::vector<int> deg;   // degree without the diagonal
  BitGraph(int m_, const uint64_t *r) : m(m_), W((m_ + 63) / 64), rows(r), deg(m_) {
    for (int i = 0; i < m; i++) {
      int c = 0;
      for (int w = 0; w < W; w++) c += __builtin_popcountll(r[(size_t)i * W + w]);
      deg[i] = c - ((r[(size_t)i * W + i / 64] >> (i % 64)) & 1);
    }
  }
  const uint64_t *row(int i) const { return rows + (size_t)i * W; }
  bool adj(int i, int j) const { return (row(i)[j / 64] >> (j % 64)) & 1; }
  // vertices that may still be in a clique larger than `best`: degree >= best
  void eligible(int best, std::vector<uint64_t> &mask) const {
    mask.assign(W, 0);
    for (int i = 0; i < m; i++)
      if (deg[i] >= best) mask[i / 64] |= 1ull << (i % 64);
  }
};

int popcount(const uint64_t *a, int W) {
  int c = 0;
  for (int w = 0; w < W; w++) c += __builtin_popcountll(a[w]);
  return c;
}

}  // namespace

// Algorithm 2 of the paper (MaxCliqueHeu): for every vertex of degree >= best, grow greedily from its eligible
// neighbours, always taking the candidate of highest degree (lowest index among ties), until no candidate is left.
int max_clique_heuristic(int m, const uint64_t *rows, std::vector<uint8_t> &out) {
  out.assign(std::max(m, 0), 0);
  if (m <= 0) return 0;
  BitGraph G(m, rows);
  const int W = G.W;
  std::vector<uint64_t> elig, U(W);
  std::vector<int> cur, best_set;
  int best = 0;
  G.eligible(best, elig);
  for (int i = 0; i < m; i++) {
    if (G.deg[i] < best) continue;
    cur.assign(1, i);
    const uint64_t *ri = G.row(i);
    for (int w = 0; w < W; w++) U[w] = ri[w] & elig[w];
    U[i / 64] &= ~(1ull << (i % 64));
    for (;;) {
      int u = -1;
      for (int w = 0; w < W; w++)
        for (uint64_t b = U[w]; b; b &= b - 1) {
          const int v = w * 64 + __builtin_ctzll(b);
          if (u < 0 || G.deg[v] > G.deg[u]) u = v;
        }
      if (u < 0) break;
      cur.push_back(u);
      const uint64_t *ru = G.row(u);
      for (int w = 0; w < W; w++) U[w] &= ru[w] & elig[w];
      U[u / 64] &= ~(1ull << (u % 64));
    }
    if ((int)cur.size() > best) {
      best = (int)cur.size();
      best_set = cur;
      G.eligible(best, elig);
    }
  }
  for (int v : best_set) out[v] = 1;
  return best;
}

// Algorithm 1 of the paper (MaxClique): branch and bound over the vertices in index order.  Vertex i roots the cliques
// whose smallest member it is (candidates: neighbours j > i); vertices of degree < best are pruned, and a branch ends
// when |clique| + |candidates| <= best.  Candidate sets are AND-ed bit rows, sizes are popcounts; the search is an
// explicit stack (its depth is the clique size, up to m).  The result is the first clique of maximum size the search
// meets, starting from the heuristic's clique as the bound (so among ties it is the heuristic's when that is maximum).
int max_clique_exact(int m, const uint64_t *rows, std::vector<uint8_t> &out) {
  int best = max_clique_heuristic(m, rows, out);
  if (m <= 0) return 0;
  BitGraph G(m, rows);
  const int W = G.W;
  std::vector<uint64_t> elig;
  G.eligible(best, elig);
  std::vector<std::vector<uint64_t>> cand;   // cand[L]: candidates with L members chosen
  std::vector<int> clique;
  std::vector<int> best_set;
  auto level = [&](int L) -> uint64_t * {
    while ((int)cand.size() <= L) cand.emplace_back(W, 0);
    return cand[L].data();
  };
  for (int i = 0; i < m; i++) {
    if (G.deg[i] < best) continue;
    clique.assign(1, i);
    uint64_t *U = level(1);
    const uint64_t *ri = G.row(i);
    for (int w = 0; w < W; w++) {
      // neighbours j > i only
      uint64_t above = w < i / 64 ? 0 : w > i / 64 ? ~0ull : (i % 64 == 63 ? 0 : ~0ull << (i % 64 + 1));
      U[w] = ri[w] & elig[w] & above;
    }
    int L = 1;
    while (L >= 1) {
      uint64_t *C = level(L);
      const int c = popcount(C, W);
      if (c == 0) {
        if (L > best) {
          best = L;
          best_set.assign(clique.begin(), clique.begin() + L);
          G.eligible(best, elig);
        }
        L--;
        continue;
      }
      if (L + c <= best) {
        L--;
        continue;
      }
      int w0 = 0;
      while (!C[w0]) w0++;
      const int u = w0 * 64 + __builtin_ctzll(C[w0]);
      C[w0] &= C[w0] - 1;
      clique.resize(L + 1);
      clique[L] = u;
      uint64_t *N = level(L + 1);
      C = level(L);   // level() may have moved the vectors' storage
      const uint64_t *ru = G.row(u);
      for (int w = 0; w < W; w++) N[w] = C[w] & ru[w] & elig[w];
      L++;
    }
  }
  if (!best_set.empty()) {
    out.assign(m, 0);
    for (int v : best_set) out[v] = 1;
  }
  return best;
}

}  // namespace dpgo
