// Edge evaluation, host side: the edge records (uploaded once), the per-call pose records of X, the read-back.
#include "edges.h"
#include "edge_math.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>

namespace dpgo {

#define EDGE_HIP(x)                                                                                        \
  do {                                                                                                     \
    hipError_t e_ = (x);                                                                                   \
    if (e_ != hipSuccess) {                                                                                \
      fprintf(stderr, "[dpgo_amd] ERROR: HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
      throw std::runtime_error(hipGetErrorString(e_));                                                     \
    }                                                                                                      \
  } while (0)

void edge_inter_flags(const Graph &g, std::vector<uint8_t> &inter) {
  std::vector<int> node_of(g.num_poses, -1);
  for (int a = 0; a < g.num_nodes; a++)
    for (const auto &kv : g.g_index[a]) node_of[kv.second] = a;
  inter.resize(g.all.size());
  for (size_t e = 0; e < g.all.size(); e++) inter[e] = node_of[g.all[e].ipose] != node_of[g.all[e].jpose];
}

void edge_records(const Graph &g, std::vector<double> &rec) {
  const int d = g.d, m = (int)g.all.size();
  std::vector<uint8_t> inter;
  edge_inter_flags(g, inter);
  const int L = edge_rec_doubles(d);
  rec.assign((size_t)m * L, 0.0);
  for (int e = 0; e < m; e++) {
    const Measurement &mm = g.all[e];
    double *r = rec.data() + (size_t)e * L;
    const int head[4] = {mm.ipose, mm.jpose, inter[e] ? 1 : 0, 0};
    std::memcpy(r, head, sizeof(head));
    for (int k = 0; k < d * d; k++) r[2 + k] = mm.R[k];
    for (int k = 0; k < d; k++) r[2 + d * d + k] = mm.t[k];
    r[2 + d * d + d] = mm.kappa;
    r[2 + d * d + d + 1] = mm.tau;
  }
}

// pose p of the global X: t_p = row p, row r of Y_p = row N + d p + r
void pose_records(int d, int N, const double *X, int ld, double *out) {
  const int RS = pose_rec_doubles(d);
  for (int p = 0; p < N; p++) {
    double *o = out + (size_t)p * RS;
    for (int c = 0; c < d; c++) {
      o[c] = X[(size_t)c * ld + p];
      for (int r = 0; r < d; r++) o[d + r * d + c] = X[(size_t)c * ld + N + (size_t)d * p + r];
    }
  }
}

static bool edge_args_ok(int d, int N, const double *X, int ld, int loss, double loss_reg) {
  if (!X || ld < (d + 1) * N) {
    fprintf(stderr, "[dpgo_amd] ERROR: edge evaluation needs the global X ((d+1)N x d, ld >= %d).\n", (d + 1) * N);
    return false;
  }
  if (loss < 0 || loss > 3) {
    fprintf(stderr, "[dpgo_amd] ERROR: edge evaluation: loss %d is not one of 0 (none), 1 (Huber), 2 (GM), 3 (Welsch).\n", loss);
    return false;
  }
  if (loss != 0 && !(std::isfinite(loss_reg) && loss_reg > 0)) {
    fprintf(stderr, "[dpgo_amd] ERROR: edge evaluation: a robust loss needs a finite loss_reg > 0.\n");
    return false;
  }
  return true;
}

static bool edge_graph_ok(const Graph &g) {
  if ((g.d != 2 && g.d != 3) || g.num_poses <= 0 || g.all.empty()) return false;
  for (const Measurement &mm : g.all)
    if (mm.ipose < 0 || mm.ipose >= g.num_poses || mm.jpose < 0 || mm.jpose >= g.num_poses) return false;
  return true;
}

// The device's computation on the host, lane by lane and in the device's order of summation (the shuffle tree of a wave:
// lane l += lane l + o for o = 32 .. 1; the final pass's strided sums): the same edge_lane, the same records.  A debug
// restatement for machines without a GPU -- the host's exp / expm1 and its unfused multiply-adds round differently.
int edge_eval_host(const Graph &g, const double *X, int ld, int loss, double loss_reg, double *s_rot, double *s_trans,
                   double *rho, double *weight, EdgeSummary *sum) {
  if (!edge_graph_ok(g)) return -1;
  const int d = g.d, N = g.num_poses, m = (int)g.all.size();
  if (!edge_args_ok(d, N, X, ld, loss, loss_reg)) return -1;
  std::vector<double> rec, pose((size_t)N * pose_rec_doubles(d));
  edge_records(g, rec);
  pose_records(d, N, X, ld, pose.data());
  const int L = edge_rec_doubles(d), RS = pose_rec_doubles(d), nb = (m + EDGE_BLOCK - 1) / EDGE_BLOCK;
  auto tree = [](double *v, bool is_min) {
    for (int o = 32; o > 0; o >>= 1)
      for (int l = 0; l < 64; l++) {   // (ascending l: lane l reads lane l + o before that lane is overwritten)
        const double other = l + o < 64 ? v[l + o] : v[l];
        v[l] = is_min ? std::fmin(v[l], other) : (l + o < 64 ? v[l] + other : v[l] + v[l]);
      }
    return v[0];
  };
  std::vector<double> part(3 * (size_t)nb);
  std::vector<long long> cnt(2 * (size_t)nb);
  for (int bk = 0; bk < nb; bk++) {
    double fi[64], fe[64], wm[64];
    long long ni = 0, nd = 0;
    for (int l = 0; l < 64; l++) {
      fi[l] = fe[l] = 0;
      wm[l] = INFINITY;
      const int e = bk * EDGE_BLOCK + l;
      if (e >= m) continue;
      const double *q = rec.data() + (size_t)e * L;
      int i, j;
      bool inter;
      edge_head(q, i, j, inter);
      double v[4];
      if (d == 2) edge_lane<2>(q, pose.data() + (size_t)i * RS, pose.data() + (size_t)j * RS, inter, loss, loss_reg, v);
      else edge_lane<3>(q, pose.data() + (size_t)i * RS, pose.data() + (size_t)j * RS, inter, loss, loss_reg, v);
      if (s_rot) s_rot[e] = v[0];
      if (s_trans) s_trans[e] = v[1];
      if (rho) rho[e] = v[2];
      if (weight) weight[e] = v[3];
      (inter ? fe[l] : fi[l]) = v[2];   // (rho = s on an intra edge)
      wm[l] = v[3];
      ni += inter;
      nd += v[3] < 1.0;
    }
    part[bk] = tree(fi, false);
    part[nb + bk] = tree(fe, false);
    part[2 * (size_t)nb + bk] = tree(wm, true);
    cnt[bk] = ni;
    cnt[nb + bk] = nd;
  }
  double fi[64], fe[64], wm[64];
  long long ni = 0, nd = 0;
  for (int l = 0; l < 64; l++) {
    fi[l] = fe[l] = 0;
    wm[l] = INFINITY;
    for (int k = l; k < nb; k += 64) {
      fi[l] += part[k];
      fe[l] += part[nb + k];
      wm[l] = std::fmin(wm[l], part[2 * (size_t)nb + k]);
    }
  }
  for (int k = 0; k < nb; k++) {
    ni += cnt[k];
    nd += cnt[nb + k];
  }
  if (sum) {
    sum->F_intra = 0.5 * tree(fi, false);
    sum->F_inter = 0.5 * tree(fe, false);
    sum->F = sum->F_intra + sum->F_inter;
    sum->weight_min = tree(wm, true);
    sum->num_inter = (int)ni;
    sum->num_downweighted = (int)nd;
  }
  return 0;
}

EdgeEval::EdgeEval(const Graph &g, int dev) : device(dev), d(g.d), N(g.num_poses), m((int)g.all.size()) {
  if (!edge_graph_ok(g)) throw std::runtime_error("edge evaluation: an empty graph, or an edge that names a pose outside it");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) throw std::runtime_error("edge evaluation: no HIP device");
  if (dev < 0 || dev >= ndev) throw std::runtime_error("edge evaluation: device out of range");
  nblk = (m + EDGE_BLOCK - 1) / EDGE_BLOCK;
  std::vector<double> rec;
  edge_records(g, rec);
  EDGE_HIP(hipSetDevice(device));
  try {
    hipStream_t st;
    EDGE_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    stream = (void *)st;
    hipEvent_t a, b;
    EDGE_HIP(hipEventCreate(&a));
    ev0 = (void *)a;
    EDGE_HIP(hipEventCreate(&b));
    ev1 = (void *)b;
    EDGE_HIP(hipMalloc((void **)&rec_dev, rec.size() * sizeof(double)));
    EDGE_HIP(hipMalloc((void **)&pose_dev, (size_t)N * pose_rec_doubles(d) * sizeof(double)));
    EDGE_HIP(hipMalloc((void **)&out_dev, 4 * (size_t)m * sizeof(double)));
    EDGE_HIP(hipMalloc((void **)&part_dev, 3 * (size_t)nblk * sizeof(double)));
    EDGE_HIP(hipMalloc((void **)&cnt_dev, 2 * (size_t)nblk * sizeof(long long)));
    EDGE_HIP(hipMalloc((void **)&sum_dev, sizeof(EdgeSummaryDev)));
    EDGE_HIP(hipMemcpyAsync(rec_dev, rec.data(), rec.size() * sizeof(double), hipMemcpyHostToDevice, st));
    EDGE_HIP(hipStreamSynchronize(st));
  } catch (...) {
    release();
    throw;
  }
  pose_host.resize((size_t)N * pose_rec_doubles(d));
}

EdgeEval::~EdgeEval() { release(); }

void EdgeEval::release() {
  (void)hipSetDevice(device);
  for (void *p : {(void *)rec_dev, (void *)pose_dev, (void *)out_dev, (void *)part_dev, (void *)cnt_dev, (void *)sum_dev})
    if (p) (void)hipFree(p);
  rec_dev = pose_dev = out_dev = part_dev = nullptr;
  cnt_dev = nullptr;
  sum_dev = nullptr;
  if (ev0) (void)hipEventDestroy((hipEvent_t)ev0);
  if (ev1) (void)hipEventDestroy((hipEvent_t)ev1);
  if (stream) (void)hipStreamDestroy((hipStream_t)stream);
  ev0 = ev1 = stream = nullptr;
}

int EdgeEval::run(const double *X, int ld, int loss, double loss_reg, double *s_rot, double *s_trans, double *rho,
                  double *weight, EdgeSummary *sum) {
  if (!edge_args_ok(d, N, X, ld, loss, loss_reg)) return -1;
  pose_records(d, N, X, ld, pose_host.data());
  EDGE_HIP(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  EDGE_HIP(hipMemcpyAsync(pose_dev, pose_host.data(), pose_host.size() * sizeof(double), hipMemcpyHostToDevice, st));
  EDGE_HIP(hipEventRecord((hipEvent_t)ev0, st));
  if (edge_eval_launch(d, m, rec_dev, pose_dev, loss, loss_reg, out_dev, part_dev, cnt_dev, sum_dev, stream) != 0) return -1;
  EDGE_HIP(hipEventRecord((hipEvent_t)ev1, st));
  double *dst[4] = {s_rot, s_trans, rho, weight};
  for (int k = 0; k < 4; k++)
    if (dst[k]) EDGE_HIP(hipMemcpyAsync(dst[k], out_dev + (size_t)k * m, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, st));
  EdgeSummaryDev sd;
  EDGE_HIP(hipMemcpyAsync(&sd, sum_dev, sizeof(sd), hipMemcpyDeviceToHost, st));
  EDGE_HIP(hipStreamSynchronize(st));
  EDGE_HIP(hipEventElapsedTime(&kernel_ms, (hipEvent_t)ev0, (hipEvent_t)ev1));
  if (sum) {
    sum->F_intra = sd.F_intra;
    sum->F_inter = sd.F_inter;
    sum->F = sd.F_intra + sd.F_inter;
    sum->weight_min = sd.weight_min;
    sum->num_inter = (int)sd.num_inter;
    sum->num_downweighted = (int)sd.num_downweighted;
  }
  return 0;
}

}  // namespace dpgo
