// Pairwise consistency maximisation (PCM): outlier rejection for the inter-node loop closures of one pair of
// nodes (alpha, beta) -- C++/DPGO/include/DPGO/PCM.h, C++/DPGO/src/PCM.cpp:5-235.
//
// update() restates PCM::update exactly: the measurement list is the graph's alpha-beta edges in graph edge order
// (either direction), the p / q orientation forms are built as the reference builds them (:91-92, :115-116,
// :156-157, :181-182), and the pair error is the reference's cycle composition (:194-230) in fp64 on the device.
// The m x m consistency matrix is kept as bit rows, ceil(m/64) uint64 words per row, row-major.
//
// Stated deviations from the reference:
//  - alpha == beta, or a node out of range, returns -1 (the reference would run on alpha's intra-node edges);
//  - nothing calls exit(): errors are -1 plus a line on stderr;
//  - X is the global iterate ((d+1)N x d, column-major, R_i(r, c) = X(N + d i + c, r)), not the reference's
//    two-node stacked X with index / num_s offsets -- both pick the same poses;
//  - rounding is not Eigen's, so only the decisions away from the tolerance are promised to match.
//
// The max-clique solvers (Pattabiraman et al. 2015, cited at C++/PCM/include/PCM/PCM.hpp:29-66) are written here
// from the paper, on the bit rows, on the host.
#pragma once
#include <cstdint>
#include <vector>

#include "graph.h"

namespace dpgo {

// Per-measurement record of one pair, in doubles: the alpha pose (R row-major d x d, t), the beta pose, the
// first-role form (R_ij, t_ij), the second-role form (R_ji, t_ji), kappa, tau.
constexpr int pcm_rec_len(int d) { return 4 * (d * d + d) + 2; }
constexpr int PCM_MAX_M = 65536;       // bit words m * ceil(m/64) * 8 bytes = 512 MiB at the cap
constexpr int PCM_MAX_M_ERRORS = 4096; // the debug fp64 error matrix

// Host: the alpha-beta measurements of g (edge ids in graph order) and their records.  -1 on bad arguments.
int pcm_records(const Graph &g, int alpha, int beta, const double *X, int ld, std::vector<int> &edge_ids,
                std::vector<double> &rec);

// Device (pcm.hip): the full symmetric bit matrix (words = m * ceil(m/64)) and, when err != nullptr, the m x m fp64
// error matrix, from the records already on the device.  Enqueued on `stream`.
int pcm_pairs_launch(int d, int m, const double *rec, double tol, bool weighted, uint64_t *bits, double *err,
                     void *stream);

// Host max clique on bit rows (W = ceil(m/64) words per row, diagonal set).  out[i] = 1 for the members.
// Returns the clique size.
int max_clique_exact(int m, const uint64_t *rows, std::vector<uint8_t> &out);
int max_clique_heuristic(int m, const uint64_t *rows, std::vector<uint8_t> &out);

// One PCM object of the C ABI: device buffers and the last update's results.
struct Pcm {
  int device = 0;
  int d = 0, m = 0;
  double tolerance = 0.2;
  bool weighted = false;
  std::vector<int> edge_ids;
  std::vector<double> rec;
  std::vector<uint64_t> bits;   // host copy of the bit rows
  double *rec_dev = nullptr;
  uint64_t *bits_dev = nullptr;
  double *err_dev = nullptr;
  size_t rec_cap = 0, bits_cap = 0, err_cap = 0;
  void *stream = nullptr;

  explicit Pcm(int device);
  ~Pcm();
  int update(const Graph &g, int alpha, int beta, const double *X, int ld, double tol, bool weighted);
  int errors(double *E);
};

}  // namespace dpgo
