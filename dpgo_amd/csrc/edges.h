// Per-edge residuals, loss values and loss weights of a whole graph at a global X, on the device.
//
// What k_inter computes for a node's inter-node edges inside every iteration (DPGOProblem::evaluate_E,
// C++/DPGO/src/DPGOProblem.cpp:634-681), restated for ALL edges of the graph in graph (file) order and returned to the
// caller.  X in the reference layout, t_p = row p, Y_p = R_p^T = rows N + d p ..:
//   s_rot_e   = kappa_e |Y_j - R_e^T Y_i|_F^2
//   s_trans_e = tau_e |t_j - t_i - t_e^T Y_i|^2
//   s_e       = s_rot_e + s_trans_e                      (= |(B X)_e|^2 of construct_data_matrix's residual rows)
// An edge is INTER when its endpoints lie in different nodes of the graph's partition.  Intra edges and the trivial loss:
// rho = s, w = 1.  Inter edges: the formulas of DPGOProblem.cpp:651-670 with delta = loss_reg.
//   F = 1/2 sum_intra s_e + 1/2 sum_inter rho_e          (DPGOStar::evaluate_f, DPGOStar.cpp:713-761)
//
// A stand-alone object, as PCM is: no group is needed, and it works for any partition.
#pragma once
#include <cstdint>
#include <vector>

#include "graph.h"

namespace dpgo {

// Edge record on the device, in 16-byte units (double2): unit 0 holds the ints i, j, inter, 0; then R (row-major d x d),
// t, kappa, tau as doubles.  d = 3: 16 + 14 * 8 = 128 bytes; d = 2: 16 + 8 * 8 = 80 bytes.
constexpr int edge_rec_doubles(int d) { return 2 + d * d + d + 2; }
// Pose record of X: [t (d) | rows of Y_p (d x d)], (d + 1) d doubles (96 / 48 bytes: whole 16-byte units).
constexpr int pose_rec_doubles(int d) { return (d + 1) * d; }
constexpr int EDGE_BLOCK = 64;   // one wave per workgroup: the workgroup's partial needs no LDS

// What the final pass leaves on the device (40 bytes).
struct EdgeSummaryDev {
  double F_intra, F_inter, weight_min;
  long long num_inter, num_downweighted;
};

struct EdgeSummary {
  double F = 0, F_intra = 0, F_inter = 0, weight_min = 1;
  int num_inter = 0, num_downweighted = 0;
};

// Device (edges.hip): k_edge_eval<D> over m edges, then the fixed-order final pass over its ceil(m / 64) partials.
// out: 4 arrays of m doubles one after the other (s_rot, s_trans, rho, weight).  Enqueued on `stream`.
int edge_eval_launch(int d, int m, const double *rec, const double *poses, int loss, double loss_reg, double *out,
                     double *partials, long long *counts, EdgeSummaryDev *summary, void *stream);

// Host: the inter flag of every edge of g (graph order); the edge records as the device reads them; the pose records of X.
void edge_inter_flags(const Graph &g, std::vector<uint8_t> &inter);
void edge_records(const Graph &g, std::vector<double> &rec);
void pose_records(int d, int N, const double *X, int ld, double *out);
// Host, debug: the kernel's computation lane by lane in the device's order of summation, from the same records through the
// same edge_lane (edge_math.h).  No GPU needed.  Output pointers may be null.
int edge_eval_host(const Graph &g, const double *X, int ld, int loss, double loss_reg, double *s_rot, double *s_trans,
                   double *rho, double *weight, EdgeSummary *sum);

struct EdgeEval {
  int device = 0;
  int d = 0, N = 0, m = 0, nblk = 0;
  double *rec_dev = nullptr, *pose_dev = nullptr, *out_dev = nullptr, *part_dev = nullptr;
  long long *cnt_dev = nullptr;
  EdgeSummaryDev *sum_dev = nullptr;
  std::vector<double> pose_host;
  void *stream = nullptr;

  EdgeEval(const Graph &g, int device);
  ~EdgeEval();
  void release();
  EdgeEval(const EdgeEval &) = delete;
  EdgeEval &operator=(const EdgeEval &) = delete;
  void *ev0 = nullptr, *ev1 = nullptr;
  float kernel_ms = 0;   // the last run's two launches, between two HIP events on the stream

  // any of the four output pointers may be null; sum may be null
  int run(const double *X, int ld, int loss, double loss_reg, double *s_rot, double *s_trans, double *rho, double *weight,
          EdgeSummary *sum);
};

}  // namespace dpgo
