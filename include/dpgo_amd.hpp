// dpgo_amd.hpp -- header-only C++ facade over the C ABI (dpgo_amd.h) with the reference's names.
//
// What a C++ caller of MurpheyLab/DPGO sees, minus Eigen: DPGO::Matrix is a small column-major
// owner of doubles (the layout Eigen::MatrixXd has by default), everything else keeps the
// reference's spelling and meaning:
//
//   reference (C++/DPGO/include/DPGO)                  here (namespace DPGO)
//   -------------------------------------------------  ----------------------------------------------
//   read_g2o(...)                  DPGO_utils.h:49-51   Graph::read_g2o(filename, num_nodes)
//   Options                        DPGO_types.h:78-201  Options (same field names, same defaults)
//   DPGOResult (scalars, Xk, Xak)  DPGO_types.h:204-322 DPGOResult
//   DPGOHash(node, meas, options)  DPGOHash.h:13-107    DPGOHash  = one node of a DPGOHashGroup
//     initialize / update / iterate / communicate / receive / results / options
//   vector<shared_ptr<DPGOHash>>   dist_pgo.cpp:96      DPGOHashGroup (the nodes one GPU hosts; batched calls)
//   DPGOStar                       DPGOStar.h:13-61     DPGOStar (AMM-PGO*, all nodes in one group)
//   PCM (outlier rejection)        PCM.h:10-71          PCM: update(alpha, beta, graph, global X, opts) instead of
//                                                       (measurements, num_n, num_s, index, X); measurements() are
//                                                       edge indices of the graph
//
// Return codes follow the reference: 0 ok, -1 error (a line on stderr).  Constructors throw
// std::runtime_error (there is no CPU fallback: no HIP device => no group).
#ifndef DPGO_AMD_HPP
#define DPGO_AMD_HPP

#include <algorithm>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "dpgo_amd.h"

namespace DPGO {

using Scalar = double;

// column-major dense matrix (Eigen::MatrixXd layout)
class Matrix {
 public:
  Matrix() = default;
  Matrix(int rows, int cols) : rows_(rows), cols_(cols), v_((size_t)rows * cols, 0.0) {}
  int rows() const { return rows_; }
  int cols() const { return cols_; }
  Scalar *data() { return v_.data(); }
  const Scalar *data() const { return v_.data(); }
  Scalar &operator()(int r, int c) { return v_[(size_t)c * rows_ + r]; }
  Scalar operator()(int r, int c) const { return v_[(size_t)c * rows_ + r]; }
  void resize(int rows, int cols) { rows_ = rows; cols_ = cols; v_.assign((size_t)rows * cols, 0.0); }

 private:
  int rows_ = 0, cols_ = 0;
  std::vector<Scalar> v_;
};

enum class Scheme { MM = 0, AMM = 1 };                                       // DPGO_types.h:52
enum class Loss { None = 0, Huber = 1, GemanMcClure = 2, Welsch = 3 };       // DPGO_types.h:54
enum class Preconditioner { None = 0, Jacobi = 1, IncompleteCholesky = 2, RegularizedCholesky = 3 };   // DPGO_types.h:35-40
enum class Rescale { Static = 0, Dynamic = 1 };                              // DPGO_types.h:43-46

// entry of DPGOProblem::index() / sent() / recv() (DPGOProblem.h:212-225): (node, pose) -> {block, k}
struct IndexEntry {
  int node, pose, block, k;
};

// DPGO::Options (DPGO_types.h:78-201): the C struct with the reference's field names
struct Options : dpgo_options_t {
  Options() { dpgo_options_default(this); }
  // the overrides of C++/examples/dist_pgo.cpp:103-120
  static Options driver(Loss loss = Loss::None, bool accelerated = true) {
    Options o;
    dpgo_options_driver(&o, (int)loss, accelerated ? 1 : 0);
    return o;
  }
};

// the partitioned measurements of read_g2o + generate_data_info (host only)
class Graph {
 public:
  static std::shared_ptr<Graph> read_g2o(const std::string &filename, int num_nodes) {
    dpgo_graph_t *h = nullptr;
    if (dpgo_read_g2o(filename.c_str(), num_nodes, &h) != 0) throw std::runtime_error("DPGO::read_g2o: " + filename);
    return std::shared_ptr<Graph>(new Graph(h));
  }
  ~Graph() { dpgo_graph_free(h_); }
  Graph(const Graph &) = delete;
  Graph &operator=(const Graph &) = delete;
  int d() const { return d_; }
  int num_poses() const { return num_poses_; }
  int num_nodes() const { return num_nodes_; }
  int num_edges() const { return num_edges_; }
  // DPGOProblem::n() / m() (DPGOProblem.h:241-248): {own, neighbour} poses, {intra, inter} edges
  void sizes(int node, int n[2], int m[2]) const { dpgo_graph_node_sizes(h_, node, &n[0], &n[1], &m[0], &m[1]); }
  int offset(int node) const { return dpgo_graph_node_offset(h_, node); }   // first global pose id of the node
  // DPGOProblem::index() / sent() / recv() of a node (DPGOProblem.h:212-225), entries in map order
  std::vector<IndexEntry> index(int node) const { return maps(node, 0); }
  std::vector<IndexEntry> sent(int node) const { return maps(node, 1); }
  std::vector<IndexEntry> recv(int node) const { return maps(node, 2); }
  // g2o export: VERTEX_* lines from X ((d+1) N x d) + the EDGE_* lines
  int write_g2o(const std::string &filename, const Matrix &X) const {
    return dpgo_write_g2o(h_, X.data(), X.rows(), filename.c_str());
  }
  // centralised chordal initialisation (dist_pgo.cpp:416-444): X is (d+1) N x d
  Matrix chordal_initialization() const {
    Matrix X((d_ + 1) * num_poses_, d_);
    if (dpgo_chordal_initialization(h_, X.data(), X.rows()) != 0) throw std::runtime_error("chordal_initialization");
    return X;
  }
  // dpgo_graph_scale_edges: the same poses, partition, R, t and edge order with kappa_e, tau_e multiplied by w[e] >= 0 (the
  // graph of the re-weighted problem; w[e] = 0 keeps the edge with zero values).  Throws on a bad weight or a wrong length.
  std::shared_ptr<Graph> scale_edges(const std::vector<Scalar> &w) const {
    dpgo_graph_t *h = nullptr;
    if ((int)w.size() != num_edges_ || dpgo_graph_scale_edges(h_, w.data(), &h) != 0)
      throw std::runtime_error("DPGO::Graph::scale_edges: one finite weight >= 0 per edge");
    return std::shared_ptr<Graph>(new Graph(h));
  }
  const dpgo_graph_t *handle() const { return h_; }

 private:
  explicit Graph(dpgo_graph_t *h) : h_(h) { dpgo_graph_info(h_, &d_, &num_poses_, &num_nodes_, &num_edges_); }
  std::vector<IndexEntry> maps(int node, int which) const {
    int cnt = 0;
    if (dpgo_graph_node_maps(h_, node, which, nullptr, nullptr, nullptr, nullptr, &cnt) != 0) return {};
    std::vector<int> a(cnt), b(cnt), c(cnt), d(cnt);
    dpgo_graph_node_maps(h_, node, which, a.data(), b.data(), c.data(), d.data(), &cnt);
    std::vector<IndexEntry> out(cnt);
    for (int i = 0; i < cnt; i++) out[i] = {a[i], b[i], c[i], d[i]};
    return out;
  }
  dpgo_graph_t *h_;
  int d_ = 0, num_poses_ = 0, num_nodes_ = 0, num_edges_ = 0;
};

// scalar part of DPGOResult + on-demand copies of Xk / Xak (DPGO_types.h:204-322)
struct DPGOResult : dpgo_results_t {
  Matrix Xk, Xak;
};

class DPGOHashGroup;

// One node: the reference's DPGOHash interface (DPGOHash.h:13-107) on top of its group.
class DPGOHash {
 public:
  int node() const;
  int initialize(const Matrix &X) const;             // (d+1)(n0+n1) x d            DPGOHash.cpp:20-43
  int update() const;                                //                               :84-228
  int iterate() const;                               //                               :583-628
  // message from neighbour node beta: ((d+1) |recv[beta]|) x d, [t rows ; R rows]    :45-82
  int receive(int beta, const Matrix &msg) const;
  Matrix send(int beta) const;                       // what this node owes beta (sent[beta], DPGO_utils.cpp:428-435)
  DPGOResult results(bool with_X = true) const;      // results().Xk is what peers and the driver read
  const Options &options() const;

 private:
  friend class DPGOHashGroup;
  DPGOHash(DPGOHashGroup *g, int local) : g_(g), local_(local) {}
  DPGOHashGroup *g_;
  int local_;
};

// The nodes hosted by one GPU.  Batched update()/iterate()/communicate() replace the driver's loops over
// alpha (dist_pgo.cpp:455-462, 496-521); operator[] gives the per-node view.
class DPGOHashGroup {
 public:
  DPGOHashGroup(std::shared_ptr<Graph> graph, const std::vector<int> &nodes, const Options &options, int device = 0)
      : graph_(std::move(graph)), nodes_(nodes), options_(options) {
    if (dpgo_group_create(graph_->handle(), nodes_.data(), (int)nodes_.size(), &options_, device, &h_) != 0)
      throw std::runtime_error("dpgo_group_create failed (no HIP device, or inconsistent input); there is no CPU path");
    for (int k = 0; k < (int)nodes_.size(); k++) hash_.push_back(DPGOHash(this, k));
  }
  ~DPGOHashGroup() { dpgo_group_free(h_); }
  DPGOHashGroup(const DPGOHashGroup &) = delete;
  DPGOHashGroup &operator=(const DPGOHashGroup &) = delete;

  size_t size() const { return nodes_.size(); }
  const DPGOHash &operator[](int local) const { return hash_[local]; }
  // split a global X over the nodes and fill the neighbour rows (dist_pgo.cpp:435-446 + DPGO::communicate)
  int initialize(const Matrix &X) { return dpgo_group_initialize_global(h_, X.data(), X.rows()); }
  int update() { return dpgo_group_update(h_, nullptr, 0); }
  int iterate() { return dpgo_group_iterate(h_, nullptr, 0); }
  int communicate() { return dpgo_group_communicate_local(h_); }   // neighbours hosted by this group
  // gather X^alpha into the global X (dist_pgo.cpp:502-511)
  int gather(Matrix &X) const { return dpgo_group_scatter_global(h_, X.data(), X.rows()); }
  const Options &options() const { return options_; }
  // DPGOHash::set_options (DPGOHash.h:93-96) for every node of the group
  int set_options(const Options &o) {
    if (dpgo_group_set_options(h_, &o) != 0) return -1;
    options_ = o;
    return 0;
  }
  // DPGOStar::evaluate_f / evaluate_grad at an arbitrary global X (DPGOStar.cpp:713-829), summed over this group
  int evaluate_f(const Matrix &X, Scalar &fobj) const { return dpgo_group_evaluate(h_, X.data(), X.rows(), &fobj, nullptr, nullptr, 0); }
  int evaluate_grad(const Matrix &X, Matrix &grad) const {
    grad.resize(X.rows(), X.cols());
    return dpgo_group_evaluate(h_, X.data(), X.rows(), nullptr, nullptr, grad.data(), grad.rows());
  }
  // SESyncProblem::verify_solution (C++/SESync/include/SESync/SESyncProblem.h:345, SESyncProblem.cpp:397-468) without its
  // block-size and ILDL arguments: LOBPCG on the certificate matrix S = M - Lambda(X), block size d, block-Jacobi
  // preconditioner (dpgo_group_certify).  theta: x' S x of the returned unit vector x ((d+1)N x 1); num_iters: LOBPCG
  // iterations.  Returns true when the search converged with theta >= -eta / 2 (DPGO_CERT_NONNEGATIVE) -- evidence, NOT
  // proof, that X is a global minimiser: a converged Ritz pair need not be the smallest; the proof (a Cholesky
  // factorisation of S + eta I) is fast_verification below.  status (optional): the DPGO_CERT_* outcome, -1
  // when the call itself failed (robust loss, a group that does not host every node).
  bool verify_solution(const Matrix &X, Scalar eta, Scalar &theta, Matrix &x, int &num_iters, int *status = nullptr,
                       dpgo_cert_result_t *result = nullptr) const {
    dpgo_cert_options_t o;
    dpgo_cert_options_default(&o);
    o.eta = eta;
    dpgo_cert_result_t r;
    x.resize(X.rows(), 1);
    const int rc = dpgo_group_certify(h_, X.data(), X.rows(), &o, nullptr, 0, &r, x.data(), x.rows());
    theta = r.theta;
    num_iters = r.iterations;
    if (status) *status = rc == 0 ? r.status : -1;
    if (result) *result = r;
    return rc == 0 && r.status == DPGO_CERT_NONNEGATIVE;
  }
  // fast_verification (C++/SESync/src/SESync_utils.cpp:721-830) without its ILDL arguments: STEP 1, the Cholesky
  // factorisation of S + eta I on the device, and the LOBPCG search of verify_solution only when it did not succeed
  // (dpgo_group_verify).  Returns true when the factorisation PROVED lambda_min(S) > -eta (DPGO_CERT_PROVEN; theta, x and
  // num_iters are then 0 / untouched) -- which says "global minimiser" only where result->stationarity is small.
  // max_factor_bytes > 0 caps the device memory of the factorisation (beyond it STEP 1 is skipped and the answer is
  // verify_solution's).  status: the DPGO_CERT_* outcome, -1 when the call itself failed.
  bool fast_verification(const Matrix &X, Scalar eta, Scalar &theta, Matrix &x, int &num_iters, int *status = nullptr,
                         dpgo_cert_result_t *result = nullptr, dpgo_cert_factor_t *factor = nullptr,
                         long long max_factor_bytes = 0) const {
    dpgo_cert_options_t o;
    dpgo_cert_options_default(&o);
    o.eta = eta;
    dpgo_cert_result_t r = {};
    dpgo_cert_factor_t f = {};
    x.resize(X.rows(), 1);
    const int rc = dpgo_group_verify(h_, X.data(), X.rows(), &o, max_factor_bytes, nullptr, 0, &r, x.data(), x.rows(), &f);
    theta = r.theta;
    num_iters = r.iterations;
    if (status) *status = rc == 0 ? r.status : -1;
    if (result) *result = r;
    if (factor) *factor = f;
    return rc == 0 && r.status == DPGO_CERT_PROVEN;
  }
  // Marginal pose covariances at X relative to the pose `anchor` (dpgo_group_covariance).  marginals is resized to
  // N dof dof doubles: block p, row-major, is Sigma_pp in tangent coordinates (translation in the world frame, then rotation
  // in the body frame; dof = d + d (d - 1) / 2).  pairs / cross (optional): 2 npairs global poses, each an edge of the
  // graph, and their blocks Sigma_pq (npairs dof dof doubles).  Returns true for DPGO_COV_OK; result (optional) carries the
  // outcome (NOT_PD, SKIPPED: the blocks are zero) and the sizes; status: the DPGO_COV_* outcome, -1 when the call itself
  // failed (robust loss, a group that does not host every node, a pair that is not an edge).
  bool marginal_covariances(const Matrix &X, std::vector<Scalar> &marginals, int anchor = 0, dpgo_cov_result_t *result = nullptr,
                            int *status = nullptr, const std::vector<int> *pairs = nullptr, std::vector<Scalar> *cross = nullptr,
                            long long max_bytes = 0) const {
    const int d = graph_->d(), N = graph_->num_poses();
    const int dof = d + d * (d - 1) / 2, npairs = pairs && cross ? (int)pairs->size() / 2 : 0;
    marginals.assign((size_t)N * dof * dof, 0.0);
    if (cross) cross->assign((size_t)npairs * dof * dof, 0.0);
    dpgo_cov_result_t r = {};
    const int rc = dpgo_group_covariance(h_, X.data(), X.rows(), anchor, max_bytes, npairs ? pairs->data() : nullptr, npairs,
                                         marginals.data(), npairs ? cross->data() : nullptr, &r);
    if (status) *status = rc == 0 ? r.outcome : -1;
    if (result) *result = r;
    return rc == 0 && r.outcome == DPGO_COV_OK;
  }
  // Joint covariances of arbitrary pose pairs and the loop-closure gate (dpgo_group_pair_covariance).  pairs: 2 npairs global
  // poses, any two (no edge needed).  joint is resized to npairs 3 dof dof doubles (Sigma_pp, Sigma_pq with the rows of p and
  // the columns of q, Sigma_qq), rel to npairs dof dof (the covariance of T_p^-1 T_q).  candidates / gate (optional, both or
  // neither): npairs (d d + d + 2) doubles R~ row-major, t~, kappa, tau, and npairs (2 + dof) doubles d^2, not_pd, the
  // residual.  Returns true for DPGO_PAIRS_OK; status: the DPGO_PAIRS_* outcome, -1 when the call itself failed.
  bool pair_covariances(const Matrix &X, const std::vector<int> &pairs, std::vector<Scalar> &joint, std::vector<Scalar> &rel,
                        int anchor = 0, dpgo_pairs_result_t *result = nullptr, int *status = nullptr,
                        const std::vector<Scalar> *candidates = nullptr, std::vector<Scalar> *gate = nullptr,
                        long long max_bytes = 0) const {
    const int d = graph_->d(), npairs = (int)pairs.size() / 2;
    const int dof = d + d * (d - 1) / 2;
    joint.assign((size_t)npairs * 3 * dof * dof, 0.0);
    rel.assign((size_t)npairs * dof * dof, 0.0);
    const bool gated = candidates && gate && candidates->size() == (size_t)npairs * (d * d + d + 2);
    if (gate) gate->assign(gated ? (size_t)npairs * (2 + dof) : 0, 0.0);
    dpgo_pairs_result_t r = {};
    const int rc = candidates && !gated ? -1
                                        : dpgo_group_pair_covariance(h_, X.data(), X.rows(), anchor, max_bytes, pairs.data(), npairs,
                                                                     gated ? candidates->data() : nullptr, joint.data(), rel.data(),
                                                                     gated ? gate->data() : nullptr, &r);
    if (status) *status = rc == 0 ? r.outcome : -1;
    if (result) *result = r;
    return rc == 0 && r.outcome == DPGO_PAIRS_OK;
  }
  // The joint marginal of a SET of poses (dpgo_group_joint_marginal).  keep: distinct global poses in any order; the outputs
  // follow that order.  base < 0: the absolute form, cov = (H^-1)_KK, n = dof K (the anchor may not be kept); base a member of
  // keep: the covariance of T_base^-1 T_k of the others, n = dof (K - 1).  cov is resized to n n doubles (row-major, symmetric
  // bit for bit); info (optional) to n n: cov^-1, and then *logdet (optional) = log det cov.  X should be a critical point
  // (newton_polish).  Returns true for DPGO_MARG_OK; status: the DPGO_MARG_* outcome, -1 when the call itself failed (a pose
  // outside the graph or kept twice, the anchor kept without a base, a base that is not one of at least two kept poses).
  bool joint_marginal(const Matrix &X, const std::vector<int> &keep, std::vector<Scalar> &cov, std::vector<Scalar> *info = nullptr,
                      Scalar *logdet = nullptr, int anchor = 0, int base = -1, dpgo_marg_result_t *result = nullptr,
                      int *status = nullptr, long long max_bytes = 0) const {
    const int d = graph_->d(), dof = d + d * (d - 1) / 2, K = (int)keep.size();
    const size_t n = (size_t)dof * (size_t)std::max(K - (base >= 0 ? 1 : 0), 0);
    cov.assign(n * n, 0.0);
    if (info) info->assign(n * n, 0.0);
    Scalar ld = 0.0;
    dpgo_marg_result_t r = {};
    const int rc = K < 1 || n < 1 ? -1
                                  : dpgo_group_joint_marginal(h_, X.data(), X.rows(), keep.data(), K, anchor, base, info ? 1 : 0, max_bytes,
                                                              cov.data(), info ? info->data() : nullptr, &ld, &r);
    if (logdet) *logdet = ld;
    if (status) *status = rc == 0 ? r.outcome : -1;
    if (result) *result = r;
    return rc == 0 && r.outcome == DPGO_MARG_OK;
  }
  // Joint compatibility and budgeted selection of loop-closure candidates (dpgo_group_candidate_set).  pairs: 2 m global poses,
  // p != q; candidates: m (d^2 + d + 2) doubles, R~, t~, kappa, tau as for pair_covariances.  S is resized to n n doubles,
  // n = dof m: the joint innovation covariance; residual to n; info (optional) to n n: S^-1, and then scalars[0..2] = log det S,
  // d2_joint, gain_all; selected to the chosen candidates in order (at most budget of them, by conditional information gain,
  // gated by d2_max > 0 on the conditional d2), steps to 4 doubles per choice: index, gain, d2, eligible; scalars[3..4] =
  // gain_selected, d2_selected.  X should be a critical point (newton_polish).  Returns true for DPGO_CAND_OK; status: the
  // DPGO_CAND_* outcome, -1 when the call itself failed (a pose outside the graph, p == q, a weight that is not positive).
  bool candidate_set(const Matrix &X, const std::vector<int> &pairs, const std::vector<Scalar> &candidates, int budget,
                     std::vector<Scalar> &S, std::vector<Scalar> &residual, std::vector<int> &selected, std::vector<Scalar> &steps,
                     Scalar scalars[5], std::vector<Scalar> *info = nullptr, Scalar d2_max = 0.0, int anchor = 0,
                     dpgo_cand_result_t *result = nullptr, int *status = nullptr, long long max_bytes = 0) const {
    const int d = graph_->d(), dof = d + d * (d - 1) / 2, m = (int)pairs.size() / 2;
    const size_t n = (size_t)dof * (size_t)m, nb = (size_t)std::max(budget, 1);
    S.assign(n * n, 0.0);
    residual.assign(n, 0.0);
    if (info) info->assign(n * n, 0.0);
    selected.assign(nb, -1);
    steps.assign(4 * nb, 0.0);
    std::vector<int> poses(2 * (size_t)std::max(m, 1));
    for (int k = 0; k < 5; k++) scalars[k] = 0.0;
    dpgo_cand_result_t r = {};
    const bool sized = m >= 1 && budget >= 0 && candidates.size() == (size_t)m * (size_t)(d * d + d + 2);
    const int rc = !sized ? -1
                          : dpgo_group_candidate_set(h_, X.data(), X.rows(), pairs.data(), m, candidates.data(), anchor, budget, d2_max,
                                                     info ? 1 : 0, max_bytes, nullptr, S.data(), residual.data(),
                                                     info ? info->data() : nullptr, scalars, selected.data(), steps.data(),
                                                     poses.data(), &r);
    selected.resize(rc == 0 ? (size_t)r.n_selected : 0);
    steps.resize(4 * selected.size());
    if (status) *status = rc == 0 ? r.outcome : -1;
    if (result) *result = r;
    return rc == 0 && r.outcome == DPGO_CAND_OK;
  }
  // Measurement sensitivities by implicit differentiation (dpgo_group_sensitivity): upstream holds k tangent gradients of
  // scalars L_l(X), (dof N) x k column-major by global pose in marginal_covariances' coordinates; sens is resized to
  // k num_edges (2 + dof) doubles, [l][e][d/dkappa, d/dtau, d/dt~, d/deta] with the edges in the graph's order; adjoint
  // (optional) to (dof N) k: lambda_l = H^-1 c_l, zeros on the anchor.  X should be a critical point (newton_polish).  Returns
  // true for DPGO_SENS_OK; status: the DPGO_SENS_* outcome, -1 when the call itself failed (robust loss, a group that does not
  // host every node, an upstream of the wrong size or with an entry that is not finite).
  bool measurement_sensitivities(const Matrix &X, const std::vector<Scalar> &upstream, std::vector<Scalar> &sens, int anchor = 0,
                                 dpgo_sens_result_t *result = nullptr, int *status = nullptr, std::vector<Scalar> *adjoint = nullptr,
                                 long long max_bytes = 0) const {
    const int d = graph_->d(), dof = d + d * (d - 1) / 2, m = graph_->num_edges();
    const size_t n = (size_t)dof * graph_->num_poses();
    const int k = n ? (int)(upstream.size() / n) : 0;
    const bool sized = k >= 1 && upstream.size() == n * (size_t)k;
    sens.assign(sized ? (size_t)k * m * (2 + dof) : 0, 0.0);
    if (adjoint) adjoint->assign(sized ? n * (size_t)k : 0, 0.0);
    dpgo_sens_result_t r = {};
    const int rc = !sized ? -1
                          : dpgo_group_sensitivity(h_, graph_->handle(), X.data(), X.rows(), anchor, max_bytes, upstream.data(), (int)n, k,
                                                   adjoint ? adjoint->data() : nullptr, sens.data(), &r);
    if (status) *status = rc == 0 ? r.outcome : -1;
    if (result) *result = r;
    return rc == 0 && r.outcome == DPGO_SENS_OK;
  }
  // Per-edge reliability (dpgo_group_edge_reliability): for every edge of the graph, or for the listed indices into its edges
  // (any order, repeats allowed; null: all), one record of 6 + 2 dof doubles -- d2_loo, flag, redundancy, redundancy_trans,
  // d2_own, influence, r[dof], r_loo[dof] -- the leave-one-out chi-square of an edge that is already in the graph, the residual
  // it would have without it, and how well the other measurements check it.  method: DPGO_RELY_AUTO / SELINV / SOLVE.  X
  // should be a critical point (newton_polish).  Returns true for DPGO_RELY_OK; status: the DPGO_RELY_* outcome, -1 when the
  // call itself failed (robust loss, a group that does not host every node, an edge index outside the graph, an unknown method).
  bool edge_reliability(const Matrix &X, std::vector<Scalar> &records, int anchor = 0, dpgo_rely_result_t *result = nullptr,
                        int *status = nullptr, const std::vector<int> *edges = nullptr, int method = DPGO_RELY_AUTO,
                        long long max_bytes = 0, std::vector<Scalar> *rel = nullptr, std::vector<Scalar> *joint = nullptr) const {
    const int d = graph_->d(), dof = d + d * (d - 1) / 2;
    const size_t n = edges ? edges->size() : (size_t)graph_->num_edges();
    records.assign(n * (6 + 2 * dof), 0.0);
    if (rel) rel->assign(n * dof * dof, 0.0);
    if (joint) joint->assign(n * 3 * dof * dof, 0.0);
    const int none = 0;   // (an empty list is a list: neither its pointer nor that of its records may be null)
    Scalar no_record = 0;
    dpgo_rely_result_t r = {};
    const int rc = dpgo_group_edge_reliability(h_, graph_->handle(), X.data(), X.rows(), anchor, max_bytes, method,
                                               edges ? (edges->empty() ? &none : edges->data()) : nullptr, edges ? (int)edges->size() : 0,
                                               records.empty() ? &no_record : records.data(),
                                               rel ? rel->data() : nullptr, joint ? joint->data() : nullptr, &r);
    if (status) *status = rc == 0 ? r.outcome : -1;
    if (result) *result = r;
    return rc == 0 && r.outcome == DPGO_RELY_OK;
  }
  // Newton polish (dpgo_group_polish): damped Riemannian Newton steps from X on the anchored tangent-space Hessian of
  // marginal_covariances, until the tangent gradient is at rounding level or the step budget is spent.  Xout: the new point
  // (X itself when the call is SKIPPED or fails).  opt (optional): the rule's parameters and the anchor; log (optional): per
  // iteration F0, |g|, mu at entry, rho of the accepted try, tries.  Returns true for DPGO_POLISH_CONVERGED; status: the
  // DPGO_POLISH_* outcome, -1 when the call itself failed (robust loss, a group that does not host every node, a bad anchor).
  bool newton_polish(const Matrix &X, Matrix &Xout, dpgo_polish_result_t *result = nullptr, int *status = nullptr,
                     const dpgo_polish_options_t *opt = nullptr, long long max_bytes = 0, std::vector<Scalar> *log = nullptr) const {
    dpgo_polish_options_t o;
    dpgo_polish_options_default(&o);
    if (opt) o = *opt;
    Xout = X;
    const int cap = o.max_steps >= 0 ? o.max_steps + 1 : 0;
    if (log) log->assign((size_t)cap * 5, 0.0);
    dpgo_polish_result_t r = {};
    const int rc = dpgo_group_polish(h_, X.data(), X.rows(), &o, max_bytes, Xout.data(), Xout.rows(), log ? log->data() : nullptr,
                                     log ? cap : 0, &r);
    if (log) log->resize(rc == 0 && r.outcome != DPGO_POLISH_SKIPPED ? (size_t)std::min(cap, r.steps + 1) * 5 : 0);
    if (status) *status = rc == 0 ? r.outcome : -1;
    if (result) *result = r;
    return rc == 0 && r.outcome == DPGO_POLISH_CONVERGED;
  }
  // Hessian modes (dpgo_group_hessian_modes): the k smallest eigenpairs of marginal_covariances' anchored Hessian by shift-invert
  // block subspace iteration on its factor; an indefinite Hessian is an input (the factor is that of H + mu I).  values and
  // residuals are resized to k, vectors to k dof N (row j the unit vector v_j by global pose), energy to k N (|v_j|^2 per pose).
  // X_escape (optional; sets want_escape): where values[0] < 0 a lower point along v_0, otherwise X.  At a polished minimum
  // 1 / values[0] is the largest eigenvalue of the covariance.  Returns true for DPGO_MODES_CONVERGED; status: the DPGO_MODES_*
  // outcome, -1 when the call itself failed (robust loss, a group that does not host every node, a bad anchor, k outside
  // 1 ... min(60, dof (N - 1))).
  bool hessian_modes(const Matrix &X, int k, std::vector<Scalar> &values, std::vector<Scalar> &vectors,
                     std::vector<Scalar> *residuals = nullptr, std::vector<Scalar> *energy = nullptr, Matrix *X_escape = nullptr,
                     int anchor = 0, dpgo_modes_result_t *result = nullptr, int *status = nullptr,
                     const dpgo_modes_options_t *opt = nullptr, long long max_bytes = 0) const {
    dpgo_modes_options_t o;
    dpgo_modes_options_default(&o);
    if (opt) o = *opt;
    o.want_escape = X_escape ? 1 : 0;
    const int d = graph_->d(), dof = d + d * (d - 1) / 2, N = (int)X.rows() / (d + 1), kk = std::max(k, 1);
    std::vector<Scalar> res_own, en_own;
    std::vector<Scalar> &res = residuals ? *residuals : res_own, &en = energy ? *energy : en_own;
    values.assign((size_t)kk, 0.0);
    res.assign((size_t)kk, 0.0);
    vectors.assign((size_t)kk * dof * N, 0.0);
    en.assign((size_t)kk * N, 0.0);
    if (X_escape) *X_escape = X;
    dpgo_modes_result_t r = {};
    const int rc = dpgo_group_hessian_modes(h_, X.data(), X.rows(), anchor, k, &o, max_bytes, values.data(), res.data(), vectors.data(),
                                            en.data(), X_escape ? X_escape->data() : nullptr, &r);
    if (status) *status = rc == 0 ? r.outcome : -1;
    if (result) *result = r;
    return rc == 0 && r.outcome == DPGO_MODES_CONVERGED;
  }
  // Newton polish of the ROBUST objective F = 1/2 sum_intra s_e + 1/2 sum_inter rho(s_e) (dpgo_group_robust_polish): the loop of
  // newton_polish with the robust F, gradient and Hessian written on the device.  This group is a trivial-loss group that hosts
  // every node of its graph; the loss is an argument.  curvature 1: the true Hessian, with the curvature 2 rho'' of the loss;
  // 0: the re-weighted one.  summary (optional) describes the final point.  Returns, status and the rest as newton_polish.
  bool robust_newton_polish(const Matrix &X, Loss loss, double loss_reg, Matrix &Xout, dpgo_polish_result_t *result = nullptr,
                            int *status = nullptr, int curvature = 1, const dpgo_polish_options_t *opt = nullptr,
                            long long max_bytes = 0, std::vector<Scalar> *log = nullptr, dpgo_edge_summary_t *summary = nullptr) const {
    dpgo_polish_options_t o;
    dpgo_polish_options_default(&o);
    if (opt) o = *opt;
    Xout = X;
    const int cap = o.max_steps >= 0 ? o.max_steps + 1 : 0;
    if (log) log->assign((size_t)cap * 5, 0.0);
    dpgo_polish_result_t r = {};
    const int rc = dpgo_group_robust_polish(h_, graph_->handle(), X.data(), X.rows(), (int)loss, loss_reg, curvature, &o, max_bytes,
                                            Xout.data(), Xout.rows(), log ? log->data() : nullptr, log ? cap : 0, &r, summary);
    if (log) log->resize(rc == 0 && r.outcome != DPGO_POLISH_SKIPPED ? (size_t)std::min(cap, r.steps + 1) * 5 : 0);
    if (status) *status = rc == 0 ? r.outcome : -1;
    if (result) *result = r;
    return rc == 0 && r.outcome == DPGO_POLISH_CONVERGED;
  }
  // Maximum-likelihood refinement on the measurements' full information matrices (dpgo_group_ml_polish): the loop of newton_polish
  // on F_ml = 1/2 sum r' Omega r with its Gauss-Newton Hessian -- what g2o, GTSAM and Ceres minimise on the same file.  Start it
  // from newton_polish's point.  The graph's Omega is the file's (Omega_iso for a graph built from arrays without).  Returns,
  // status and the rest as newton_polish; result->polish carries its fields.
  bool ml_polish(const Matrix &X, Matrix &Xout, dpgo_ml_result_t *result = nullptr, int *status = nullptr,
                 const dpgo_polish_options_t *opt = nullptr, long long max_bytes = 0, std::vector<Scalar> *log = nullptr) const {
    dpgo_polish_options_t o;
    dpgo_polish_options_default(&o);
    if (opt) o = *opt;
    Xout = X;
    const int cap = o.max_steps >= 0 ? o.max_steps + 1 : 0;
    if (log) log->assign((size_t)cap * 5, 0.0);
    dpgo_ml_result_t r = {};
    const int rc = dpgo_group_ml_polish(h_, graph_->handle(), X.data(), X.rows(), &o, max_bytes, Xout.data(), Xout.rows(),
                                        log ? log->data() : nullptr, log ? cap : 0, &r);
    if (log) log->resize(rc == 0 && r.polish.outcome != DPGO_POLISH_SKIPPED ? (size_t)std::min(cap, r.polish.steps + 1) * 5 : 0);
    if (status) *status = rc == 0 ? r.polish.outcome : -1;
    if (result) *result = r;
    return rc == 0 && r.polish.outcome == DPGO_POLISH_CONVERGED;
  }
  // Marginal covariances of the maximum-likelihood objective at X (dpgo_group_ml_covariance): marginal_covariances on
  // H = sum J' Omega J, the Fisher information.  Arguments, returns and status as marginal_covariances.
  bool ml_marginal_covariances(const Matrix &X, std::vector<Scalar> &marginals, int anchor = 0, dpgo_cov_result_t *result = nullptr,
                               int *status = nullptr, const std::vector<int> *pairs = nullptr, std::vector<Scalar> *cross = nullptr,
                               long long max_bytes = 0) const {
    const int d = graph_->d(), N = graph_->num_poses();
    const int dof = d + d * (d - 1) / 2, npairs = pairs && cross ? (int)pairs->size() / 2 : 0;
    marginals.assign((size_t)N * dof * dof, 0.0);
    if (cross) cross->assign((size_t)npairs * dof * dof, 0.0);
    dpgo_cov_result_t r = {};
    const int rc = dpgo_group_ml_covariance(h_, graph_->handle(), X.data(), X.rows(), anchor, max_bytes,
                                            npairs ? pairs->data() : nullptr, npairs, marginals.data(),
                                            npairs ? cross->data() : nullptr, &r);
    if (status) *status = rc == 0 ? r.outcome : -1;
    if (result) *result = r;
    return rc == 0 && r.outcome == DPGO_COV_OK;
  }
  // Per-edge reliability on the full information matrices (dpgo_group_ml_edge_reliability): edge_reliability on
  // H = sum J' Omega J with the statistics measured in the graph's Omega, so that d2_loo is a chi-square quantity of dof degrees
  // of freedom for anisotropic noise.  X should be ml_polish's point.  Arguments, records, returns and status as edge_reliability.
  bool ml_edge_reliability(const Matrix &X, std::vector<Scalar> &records, int anchor = 0, dpgo_rely_result_t *result = nullptr,
                           int *status = nullptr, const std::vector<int> *edges = nullptr, int method = DPGO_RELY_AUTO,
                           long long max_bytes = 0, std::vector<Scalar> *rel = nullptr, std::vector<Scalar> *joint = nullptr) const {
    const int d = graph_->d(), dof = d + d * (d - 1) / 2;
    const size_t n = edges ? edges->size() : (size_t)graph_->num_edges();
    records.assign(n * (6 + 2 * dof), 0.0);
    if (rel) rel->assign(n * dof * dof, 0.0);
    if (joint) joint->assign(n * 3 * dof * dof, 0.0);
    const int none = 0;   // (an empty list is a list: neither its pointer nor that of its records may be null)
    Scalar no_record = 0;
    dpgo_rely_result_t r = {};
    const int rc = dpgo_group_ml_edge_reliability(h_, graph_->handle(), X.data(), X.rows(), anchor, max_bytes, method,
                                                  edges ? (edges->empty() ? &none : edges->data()) : nullptr,
                                                  edges ? (int)edges->size() : 0, records.empty() ? &no_record : records.data(),
                                                  rel ? rel->data() : nullptr, joint ? joint->data() : nullptr, &r);
    if (status) *status = rc == 0 ? r.outcome : -1;
    if (result) *result = r;
    return rc == 0 && r.outcome == DPGO_RELY_OK;
  }
  // The loop-closure gate on the full information matrices (dpgo_group_ml_pair_gate).  pairs: 2 npairs global poses (p == q and
  // the anchor allowed); cand_R: npairs d d doubles, row-major; cand_t: npairs d; cand_info: npairs dof dof, each symmetric
  // positive definite.  gate is resized to npairs (2 + dof) doubles -- d2 = r' (rel + info^-1)^-1 r, not_pd, the ML residual --
  // joint and rel as pair_covariances.  Returns true for DPGO_PAIRS_OK; status: the outcome, -1 when the call itself failed.
  bool ml_pair_gate(const Matrix &X, const std::vector<int> &pairs, const std::vector<Scalar> &cand_R, const std::vector<Scalar> &cand_t,
                    const std::vector<Scalar> &cand_info, std::vector<Scalar> &gate, std::vector<Scalar> &joint, std::vector<Scalar> &rel,
                    int anchor = 0, dpgo_pairs_result_t *result = nullptr, int *status = nullptr, long long max_bytes = 0) const {
    const int d = graph_->d(), npairs = (int)pairs.size() / 2;
    const int dof = d + d * (d - 1) / 2;
    joint.assign((size_t)npairs * 3 * dof * dof, 0.0);
    rel.assign((size_t)npairs * dof * dof, 0.0);
    gate.assign((size_t)npairs * (2 + dof), 0.0);
    const bool sized = cand_R.size() == (size_t)npairs * d * d && cand_t.size() == (size_t)npairs * d &&
                       cand_info.size() == (size_t)npairs * dof * dof;
    dpgo_pairs_result_t r = {};
    const int rc = !sized ? -1
                          : dpgo_group_ml_pair_gate(h_, graph_->handle(), X.data(), X.rows(), anchor, max_bytes, pairs.data(), npairs,
                                                    cand_R.data(), cand_t.data(), cand_info.data(), joint.data(), rel.data(),
                                                    gate.data(), &r);
    if (status) *status = rc == 0 ? r.outcome : -1;
    if (result) *result = r;
    return rc == 0 && r.outcome == DPGO_PAIRS_OK;
  }
  // Graduated non-convexity (dpgo_group_gnc): GNC-TLS / GNC-GM outlier rejection from X on the device.  This group is a
  // trivial-loss group that hosts every node of its graph.  opt NULL: the defaults (TLS, barc2 1); robust_set (optional, one int
  // per edge of the graph): the edges the loss may touch, instead of the inter-node ones.  Xout: the point (X itself for
  // SKIPPED), weights: one per edge (0: rejected under TLS).  log (optional): 10 doubles per level (include/dpgo_amd.h).
  // Returns true for CONVERGED and ALL_INLIERS; status: the outcome, -1 where the call failed.
  bool graduated_non_convexity(const Matrix &X, Matrix &Xout, std::vector<Scalar> &weights, dpgo_gnc_result_t *result = nullptr,
                               int *status = nullptr, const dpgo_gnc_options_t *opt = nullptr,
                               const std::vector<int> *robust_set = nullptr, long long max_bytes = 0,
                               std::vector<Scalar> *log = nullptr) const {
    dpgo_gnc_options_t o;
    dpgo_gnc_options_default(&o);
    if (opt) o = *opt;
    Xout = X;
    weights.assign((size_t)graph_->num_edges(), 1.0);
    if (robust_set && (int)robust_set->size() != graph_->num_edges()) {
      if (status) *status = -1;
      return false;
    }
    const int cap = o.max_levels > 0 ? o.max_levels : 0;
    if (log) log->assign((size_t)cap * 10, 0.0);
    dpgo_gnc_result_t r = {};
    const int rc = dpgo_group_gnc(h_, graph_->handle(), X.data(), X.rows(), &o, robust_set ? robust_set->data() : nullptr, max_bytes,
                                  Xout.data(), Xout.rows(), weights.data(), log && cap ? log->data() : nullptr, log ? cap : 0, &r);
    if (log) log->resize(rc == 0 ? (size_t)std::min(cap, r.levels) * 10 : 0);
    if (status) *status = rc == 0 ? r.outcome : -1;
    if (result) *result = r;
    return rc == 0 && (r.outcome == DPGO_GNC_CONVERGED || r.outcome == DPGO_GNC_ALL_INLIERS);
  }
  // Graduated non-convexity on the measurements' full information matrices (dpgo_group_ml_gnc): graduated_non_convexity's
  // levels on chi2_e = r_e' Omega_e r_e of ml_polish's objective, so that opt->barc2 is a chi2_dof quantile (dof 3 for d = 2, 6
  // for d = 3: 16.266 / 22.458 at 0.999).  An inner MAX_STEPS is normal; an edge of weight exactly 0 contributes exact zeros.
  // Arguments, returns and status as graduated_non_convexity; result->gnc carries its fields, result->near_pi the edges with
  // w > 0 within 1e-3 of pi at the final point.
  bool ml_graduated_non_convexity(const Matrix &X, Matrix &Xout, std::vector<Scalar> &weights, dpgo_ml_gnc_result_t *result = nullptr,
                                  int *status = nullptr, const dpgo_gnc_options_t *opt = nullptr,
                                  const std::vector<int> *robust_set = nullptr, long long max_bytes = 0,
                                  std::vector<Scalar> *log = nullptr) const {
    dpgo_gnc_options_t o;
    dpgo_gnc_options_default(&o);
    if (opt) o = *opt;
    Xout = X;
    weights.assign((size_t)graph_->num_edges(), 1.0);
    if (robust_set && (int)robust_set->size() != graph_->num_edges()) {
      if (status) *status = -1;
      return false;
    }
    const int cap = o.max_levels > 0 ? o.max_levels : 0;
    if (log) log->assign((size_t)cap * 10, 0.0);
    dpgo_ml_gnc_result_t r = {};
    const int rc = dpgo_group_ml_gnc(h_, graph_->handle(), X.data(), X.rows(), &o, robust_set ? robust_set->data() : nullptr, max_bytes,
                                     Xout.data(), Xout.rows(), weights.data(), log && cap ? log->data() : nullptr, log ? cap : 0, &r);
    if (log) log->resize(rc == 0 ? (size_t)std::min(cap, r.gnc.levels) * 10 : 0);
    if (status) *status = rc == 0 ? r.gnc.outcome : -1;
    if (result) *result = r;
    return rc == 0 && (r.gnc.outcome == DPGO_GNC_CONVERGED || r.gnc.outcome == DPGO_GNC_ALL_INLIERS);
  }
  // Marginal covariances of the robust objective at X (dpgo_group_robust_covariance): marginal_covariances on the true Hessian
  // (curvature 1) or the re-weighted one (0).  DPGO_COV_NOT_PD is a legitimate answer where the negative curvature of the loss
  // wins.  Arguments, returns and status as marginal_covariances.
  bool robust_marginal_covariances(const Matrix &X, Loss loss, double loss_reg, std::vector<Scalar> &marginals, int anchor = 0,
                                   dpgo_cov_result_t *result = nullptr, int *status = nullptr, int curvature = 1,
                                   const std::vector<int> *pairs = nullptr, std::vector<Scalar> *cross = nullptr,
                                   long long max_bytes = 0) const {
    const int d = graph_->d(), N = graph_->num_poses();
    const int dof = d + d * (d - 1) / 2, npairs = pairs && cross ? (int)pairs->size() / 2 : 0;
    marginals.assign((size_t)N * dof * dof, 0.0);
    if (cross) cross->assign((size_t)npairs * dof * dof, 0.0);
    dpgo_cov_result_t r = {};
    const int rc = dpgo_group_robust_covariance(h_, graph_->handle(), X.data(), X.rows(), (int)loss, loss_reg, curvature, anchor,
                                                max_bytes, npairs ? pairs->data() : nullptr, npairs, marginals.data(),
                                                npairs ? cross->data() : nullptr, &r);
    if (status) *status = rc == 0 ? r.outcome : -1;
    if (result) *result = r;
    return rc == 0 && r.outcome == DPGO_COV_OK;
  }
  // Measurement sensitivities of the robust objective (dpgo_group_robust_sensitivity): measurement_sensitivities at a critical
  // point of the robust objective (robust_newton_polish with the same loss and loss_reg), the adjoints on its true Hessian, the
  // loss threshold one more parameter.  sens is resized to k num_edges (3 + dof): [l][e][d/dkappa, d/dtau, d/dt~, d/deta, the
  // edge's term of d/dloss_reg]; dloss_reg to k: dL_l/dloss_reg.  DPGO_SENS_NOT_PD is a legitimate answer under Geman-McClure and
  // Welsch.  Other arguments, returns and status as measurement_sensitivities.
  bool robust_measurement_sensitivities(const Matrix &X, Loss loss, double loss_reg, const std::vector<Scalar> &upstream,
                                        std::vector<Scalar> &sens, std::vector<Scalar> &dloss_reg, int anchor = 0,
                                        dpgo_sens_result_t *result = nullptr, int *status = nullptr,
                                        std::vector<Scalar> *adjoint = nullptr, long long max_bytes = 0) const {
    const int d = graph_->d(), dof = d + d * (d - 1) / 2, m = graph_->num_edges();
    const size_t n = (size_t)dof * graph_->num_poses();
    const int k = n ? (int)(upstream.size() / n) : 0;
    const bool sized = k >= 1 && upstream.size() == n * (size_t)k;
    sens.assign(sized ? (size_t)k * m * (3 + dof) : 0, 0.0);
    dloss_reg.assign(sized ? (size_t)k : 0, 0.0);
    if (adjoint) adjoint->assign(sized ? n * (size_t)k : 0, 0.0);
    dpgo_sens_result_t r = {};
    const int rc = !sized ? -1
                          : dpgo_group_robust_sensitivity(h_, graph_->handle(), X.data(), X.rows(), (int)loss, loss_reg, anchor, max_bytes,
                                                          upstream.data(), (int)n, k, adjoint ? adjoint->data() : nullptr, sens.data(),
                                                          dloss_reg.data(), &r);
    if (status) *status = rc == 0 ? r.outcome : -1;
    if (result) *result = r;
    return rc == 0 && r.outcome == DPGO_SENS_OK;
  }
  // The Riemannian staircase (dpgo_group_staircase): from X -- usually a point whose certificate is NEGATIVE -- the reference's
  // truncated-Newton method at rank r, fast_verification at the lifted point, an escape along the certificate's direction one
  // rank up, until the certificate is not NEGATIVE or r = r_max <= 2d; then the rounding and a polish.  Xhat: the result, never
  // worse than X (X itself when the call is SKIPPED or fails).  result->gap = F_final - F_sdp bounds the distance to the global
  // minimum only where result->cert_status is DPGO_CERT_PROVEN and result->stationarity is small.  log (optional): per level
  // rank, F in, F out, |grad|, TNT iterations, Hessian products, certificate status, theta, accepted alpha, halvings.  Returns
  // true for DPGO_STAIR_SOLVED; status: the DPGO_STAIR_* outcome, -1 when the call itself failed.
  bool riemannian_staircase(const Matrix &X, Matrix &Xhat, dpgo_staircase_result_t *result = nullptr, int *status = nullptr,
                            const dpgo_staircase_options_t *opt = nullptr, long long max_bytes = 0,
                            std::vector<Scalar> *log = nullptr, Matrix *Y = nullptr) const {
    dpgo_staircase_options_t o;
    dpgo_staircase_options_default(&o);
    if (opt) o = *opt;
    Xhat = X;
    const int cap = X.cols() + 1;
    if (log) log->assign((size_t)cap * 10, 0.0);
    if (Y) Y->resize(X.rows(), 2 * X.cols());
    dpgo_staircase_result_t r = {};
    const int rc = dpgo_group_staircase(h_, X.data(), X.rows(), &o, max_bytes, Xhat.data(), Xhat.rows(), Y ? Y->data() : nullptr,
                                        Y ? Y->rows() : 0, log ? log->data() : nullptr, log ? cap : 0, &r);
    if (log) log->resize(rc == 0 ? (size_t)std::min(cap, r.levels) * 10 : 0);
    if (status) *status = rc == 0 ? r.outcome : -1;
    if (result) *result = r;
    return rc == 0 && r.outcome == DPGO_STAIR_SOLVED;
  }
  const Graph &graph() const { return *graph_; }
  dpgo_group_t *handle() const { return h_; }

 private:
  friend class DPGOHash;
  std::shared_ptr<Graph> graph_;
  std::vector<int> nodes_;
  Options options_;
  dpgo_group_t *h_ = nullptr;
  std::vector<DPGOHash> hash_;
};

inline int DPGOHash::node() const { return dpgo_group_node_id(g_->h_, local_); }
inline int DPGOHash::initialize(const Matrix &X) const { return dpgo_group_initialize(g_->h_, local_, X.data(), X.rows()); }
inline int DPGOHash::update() const { return dpgo_group_update(g_->h_, &local_, 1); }
inline int DPGOHash::iterate() const { return dpgo_group_iterate(g_->h_, &local_, 1); }
inline int DPGOHash::receive(int beta, const Matrix &msg) const {
  return dpgo_group_receive(g_->h_, local_, beta, msg.data(), msg.rows());
}
inline Matrix DPGOHash::send(int beta) const {
  int ns = 0, nr = 0;
  if (dpgo_group_message_sizes(g_->h_, local_, beta, &ns, &nr) != 0) return Matrix();
  const int d = g_->graph_->d();
  Matrix msg((d + 1) * ns, d);
  if (ns > 0) dpgo_group_send(g_->h_, local_, beta, msg.data(), msg.rows());
  return msg;
}
inline DPGOResult DPGOHash::results(bool with_X) const {
  DPGOResult r;
  dpgo_group_results(g_->h_, local_, &r);
  if (with_X) {
    int n[2], m[2];
    g_->graph_->sizes(node(), n, m);
    const int d = g_->graph_->d(), rows = (d + 1) * (n[0] + n[1]);
    r.Xk.resize(rows, d);
    r.Xak.resize((d + 1) * n[0], d);
    dpgo_group_get_Xk(g_->h_, local_, r.Xk.data(), rows);
    dpgo_group_get_Xak(g_->h_, local_, r.Xak.data(), r.Xak.rows());
  }
  return r;
}
inline const Options &DPGOHash::options() const { return g_->options_; }

// AMM-PGO* (DPGOStar.h:13-61): initialize / update / iterate / communicate; every node lives in one group.
class DPGOStar {
 public:
  DPGOStar(int num_nodes, const std::string &filename, const Options &options, int device = 0)
      : graph_(Graph::read_g2o(filename, num_nodes)) {
    std::vector<int> all(num_nodes);
    for (int a = 0; a < num_nodes; a++) all[a] = a;
    group_.reset(new DPGOHashGroup(graph_, all, options, device));
  }
  int initialize(const Matrix &X) { return dpgo_group_star_initialize(group_->handle(), X.data(), X.rows()); }
  int update() { return dpgo_group_star_update(group_->handle()); }
  int iterate() { return dpgo_group_star_iterate(group_->handle()); }
  int communicate() { return group_->communicate(); }
  // F: running average (DPGOStar.cpp:210); fobj = F(X_k+1); fobjh = F(X_k+1/2)
  int state(double &F, double &fobj, double &fobjh, int &branches) const {
    return dpgo_group_star_state(group_->handle(), &F, &fobj, &fobjh, &branches);
  }
  // DPGOStar::evaluate_f / evaluate_grad (DPGOStar.h:49-51, DPGOStar.cpp:713-829): any X of size (d+1) N x d
  int evaluate_f(const Matrix &X, Scalar &fobj) const { return group_->evaluate_f(X, fobj); }
  int evaluate_grad(const Matrix &X, Matrix &grad) const { return group_->evaluate_grad(X, grad); }
  const Options &options() const { return group_->options(); }
  int set_options(const Options &o) { return group_->set_options(o); }
  int num_nodes() const { return graph_->num_nodes(); }
  const DPGOHashGroup &nodes() const { return *group_; }
  const Graph &graph() const { return *graph_; }

 private:
  std::shared_ptr<Graph> graph_;
  std::unique_ptr<DPGOHashGroup> group_;
};

// Pairwise consistency maximisation (PCM.h:10-71, PCM.cpp:5-235): the consistency test of the alpha-beta measurements
// runs on the GPU, the max clique on the host.  update() takes the graph and the GLOBAL iterate X ((d+1) N x d) instead
// of the reference's measurements_t + num_n / num_s / index; measurements() are edge indices of the graph, and
// adjancecy_matrix() (sic, the reference's name) is the m x m 0/1 matrix (symmetric, so row- or column-major alike).
class PCM {
 public:
  struct Options {
    Scalar tolerance = 0.2;
    bool weighted = false;
    Options() {}
  };

  explicit PCM(int device = 0) {
    if (dpgo_pcm_create(device, &h_) != 0) throw std::runtime_error("dpgo_pcm_create failed (no HIP device); there is no CPU path");
  }
  ~PCM() { dpgo_pcm_free(h_); }
  PCM(const PCM &) = delete;
  PCM &operator=(const PCM &) = delete;

  Scalar tolerance() const { return opts_.tolerance; }
  bool weighted() const { return opts_.weighted; }
  const std::vector<unsigned char> &adjancecy_matrix() const { return adjacency_; }
  const std::vector<int> &measurements() const { return measurements_; }
  const std::vector<bool> &results() const { return results_; }
  int num_m() const { return num_m_; }

  // 0 ok, -1 error (alpha == beta, a node out of range, X too small)
  int update(int alpha, int beta, const Graph &graph, const Matrix &X, const Options &opts = Options()) {
    reset();
    dpgo_pcm_options_t o;
    o.tolerance = opts.tolerance;
    o.weighted = opts.weighted ? 1 : 0;
    const int m = dpgo_pcm_update(h_, graph.handle(), alpha, beta, X.data(), X.rows(), &o);
    if (m < 0) return -1;
    opts_ = opts;
    num_m_ = m;
    measurements_.resize(m);
    adjacency_.resize((size_t)m * m);
    if (m > 0) {
      dpgo_pcm_measurements(h_, measurements_.data());
      dpgo_pcm_adjacency(h_, adjacency_.data());
    }
    return 0;
  }
  const std::vector<bool> &solveExact() const { return solve(1); }
  const std::vector<bool> &solveHeuristic() const { return solve(0); }

  int reset() {
    opts_ = Options();
    num_m_ = 0;
    measurements_.clear();
    adjacency_.clear();
    results_.clear();
    return 0;
  }

 private:
  const std::vector<bool> &solve(int exact) const {
    std::vector<unsigned char> in(num_m_ > 0 ? num_m_ : 1, 0);
    results_.assign(num_m_, false);
    if (num_m_ > 0 && dpgo_pcm_solve(h_, exact, in.data()) >= 0)
      for (int k = 0; k < num_m_; k++) results_[k] = in[k] != 0;
    return results_;
  }
  dpgo_pcm_t *h_ = nullptr;
  Options opts_;
  int num_m_ = 0;
  std::vector<int> measurements_;
  std::vector<unsigned char> adjacency_;
  mutable std::vector<bool> results_;
};

// What a robust loss did to every measurement at a global X ((d+1) N x d): per edge, in file order, the rotation and
// translation parts of the squared residual, the loss value and the loss weight (DPGOProblem::evaluate_E,
// DPGOProblem.cpp:634-681, for every edge of the graph), on the GPU (dpgo_edge_eval_*).  Intra-node edges: rho = s, w = 1.
class EdgeEvaluation {
 public:
  explicit EdgeEvaluation(const Graph &graph, int device = 0) : m_(graph.num_edges()) {
    if (dpgo_edge_eval_create(graph.handle(), device, &h_) != 0)
      throw std::runtime_error("dpgo_edge_eval_create failed (no HIP device); there is no CPU path");
  }
  ~EdgeEvaluation() { dpgo_edge_eval_free(h_); }
  EdgeEvaluation(const EdgeEvaluation &) = delete;
  EdgeEvaluation &operator=(const EdgeEvaluation &) = delete;

  // 0 ok, -1 error (X too small, a robust loss with loss_reg <= 0)
  int run(const Matrix &X, Loss loss, Scalar loss_reg) {
    for (auto *v : {&s_rot_, &s_trans_, &rho_, &weight_}) v->assign(m_, 0.0);
    return dpgo_edge_eval_run(h_, X.data(), X.rows(), (int)loss, loss_reg, s_rot_.data(), s_trans_.data(), rho_.data(),
                              weight_.data(), &summary_);
  }
  const std::vector<Scalar> &s_rot() const { return s_rot_; }
  const std::vector<Scalar> &s_trans() const { return s_trans_; }
  const std::vector<Scalar> &rho() const { return rho_; }
  const std::vector<Scalar> &weight() const { return weight_; }
  const dpgo_edge_summary_t &summary() const { return summary_; }

 private:
  dpgo_edge_eval_t *h_ = nullptr;
  int m_ = 0;
  std::vector<Scalar> s_rot_, s_trans_, rho_, weight_;
  dpgo_edge_summary_t summary_{};
};

// fast_verification of the RE-WEIGHTED problem (dpgo_graph_verify_reweighted): the loss weights are frozen at X, the
// inter-node kappa, tau scaled by them, and DPGOHashGroup::fast_verification runs on a trivial-loss group of that graph.
// true: X is PROVEN to be the global minimiser of its own quadratic surrogate (a fixed point of an exact MM step) up to eta --
// NOT the global minimum of the robust objective; read `stationarity` (the robust gradient norm) with it.
inline bool fast_verification_reweighted(const Graph &graph, const Matrix &X, Loss loss, Scalar loss_reg, Scalar eta,
                                         Scalar &theta, Matrix &x, int &num_iters, int *status = nullptr,
                                         dpgo_cert_factor_t *factor = nullptr, dpgo_edge_summary_t *edges = nullptr,
                                         Scalar *stationarity = nullptr, long long max_factor_bytes = 0, int device = 0) {
  dpgo_cert_options_t o;
  dpgo_cert_options_default(&o);
  o.eta = eta;
  dpgo_cert_result_t r;
  dpgo_cert_factor_t f;
  x.resize(X.rows(), 1);
  const int rc = dpgo_graph_verify_reweighted(graph.handle(), device, X.data(), X.rows(), (int)loss, loss_reg, &o,
                                              max_factor_bytes, &r, &f, edges, x.data(), x.rows());
  if (rc != 0) {
    if (status) *status = -1;
    return false;
  }
  theta = r.theta;
  num_iters = r.iterations;
  if (status) *status = r.status;
  if (factor) *factor = f;
  if (stationarity) *stationarity = r.stationarity;
  return r.status == DPGO_CERT_PROVEN;
}

}  // namespace DPGO

#endif  // DPGO_AMD_HPP
