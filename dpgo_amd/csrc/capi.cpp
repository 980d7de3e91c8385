// C ABI (include/dpgo_amd.h) over the C++ host layer: the public entry points -- graphs, groups, the exchange, PCM, the
// certificate, covariances, the polish, the Hessian modes, the staircase -- and nothing that touches the device itself.  The test hooks
// (dpgo_debug_*, dpgo_group_debug_*) are in capi_debug.cpp; what both files share is in capi_util.h.
#include "capi_util.h"

#include <memory>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <map>
#include <numeric>
#include <set>

#include "cert.h"
#include "comm.h"
#include "pcm.h"

namespace dpgo {
int chordal_initialization(const Graph &g, double *X, int ld);
}

static void to_c(const dpgo::Options &d, dpgo_options_t *o) {
  o->scheme = d.scheme; o->regularizer = d.regularizer; o->accepted_delta = d.accepted_delta;
  o->eta[0] = d.eta[0]; o->eta[1] = d.eta[1]; o->psi = d.psi; o->phi = d.phi;
  o->max_soft_restart_hits[0] = d.max_soft_restart_hits[0]; o->max_soft_restart_hits[1] = d.max_soft_restart_hits[1];
  o->oscillation_cnt_period = d.oscillation_cnt_period; o->max_oscillations = d.max_oscillations;
  o->loss = d.loss; o->loss_reg = d.loss_reg; o->rescale = d.rescale; o->max_rescale_count = d.max_rescale_count;
  o->grad_norm_tol = d.grad_norm_tol;
  o->rel_func_decrease_tol = d.rel_func_decrease_tol; o->stepsize_tol = d.stepsize_tol;
  o->max_iterations = d.max_iterations; o->max_iterations_accepted = d.max_iterations_accepted;
  o->reg_Cholesky_precon_max_condition_number = d.reg_Cholesky_precon_max_condition_number;
  o->preconditioned_grad_norm_tol = d.preconditioned_grad_norm_tol; o->max_tCG_iterations = d.max_tCG_iterations;
  o->STPCG_kappa = d.STPCG_kappa; o->STPCG_theta = d.STPCG_theta; o->preconditioner = d.preconditioner;
  o->verbose = d.verbose;
}

extern "C" {

void dpgo_options_default(dpgo_options_t *o) { to_c(dpgo::Options(), o); }

void dpgo_options_driver(dpgo_options_t *o, int loss, int accelerated) {
  // C++/examples/dist_pgo.cpp:103-120
  dpgo_options_default(o);
  o->loss = loss;
  o->rescale = 0;   // Rescale::Static (dist_pgo.cpp:105)
  o->loss_reg = 0.25;
  o->scheme = accelerated ? 1 : 0;
  o->STPCG_kappa = 0.05;
  o->STPCG_theta = 0.9;
  o->eta[0] = 5e-4; o->eta[1] = 2.5e-2;
  o->max_soft_restart_hits[0] = 10; o->max_soft_restart_hits[1] = 25;
  o->max_iterations = 10;
  o->max_iterations_accepted = 1;
  o->grad_norm_tol = 1e-3;
  o->preconditioned_grad_norm_tol = 1e-4;
  o->regularizer = 1e-11;
}

int dpgo_read_g2o(const char *filename, int num_nodes, dpgo_graph_t **out) {
  auto *g = new dpgo_graph();
  if (dpgo::read_g2o(filename, num_nodes, g->g) != 0) { delete g; *out = nullptr; return -1; }
  *out = g;
  return 0;
}

// dpgo_graph_from_edges and dpgo_graph_from_edges_info (info null: the graph keeps no Omega)
static int graph_from_arrays(int d, int num_poses, int m, const int *I, const int *J, const double *R, const double *t,
                             const double *kappa, const double *tau, const double *info, int num_nodes, dpgo_graph_t **out) {
  *out = nullptr;
  if ((d != 2 && d != 3) || m <= 0 || num_poses <= 0 || num_nodes < 1 || !I || !J || !R || !t || !kappa || !tau) return -1;
  for (int e = 0; e < m; e++)
    if (I[e] < 0 || I[e] >= num_poses || J[e] < 0 || J[e] >= num_poses) {
      fprintf(stderr, "[dpgo_amd] ERROR: edge %d: pose id out of range (%d, %d), num_poses = %d.\n", e, I[e], J[e], num_poses);
      return -1;
    }
  auto *g = new dpgo_graph();
  g->g.d = d;
  g->g.num_poses = num_poses;
  g->g.all.resize(m);
  for (int e = 0; e < m; e++) {
    dpgo::Measurement &mm = g->g.all[e];
    std::memset(&mm, 0, sizeof(mm));
    mm.ipose = I[e]; mm.jpose = J[e];
    for (int k = 0; k < d * d; k++) mm.R[k] = R[(size_t)e * d * d + k];
    for (int k = 0; k < d; k++) mm.t[k] = t[(size_t)e * d + k];
    mm.kappa = kappa[e]; mm.tau = tau[e];
  }
  if (info) g->g.info.assign(info, info + (size_t)m * dpgo::graph_dof(d) * dpgo::graph_dof(d));
  if (dpgo::partition(g->g, num_nodes) != 0) { delete g; *out = nullptr; return -1; }
  *out = g;
  return 0;
}

int dpgo_graph_from_edges(int d, int num_poses, int m, const int *I, const int *J, const double *R, const double *t,
                          const double *kappa, const double *tau, int num_nodes, dpgo_graph_t **out) {
  if (!out) return -1;
  return graph_from_arrays(d, num_poses, m, I, J, R, t, kappa, tau, nullptr, num_nodes, out);
}

int dpgo_graph_from_edges_info(int d, int num_poses, int m, const int *I, const int *J, const double *R, const double *t,
                               const double *kappa, const double *tau, const double *info, int num_nodes, dpgo_graph_t **out) {
  if (!out) return -1;
  *out = nullptr;
  if (!info) return -1;
  return graph_from_arrays(d, num_poses, m, I, J, R, t, kappa, tau, info, num_nodes, out);
}

int dpgo_graph_edge_information(const dpgo_graph_t *g, double *out, int *has) {
  if (!g) return -1;
  if (has) *has = g->g.has_info() ? 1 : 0;
  if (out) {
    std::vector<double> om;
    dpgo::graph_information(g->g, om);
    std::copy(om.begin(), om.end(), out);
  }
  return 0;
}

void dpgo_graph_free(dpgo_graph_t *g) { delete g; }

int dpgo_graph_info(const dpgo_graph_t *g, int *d, int *num_poses, int *num_nodes, int *num_edges) {
  if (!g) return -1;
  if (d) *d = g->g.d;
  if (num_poses) *num_poses = g->g.num_poses;
  if (num_nodes) *num_nodes = g->g.num_nodes;
  if (num_edges) *num_edges = (int)g->g.all.size();
  return 0;
}

int dpgo_graph_edges(const dpgo_graph_t *g, int *I, int *J, double *R, double *t, double *kappa, double *tau) {
  if (!g) return -1;
  const int d = g->g.d;
  for (size_t e = 0; e < g->g.all.size(); e++) {
    const auto &m = g->g.all[e];
    if (I) I[e] = m.ipose;
    if (J) J[e] = m.jpose;
    if (R) for (int k = 0; k < d * d; k++) R[e * d * d + k] = m.R[k];
    if (t) for (int k = 0; k < d; k++) t[e * d + k] = m.t[k];
    if (kappa) kappa[e] = m.kappa;
    if (tau) tau[e] = m.tau;
  }
  return 0;
}

int dpgo_graph_node_sizes(const dpgo_graph_t *g, int node, int *n0, int *n1, int *m0, int *m1) {
  dpgo::DataInfo info;
  if (node_info(g, node, info) != 0) return -1;
  if (n0) *n0 = info.n[0];
  if (n1) *n1 = info.n[1];
  if (m0) *m0 = info.m[0];
  if (m1) *m1 = info.m[1];
  return 0;
}

int dpgo_graph_node_neighbours(const dpgo_graph_t *g, int node, int *nbr_node, int *nbr_pose) {
  dpgo::DataInfo info;
  if (node_info(g, node, info) != 0) return -1;
  for (int k = 0; k < info.n[1]; k++) {
    nbr_node[k] = info.nbr_key[k].first;
    nbr_pose[k] = info.nbr_key[k].second;
  }
  return 0;
}

int dpgo_graph_node_offset(const dpgo_graph_t *g, int node) {
  if (!g || node < 0 || node >= g->g.num_nodes || g->g.g_index[node].empty()) return -1;
  return g->g.g_index[node].begin()->second;
}

int dpgo_graph_exchange_plan(const dpgo_graph_t *g, const int *node_ids, int num_local, int *sent_nodes,
                             int *sent_poses, int *recv_nodes, int *recv_poses, int *counts) {
  // which own poses the nodes of this group export to nodes outside it, and which neighbour poses
  // they import from outside (sorted by (node, pose)); pointers may be NULL to query the counts
  if (!g || num_local <= 0) return -1;
  std::set<int> local(node_ids, node_ids + num_local);
  std::set<std::pair<int, int>> sent, recv;
  for (int k = 0; k < num_local; k++) {
    dpgo::DataInfo info;
    if (node_info(g, node_ids[k], info) != 0) return -1;
    for (const auto &s : info.sent)
      if (!local.count(s.first))
        for (int row : s.second) sent.insert({node_ids[k], info.own_pose[row]});
    for (const auto &key : info.nbr_key)
      if (!local.count(key.first)) recv.insert(key);
  }
  counts[0] = (int)sent.size();
  counts[1] = (int)recv.size();
  int i = 0;
  if (sent_nodes) for (const auto &s : sent) { sent_nodes[i] = s.first; sent_poses[i] = s.second; i++; }
  i = 0;
  if (recv_nodes) for (const auto &s : recv) { recv_nodes[i] = s.first; recv_poses[i] = s.second; i++; }
  return 0;
}

int dpgo_chordal_initialization(const dpgo_graph_t *g, double *X, int ld) {
  if (!g) return -1;
  return dpgo::chordal_initialization(g->g, X, ld);
}

int dpgo_group_create(const dpgo_graph_t *g, const int *node_ids, int num_local, const dpgo_options_t *opt,
                      int device, dpgo_group_t **out) {
  *out = nullptr;
  if (!g || num_local <= 0) return -1;
  if (!node_ids || !opt) return -1;
  std::vector<int> ids(node_ids, node_ids + num_local);
  if (std::set<int>(ids.begin(), ids.end()).size() != ids.size()) {
    fprintf(stderr, "[dpgo_amd] ERROR: dpgo_group_create: a node id appears twice.\n");
    return -1;
  }
  for (int id : ids)
    if (id < 0 || id >= g->g.num_nodes) {
      fprintf(stderr, "[dpgo_amd] ERROR: dpgo_group_create: node %d is not in [0, %d).\n", id, g->g.num_nodes);
      return -1;
    }
  return guarded([&] {
    auto *h = new dpgo_group();
    h->grp = new dpgo::Group(g->g, ids, to_cpp(*opt), device);
    if (!h->grp->ok()) {
      delete h->grp;
      delete h;
      return -1;
    }
    h->all.resize(num_local);
    std::iota(h->all.begin(), h->all.end(), 0);
    *out = h;
    return 0;
  });
}

void dpgo_group_free(dpgo_group_t *h) {
  if (!h) return;
  delete h->grp;
  delete h;
}

// the nodes a batched call works on: every node (locals == NULL), or a list of distinct local indices.
// false: an index is out of range or appears twice (res_[a] and the 64-bit node mask are indexed by it)
static bool sel(const dpgo_group_t *h, const int *locals, int n, std::vector<int> &out) {
  if (!locals || n <= 0) { out = h->all; return true; }
  out.assign(locals, locals + n);
  std::vector<char> seen(h->all.size(), 0);
  for (int a : out) {
    if (a < 0 || a >= (int)h->all.size() || seen[a]) {
      fprintf(stderr, "[dpgo_amd] ERROR: local node index %d is out of range [0, %zu) or repeated.\n", a, h->all.size());
      return false;
    }
    seen[a] = 1;
  }
  return true;
}

int dpgo_group_initialize(dpgo_group_t *h, int local, const double *X, int ld) { return guarded([&] { return h->grp->initialize(local, X, ld); }); }
int dpgo_group_initialize_global(dpgo_group_t *h, const double *X, int ld) { return guarded([&] { return h->grp->initialize_global(X, ld); }); }
int dpgo_group_update(dpgo_group_t *h, const int *locals, int n) {
  std::vector<int> v;
  if (!h || !sel(h, locals, n, v)) return -1;
  return guarded([&] { return h->grp->update(v); });
}
int dpgo_group_iterate(dpgo_group_t *h, const int *locals, int n) {
  std::vector<int> v;
  if (!h || !sel(h, locals, n, v)) return -1;
  return guarded([&] { return h->grp->iterate(v); });
}
int dpgo_group_communicate_local(dpgo_group_t *h) { return guarded([&] { return h->grp->communicate_local(); }); }
int dpgo_group_step(dpgo_group_t *h, struct dpgo_comm *comm) {
  if (!h) return -1;
  return guarded([&] {
    std::vector<int> all(h->grp->num_local());
    for (int a = 0; a < (int)all.size(); a++) all[a] = a;
    std::function<int()> xchg;
    if (comm && comm->c) xchg = [comm] { return comm->c->exchange(); };
    return h->grp->step(all, xchg);
  });
}
int dpgo_group_set_collectives(dpgo_group_t *h, void *send_dev, void *gathered_dev, dpgo_allgather_fn ag, dpgo_allreduce_fn ar,
                               void *user) {
  return guarded([&] { return h->grp->set_collectives((double *)send_dev, (double *)gathered_dev, ag, ar, user); });
}

int dpgo_group_star_initialize(dpgo_group_t *h, const double *X, int ld) { return guarded([&] { return h->grp->star_initialize_global(X, ld); }); }
int dpgo_group_star_update(dpgo_group_t *h) { return guarded([&] { return h->grp->star_update(); }); }
int dpgo_group_star_iterate(dpgo_group_t *h) { return guarded([&] { return h->grp->star_iterate(); }); }
int dpgo_group_star_state(const dpgo_group_t *h, double *F, double *fobj, double *fobjh, int *branches) {
  if (!h) return -1;
  return guarded([&] {
    if (F) *F = h->grp->star_F();
    if (fobj) *fobj = h->grp->star_fobj();
    if (fobjh) *fobjh = h->grp->star_fobjh();
    if (branches) *branches = h->grp->star_branches();
    return 0;
  });
}
int dpgo_group_receive(dpgo_group_t *h, int local, int beta, const double *msg, int ld) { return guarded([&] { return h->grp->receive(local, beta, msg, ld); }); }
int dpgo_group_send(const dpgo_group_t *h, int local, int beta, double *msg, int ld) { return guarded([&] { return h->grp->send(local, beta, msg, ld); }); }
int dpgo_group_message_sizes(const dpgo_group_t *h, int local, int beta, int *num_send, int *num_recv) {
  if (!h) return -1;
  return guarded([&] {
    const int s = h->grp->num_send(local, beta), r = h->grp->num_recv(local, beta);
    if (s < 0 || r < 0) return -1;
    if (num_send) *num_send = s;
    if (num_recv) *num_recv = r;
    return 0;
  });
}
int dpgo_group_num_sent(const dpgo_group_t *h) { return h->grp->num_sent(); }
int dpgo_group_sent_keys(const dpgo_group_t *h, int *nodes, int *poses) {
  const auto &k = h->grp->sent_keys();
  for (size_t i = 0; i < k.size(); i++) { nodes[i] = k[i].first; poses[i] = k[i].second; }
  return 0;
}
int dpgo_group_set_recv_layout(dpgo_group_t *h, int nranks, int stride, const int *counts, const int *nodes,
                               const int *poses) {
  return guarded([&] { return h->grp->set_recv_layout(nranks, stride, counts, nodes, poses); });
}
int dpgo_group_pack_sent(dpgo_group_t *h, void *buf) { return guarded([&] { return h->grp->pack_sent((double *)buf); }); }
int dpgo_group_unpack_recv(dpgo_group_t *h, const void *buf) { return guarded([&] { return h->grp->unpack_recv((const double *)buf); }); }
int dpgo_group_get_Xk(const dpgo_group_t *h, int local, double *X, int ld) { return guarded([&] { return h->grp->get_Xk(local, X, ld); }); }
int dpgo_group_get_Xak(const dpgo_group_t *h, int local, double *X, int ld) { return guarded([&] { return h->grp->get_X_own(local, X, ld); }); }
int dpgo_group_scatter_global(const dpgo_group_t *h, double *X, int ld) { return guarded([&] { return h->grp->scatter_global(X, ld); }); }
int dpgo_group_node_id(const dpgo_group_t *h, int local) {
  if (!h || local < 0 || local >= h->grp->num_local()) return -1;
  return h->grp->node_id(local);
}
int dpgo_group_sync(const dpgo_group_t *h) { return guarded([&] { h->grp->sync(); return 0; }); }
void *dpgo_group_stream(const dpgo_group_t *h) { return (void *)h->grp->stream(); }

int dpgo_group_results(const dpgo_group_t *h, int local, dpgo_results_t *o) {
  if (!h || !o || local < 0 || local >= h->grp->num_local()) return -1;
  // results() may have to take the deferred read-back of the last update(): a device error there becomes -1
  return guarded([&] {
  const dpgo::NodeResults &r = h->grp->results(local);
  o->updated = r.updated; o->iters = r.iters; o->gradFnorm = r.gradFnorm; o->fobjE = r.fobjE;
  o->Fk[0] = r.Fk[0]; o->Fk[1] = r.Fk[1]; o->Gk = r.Gk; o->Gkh = r.Gkh; o->fobj = r.fobj; o->f = r.f;
  o->gamma = r.gamma; o->s[0] = r.s0; o->s[1] = r.s1;
  o->soft_restart_hits[0] = r.soft_restart_hits[0]; o->soft_restart_hits[1] = r.soft_restart_hits[1];
  o->num_oscillations = r.num_oscillations; o->refined = r.refined; o->tnt_status = r.tnt_status;
  o->tnt_inner_iterations = r.tnt_inner; o->restarts = r.restarts;
  return 0;
  });
}

int dpgo_prof_enable(int on) { dpgo::prof_enable(on != 0); if (on) dpgo::prof_reset(); return 0; }
int dpgo_prof_num_kinds(void) { return dpgo::PK_COUNT; }
const char *dpgo_prof_kind_name(int k) {
  static const char *names[] = {"k_bsr", "k_inter", "k_proximal", "k_axpby", "k_dot", "k_rot_op", "k_copy_indexed",
                                "k_bdiag_dot", "k_reduce", "k_spd_fwd", "k_spd_bwd", "k_bsr_tcol"};
  static_assert(sizeof(names) / sizeof(names[0]) == dpgo::PK_COUNT, "one name per profiled kernel family");
  return (k >= 0 && k < dpgo::PK_COUNT) ? names[k] : "";
}
int dpgo_prof_collect(double *ms, double *bytes, long *count) { dpgo::prof_collect(ms, bytes, count); return 0; }
int dpgo_prof_collect_operands(double *operand_bytes) { if (!operand_bytes) return -1; dpgo::prof_collect_operands(operand_bytes); return 0; }
int dpgo_group_solver_stats(const dpgo_group_t *h, long *nnz_tt, long *nnz_rr, int *levels_tt, int *levels_rr) {
  *nnz_tt = (long)h->grp->factor_tt().nnz();
  *nnz_rr = (long)h->grp->factor_rr().nnz();
  *levels_tt = (int)h->grp->factor_tt().by_height.size();
  *levels_rr = (int)h->grp->factor_rr().by_height.size();
  return 0;
}

int dpgo_group_graph_stats(const dpgo_group_t *h, long *replays, long *captures, long *eager) {
  if (!h || !h->grp || !replays || !captures || !eager) return -1;
  h->grp->graph_stats(replays, captures, eager);
  return 0;
}

// ---- boundary: DPGOStar::evaluate_f / evaluate_grad, set_options / options, problem() accessors, g2o export ----
int dpgo_group_evaluate(dpgo_group_t *h, const double *X, int ld, double *F, double *grad_sqnorm, double *grad, int ldg) {
  if (!h || !X) return -1;
  return guarded([&] { return h->grp->evaluate_global(X, ld, F, grad_sqnorm, grad, ldg); });
}

int dpgo_group_set_options(dpgo_group_t *h, const dpgo_options_t *opt) {
  if (!h || !opt) return -1;
  return guarded([&] { return h->grp->set_options(to_cpp(*opt)); });
}

int dpgo_group_get_options(const dpgo_group_t *h, dpgo_options_t *o) {
  if (!h || !o) return -1;
  to_c(h->grp->options(), o);
  return 0;
}

int dpgo_graph_node_maps(const dpgo_graph_t *g, int node, int which, int *nodes, int *poses, int *block, int *local,
                         int *count) {
  dpgo::DataInfo info;
  if (!count || node_info(g, node, info) != 0 || which < 0 || which > 2) return -1;
  int k = 0;
  auto emit = [&](int b, int p, int blk, int loc) {
    if (nodes) { nodes[k] = b; poses[k] = p; block[k] = blk; local[k] = loc; }
    k++;
  };
  if (which == 0) {          // index_: own poses {0, k}, neighbour poses {1, k}   (DPGO_utils.cpp:400-418)
    for (int i = 0; i < info.n[0]; i++) emit(node, info.own_pose[i], 0, i);
    for (int i = 0; i < info.n[1]; i++) emit(info.nbr_key[i].first, info.nbr_key[i].second, 1, i);
  } else if (which == 1) {   // sent_[beta][own pose] = {0, k}                     (DPGO_utils.cpp:428-431)
    for (const auto &s : info.sent)
      for (int i : s.second) emit(s.first, info.own_pose[i], 0, i);
  } else {                   // recv_[beta][pose of beta] = {1, k}                 (DPGO_utils.cpp:432-435)
    for (const auto &r : info.recv)
      for (const auto &pk : r.second) emit(r.first, pk.first, 1, pk.second);
  }
  *count = k;
  return 0;
}

// g2o export: VERTEX_SE2 / VERTEX_SE3:QUAT lines from X plus the graph's edges.  The information matrices are the
// isotropic ones the loader's formulas invert (tau = d / tr(I_t^-1), kappa = I33 | 3 / (2 tr(I_R^-1)),
// DPGO_utils.cpp:63-67, 107-116), so reading the file back gives the same (R, t, kappa, tau).
int dpgo_write_g2o(const dpgo_graph_t *g, const double *X, int ld, const char *filename) {
  if (!g || !filename) return -1;
  const int d = g->g.d, N = g->g.num_poses;
  if (X && ld < (d + 1) * N) return -1;
  FILE *fp = fopen(filename, "w");
  if (!fp) {
    fprintf(stderr, "[dpgo_amd] ERROR: cannot open %s for writing.\n", filename);
    return -1;
  }
  auto quat = [](const double *R, double *q) {   // R row-major 3x3 -> (qx, qy, qz, qw)
    const double tr = R[0] + R[4] + R[8];
    if (tr > 0) {
      const double s = std::sqrt(tr + 1.0) * 2;
      q[3] = 0.25 * s; q[0] = (R[7] - R[5]) / s; q[1] = (R[2] - R[6]) / s; q[2] = (R[3] - R[1]) / s;
    } else if (R[0] > R[4] && R[0] > R[8]) {
      const double s = std::sqrt(1.0 + R[0] - R[4] - R[8]) * 2;
      q[3] = (R[7] - R[5]) / s; q[0] = 0.25 * s; q[1] = (R[1] + R[3]) / s; q[2] = (R[2] + R[6]) / s;
    } else if (R[4] > R[8]) {
      const double s = std::sqrt(1.0 + R[4] - R[0] - R[8]) * 2;
      q[3] = (R[2] - R[6]) / s; q[0] = (R[1] + R[3]) / s; q[1] = 0.25 * s; q[2] = (R[5] + R[7]) / s;
    } else {
      const double s = std::sqrt(1.0 + R[8] - R[0] - R[4]) * 2;
      q[3] = (R[3] - R[1]) / s; q[0] = (R[2] + R[6]) / s; q[1] = (R[5] + R[7]) / s; q[2] = 0.25 * s;
    }
  };
  if (X)
    for (int i = 0; i < N; i++) {
      // rows N + d i .. of X hold R_i^T: R_i(r, c) = X(N + d i + c, r)
      double R[9], t[3];
      for (int c = 0; c < d; c++) {
        t[c] = X[(size_t)c * ld + i];
        for (int r = 0; r < d; r++) R[r * d + c] = X[(size_t)r * ld + N + i * d + c];
      }
      if (d == 2) fprintf(fp, "VERTEX_SE2 %d %.17g %.17g %.17g\n", i, t[0], t[1], std::atan2(R[2], R[0]));
      else {
        double q[4];
        quat(R, q);
        fprintf(fp, "VERTEX_SE3:QUAT %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", i, t[0], t[1], t[2], q[0], q[1], q[2], q[3]);
      }
    }
  for (const auto &m : g->g.all) {
    if (d == 2) {
      fprintf(fp, "EDGE_SE2 %d %d %.17g %.17g %.17g %.17g 0 0 %.17g 0 %.17g\n", m.ipose, m.jpose, m.t[0], m.t[1],
              std::atan2(m.R[2], m.R[0]), m.tau, m.tau, m.kappa);
    } else {
      double q[4];
      quat(m.R, q);
      fprintf(fp, "EDGE_SE3:QUAT %d %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g", m.ipose, m.jpose, m.t[0], m.t[1], m.t[2], q[0], q[1],
              q[2], q[3]);
      for (int r = 0; r < 6; r++)
        for (int c = r; c < 6; c++) fprintf(fp, " %.17g", r == c ? (r < 3 ? m.tau : 2.0 * m.kappa) : 0.0);
      fprintf(fp, "\n");
    }
  }
  fclose(fp);
  return 0;
}

// ---- RCCL exchange (comm.cpp) ----
int dpgo_comm_unique_id(void *id128) {
  if (!id128) return -1;
  return guarded([&] { return dpgo::Comm::unique_id(id128); });
}

int dpgo_comm_create(dpgo_group_t *h, int rank, int nranks, const void *id128, dpgo_comm_t **out) {
  if (!out) return -1;
  *out = nullptr;
  if (!h || !id128 || nranks < 1 || rank < 0 || rank >= nranks) return -1;
  return guarded([&] {
    std::unique_ptr<dpgo_comm> c(new dpgo_comm());
    c->c = nullptr;
    std::unique_ptr<dpgo::Comm> cc(new dpgo::Comm(h->grp, rank, nranks, id128));   // (cleans up after itself when it throws)
    if (!cc->ok()) return -1;
    c->c = cc.release();
    *out = c.release();
    return 0;
  });
}

void dpgo_comm_free(dpgo_comm_t *c) {
  if (!c) return;
  (void)guarded([&] { delete c->c; return 0; });
  delete c;
}

int dpgo_comm_exchange(dpgo_comm_t *c) {
  if (!c) return -1;
  return guarded([&] { return c->c->exchange(); });
}

int dpgo_comm_allreduce_sum(dpgo_comm_t *c, double *vals, long n) {
  if (!c || !vals || n < 0) return -1;
  return guarded([&] { return n <= 4096 ? c->c->allreduce(vals, (int)n) : c->c->allreduce_large(vals, (size_t)n); });
}

int dpgo_comm_exchange_kind(const dpgo_comm_t *c) {
  if (!c || !c->c) return -1;
  return std::string(c->c->exchange_kind()) == "p2p" ? 1 : 0;
}

long dpgo_comm_bytes_sent(const dpgo_comm_t *c) {
  if (!c || !c->c) return -1;
  return (long)c->c->bytes_sent_per_exchange();
}

int dpgo_comm_create_self(dpgo_group_t *h, dpgo_comm_t **out) {
  if (!out) return -1;
  *out = nullptr;
  if (!h) return -1;
  return guarded([&] {
    unsigned char id[128];
    if (dpgo::Comm::unique_id(id) != 0) return -1;
    std::unique_ptr<dpgo_comm> c(new dpgo_comm());
    std::unique_ptr<dpgo::Comm> cc(new dpgo::Comm(h->grp, 0, 1, id, /*layout=*/false));
    if (cc->enable_self_exchange() != 0) return -1;
    c->c = cc.release();
    *out = c.release();
    return 0;
  });
}
int dpgo_comm_self_exchange(dpgo_comm_t *c) {
  if (!c || !c->c) return -1;
  return guarded([&] { return c->c->enable_self_exchange(); });
}
int dpgo_comm_enable_timing(dpgo_comm_t *c) {
  if (!c || !c->c) return -1;
  return guarded([&] { return c->c->enable_timing(); });
}
int dpgo_comm_exchange_time(dpgo_comm_t *c, double *mean_us, long *count) {
  if (!c || !c->c) return -1;
  return guarded([&] { return c->c->exchange_time(mean_us, count); });
}

int dpgo_comm_barrier(dpgo_comm_t *c) {
  if (!c) return -1;
  return guarded([&] { return c->c->barrier(); });
}

int dpgo_host_pack_sent(const dpgo_graph_t *g, const int *node_ids, int num_local, const double *X, int ld, double *buf) {
  if (!g || !node_ids || num_local <= 0 || !X || !buf) return -1;
  const int d = g->g.d, N = g->g.num_poses, RS = (d + 1) * d;
  if (ld < (d + 1) * N) return -1;
  int cnt[2];
  if (dpgo_graph_exchange_plan(g, node_ids, num_local, nullptr, nullptr, nullptr, nullptr, cnt) != 0) return -1;
  std::vector<int> sn(cnt[0]), sp(cnt[0]), rn(cnt[1]), rp(cnt[1]);
  if (dpgo_graph_exchange_plan(g, node_ids, num_local, sn.data(), sp.data(), rn.data(), rp.data(), cnt) != 0) return -1;
  for (int k = 0; k < cnt[0]; k++) {
    const int gid = g->g.g_index[sn[k]].at(sp[k]);
    for (int c = 0; c < d; c++) {
      buf[(size_t)k * RS + c] = X[(size_t)c * ld + gid];
      for (int r = 0; r < d; r++) buf[(size_t)k * RS + d + r * d + c] = X[(size_t)c * ld + N + gid * d + r];
    }
  }
  return cnt[0];
}

int dpgo_host_unpack_recv(const dpgo_graph_t *g, const int *node_ids, int num_local, int node, int nranks, int stride,
                          const int *counts, const int *nodes, const int *poses, const double *gathered, double *Z, int ldz) {
  if (!g || !node_ids || !counts || !nodes || !poses || !gathered || !Z || nranks < 1 || stride < 1) return -1;
  dpgo::DataInfo info;
  if (node_info(g, node, info) != 0) return -1;
  const int d = g->g.d, RS = (d + 1) * d, n0 = info.n[0], n1 = info.n[1];
  if (ldz < (d + 1) * (n0 + n1)) return -1;
  std::set<int> local(node_ids, node_ids + num_local);
  std::map<std::pair<int, int>, int> slot;
  int off = 0;
  for (int r = 0; r < nranks; r++) {
    for (int k = 0; k < counts[r]; k++) slot[{nodes[off + k], poses[off + k]}] = r * stride + k;
    off += counts[r];
  }
  int written = 0;
  for (int k = 0; k < n1; k++) {
    const auto key = info.nbr_key[k];
    if (local.count(key.first)) continue;
    auto it = slot.find(key);
    if (it == slot.end()) {
      fprintf(stderr, "[dpgo_amd] ERROR: No information for pose [%d, %d].\n", key.first, key.second);
      return -1;
    }
    const double *rec = gathered + (size_t)it->second * RS;
    for (int c = 0; c < d; c++) {
      Z[(size_t)c * ldz + (d + 1) * n0 + k] = rec[c];
      for (int r = 0; r < d; r++) Z[(size_t)c * ldz + (d + 1) * n0 + n1 + k * d + r] = rec[d + r * d + c];
    }
    written++;
  }
  return written;
}

void dpgo_dchordal_options_default(dpgo_dchordal_options_t *o) {
  const dpgo::DChordalOptions d;
  for (int k = 0; k < 4; k++) o->iters[k] = d.iters[k];
  o->local_iters = d.local_iters;
  o->reg_G = d.reg_G;
}

int dpgo_group_dist_chordal_initialization(dpgo_group_t *h, const dpgo_dchordal_options_t *opt, const double *X_local,
                                           int ld_local, double *X, int ld, double *objectives, int *num_objectives) {
  if (!h || !X) return -1;
  dpgo::DChordalOptions o;
  if (opt) {
    for (int k = 0; k < 4; k++) o.iters[k] = opt->iters[k];
    o.local_iters = opt->local_iters;
    o.reg_G = opt->reg_G;
    if (o.reg_G < 0 || o.local_iters < 0 || o.iters[0] < 0 || o.iters[1] < 0 || o.iters[2] < 0 || o.iters[3] < 0) return -1;
  }
  return guarded([&] {
    std::vector<double> obj;
    const int rc = h->grp->dist_chordal_initialization(o, X_local, ld_local, X, ld, objectives ? &obj : nullptr);
    if (rc == 0 && objectives && num_objectives) {
      const int n = std::min<int>(*num_objectives, (int)obj.size());
      std::copy(obj.begin(), obj.begin() + n, objectives);
      *num_objectives = (int)obj.size();
    }
    return rc;
  });
}

// ---- PCM (C++/DPGO/include/DPGO/PCM.h, C++/DPGO/src/PCM.cpp:5-235) ------------------------------------------------
struct dpgo_pcm {
  dpgo::Pcm *p = nullptr;
};

void dpgo_pcm_options_default(dpgo_pcm_options_t *o) {
  if (!o) return;
  o->tolerance = 0.2;   // PCM.h:14
  o->weighted = 0;      // PCM.h:15
}

int dpgo_pcm_create(int device, dpgo_pcm_t **out) {
  if (!out) return -1;
  *out = nullptr;
  return guarded([&] {
    auto *h = new dpgo_pcm();
    try {
      h->p = new dpgo::Pcm(device);
    } catch (...) {
      delete h;
      throw;
    }
    *out = h;
    return 0;
  });
}

void dpgo_pcm_free(dpgo_pcm_t *h) {
  if (!h) return;
  delete h->p;
  delete h;
}

// PCM::update (PCM.cpp:5-235)
int dpgo_pcm_update(dpgo_pcm_t *h, const dpgo_graph_t *g, int alpha, int beta, const double *X, int ld,
                    const dpgo_pcm_options_t *opts) {
  if (!h || !g) return -1;
  dpgo_pcm_options_t o;
  dpgo_pcm_options_default(&o);
  if (opts) o = *opts;
  return guarded([&] { return h->p->update(g->g, alpha, beta, X, ld, o.tolerance, o.weighted != 0); });
}

// PCM::measurements (PCM.h:39), as edge indices of the graph
int dpgo_pcm_measurements(const dpgo_pcm_t *h, int *edge_ids) {
  if (!h) return -1;
  if (edge_ids) std::copy(h->p->edge_ids.begin(), h->p->edge_ids.end(), edge_ids);
  return h->p->m;
}

// PCM::adjancecy_matrix (PCM.h:37)
int dpgo_pcm_adjacency(const dpgo_pcm_t *h, unsigned char *dense) {
  if (!h || (!dense && h->p->m > 0)) return -1;
  const int m = h->p->m, W = (m + 63) / 64;
  const uint64_t *b = h->p->bits.data();
  for (int r = 0; r < m; r++)
    for (int c = 0; c < m; c++) dense[(size_t)r * m + c] = (b[(size_t)r * W + c / 64] >> (c % 64)) & 1;
  return 0;
}

int dpgo_pcm_errors(dpgo_pcm_t *h, double *E) {
  if (!h) return -1;
  return guarded([&] { return h->p->errors(E); });
}

// PCM::solveExact / solveHeuristic (PCM.cpp:232-246)
int dpgo_pcm_solve(dpgo_pcm_t *h, int exact, unsigned char *inlier) {
  if (!h || (!inlier && h->p->m > 0)) return -1;
  return guarded([&] {
    std::vector<uint8_t> out;
    const int m = h->p->m;
    const int n = exact ? dpgo::max_clique_exact(m, h->p->bits.data(), out) : dpgo::max_clique_heuristic(m, h->p->bits.data(), out);
    std::copy(out.begin(), out.end(), inlier);
    return n;
  });
}

// ::PCM::PattabiramanMaxCliqueSolver{Exact,Heuristic}::find_max_clique (C++/PCM/include/PCM/PCM.hpp:29-66) on a dense
// 0/1 matrix, host only
int dpgo_max_clique(int m, const unsigned char *dense, int exact, unsigned char *out) {
  if (m < 0 || (m > 0 && (!dense || !out))) return -1;
  if (m > dpgo::PCM_MAX_M) return -1;
  return guarded([&] {
    const int W = (m + 63) / 64;
    std::vector<uint64_t> bits((size_t)m * W, 0);
    for (int r = 0; r < m; r++)
      for (int c = 0; c < m; c++)
        if (r == c || dense[(size_t)r * m + c] || dense[(size_t)c * m + r]) bits[(size_t)r * W + c / 64] |= 1ull << (c % 64);
    std::vector<uint8_t> o;
    const int n = exact ? dpgo::max_clique_exact(m, bits.data(), o) : dpgo::max_clique_heuristic(m, bits.data(), o);
    std::copy(o.begin(), o.end(), out);
    return n;
  });
}

int dpgo_graph_filter_edges(const dpgo_graph_t *g, const unsigned char *keep, dpgo_graph_t **out) {
  if (!out) return -1;
  *out = nullptr;
  if (!g || !keep) return -1;
  return guarded([&] {
    auto *f = new dpgo_graph();
    f->g.d = g->g.d;
    f->g.num_poses = g->g.num_poses;
    const size_t DD = (size_t)dpgo::graph_dof(g->g.d) * dpgo::graph_dof(g->g.d);
    for (size_t e = 0; e < g->g.all.size(); e++)
      if (keep[e]) {
        f->g.all.push_back(g->g.all[e]);
        if (g->g.has_info()) f->g.info.insert(f->g.info.end(), g->g.info.begin() + e * DD, g->g.info.begin() + (e + 1) * DD);
      }
    if (dpgo::partition(f->g, g->g.num_nodes) != 0) {
      fprintf(stderr, "[dpgo_amd] ERROR: dpgo_graph_filter_edges: no edge kept.\n");
      delete f;
      return -1;
    }
    *out = f;
    return 0;
  });
}

// ---- solution certificate (cert.h): SESyncProblem::verify_solution / fast_verification STEP 2
// (C++/SESync/src/SESyncProblem.cpp:375-468, C++/SESync/src/SESync_utils.cpp:721-830) ----
void dpgo_cert_options_default(dpgo_cert_options_t *o) {
  if (!o) return;
  const dpgo::CertOptions c;
  o->eta = c.eta; o->tau = c.tau; o->max_iters = c.max_iters; o->precondition = c.precondition;
  o->stop_on_negative = c.stop_on_negative; o->refresh_every = c.refresh_every; o->seed = c.seed;
}

static dpgo::CertOptions to_cpp(const dpgo_cert_options_t &opts) {
  dpgo::CertOptions o;
  o.eta = opts.eta; o.tau = opts.tau; o.max_iters = opts.max_iters; o.precondition = opts.precondition;
  o.stop_on_negative = opts.stop_on_negative; o.refresh_every = opts.refresh_every; o.seed = opts.seed;
  return o;
}

static void to_c(const dpgo::CertResult &r, dpgo_cert_result_t *o) {
  o->status = r.status; o->iterations = r.iterations; o->restarts = r.restarts;
  o->theta = r.theta; o->residual = r.residual; o->S_norm_est = r.S_norm_est;
  o->stationarity = r.stationarity;
}

int dpgo_group_certify(dpgo_group_t *h, const double *X, int ld, const dpgo_cert_options_t *opts, const double *V0, int ldv0,
                       dpgo_cert_result_t *result, double *x, int ldx) {
  if (!h || !h->grp || !X || !opts || !result) return -1;
  return guarded([&] {
    dpgo::CertResult r;
    const int rc = h->grp->certify(X, ld, to_cpp(*opts), V0, ldv0, r, x, ldx);
    to_c(r, result);
    return rc;
  });
}

int dpgo_group_cert_lambda(dpgo_group_t *h, const double *X, int ld, double *Lambda) {
  if (!h || !h->grp || !X || !Lambda) return -1;
  return guarded([&] { return h->grp->cert_lambda(X, ld, Lambda); });
}

int dpgo_group_cert_apply(dpgo_group_t *h, const double *X, int ld, const double *V, int ldv, double *SV, int ldsv) {
  if (!h || !h->grp || !X || !V || !SV) return -1;
  return guarded([&] { return h->grp->cert_apply(X, ld, V, ldv, SV, ldsv); });
}

// ---- fast_verification STEP 1 and the whole of it (C++/SESync/src/SESync_utils.cpp:731-754, :721-830) ----
static void put_factor(const dpgo::CertFactor &f, dpgo_cert_factor_t *o) {
  o->outcome = f.outcome; o->fronts = f.fronts; o->levels = f.levels; o->max_front = f.max_front;
  o->factor_entries = f.factor_entries; o->factor_bytes = f.factor_bytes;
  o->eta = f.eta; o->pivot_min = f.pivot_min; o->pivot_max = f.pivot_max; o->stationarity = f.stationarity;
  o->symbolic_s = f.symbolic_s; o->numeric_s = f.numeric_s;
}

int dpgo_group_cert_factor(dpgo_group_t *h, const double *X, int ld, double eta, long long max_factor_bytes,
                           dpgo_cert_factor_t *factor) {
  if (!h || !h->grp || !X || !factor) return -1;
  return guarded([&] {
    dpgo::CertFactor f;
    const int rc = h->grp->cert_factor(X, ld, eta, max_factor_bytes, f);
    put_factor(f, factor);
    return rc;
  });
}

int dpgo_group_verify(dpgo_group_t *h, const double *X, int ld, const dpgo_cert_options_t *opts, long long max_factor_bytes,
                      const double *V0, int ldv0, dpgo_cert_result_t *result, double *x, int ldx, dpgo_cert_factor_t *factor) {
  if (!h || !h->grp || !X || !opts || !result || !factor) return -1;
  return guarded([&] {
    dpgo::CertResult r;
    dpgo::CertFactor f;
    const int rc = h->grp->verify(X, ld, to_cpp(*opts), max_factor_bytes, V0, ldv0, r, x, ldx, f);
    to_c(r, result);
    put_factor(f, factor);
    return rc;
  });
}

int dpgo_group_cert_matrix(dpgo_group_t *h, const double *X, int ld, double eta, int *ptr, int *col, double *val, long long cap,
                           long long *nnz) {
  if (!h || !h->grp || !X || !nnz) return -1;
  return guarded([&] { return h->grp->cert_matrix(X, ld, eta, ptr, col, val, cap, nnz); });
}

// ---- per-edge residuals / weights (edges.h) and the certificate of the re-weighted problem ----
struct dpgo_edge_eval {
  dpgo::EdgeEval *p = nullptr;
};

int dpgo_edge_eval_create(const dpgo_graph_t *g, int device, dpgo_edge_eval_t **out) {
  if (!out) return -1;
  *out = nullptr;
  if (!g) return -1;
  return guarded([&] {
    auto h = std::make_unique<dpgo_edge_eval>();
    h->p = new dpgo::EdgeEval(g->g, device);
    *out = h.release();
    return 0;
  });
}

void dpgo_edge_eval_free(dpgo_edge_eval_t *h) {
  if (!h) return;
  delete h->p;
  delete h;
}

int dpgo_edge_eval_run(dpgo_edge_eval_t *h, const double *X, int ld, int loss, double loss_reg, double *s_rot, double *s_trans,
                       double *rho, double *weight, dpgo_edge_summary_t *sum) {
  if (!h || !h->p) return -1;
  return guarded([&] {
    dpgo::EdgeSummary s;
    const int rc = h->p->run(X, ld, loss, loss_reg, s_rot, s_trans, rho, weight, &s);
    if (rc == 0 && sum) to_c(s, sum);
    return rc;
  });
}

int dpgo_edge_eval_kernel_ms(const dpgo_edge_eval_t *h, double *ms) {
  if (!h || !h->p || !ms) return -1;
  *ms = h->p->kernel_ms;
  return 0;
}

int dpgo_graph_scale_edges(const dpgo_graph_t *g, const double *w, dpgo_graph_t **out) {
  if (!out) return -1;
  *out = nullptr;
  if (!g || !w) return -1;
  return guarded([&] {
    auto f = std::make_unique<dpgo_graph>();
    if (dpgo::scale_edges(g->g, w, f->g) != 0) return -1;
    *out = f.release();
    return 0;
  });
}

// The re-weighted problem at X: the loss weights w_e(X) of every edge (and their summary), the graph with kappa_e, tau_e
// scaled by them, a trivial-loss group of all its nodes.  `call` runs on that group and that graph; everything is freed again.  0 / -1
static int with_reweighted_group(const dpgo_graph_t *g, int device, const double *X, int ld, int loss, double loss_reg,
                                 dpgo_edge_summary_t *edge_summary, const std::function<int(dpgo_group_t *, const dpgo_graph_t *)> &call) {
  const int m = (int)g->g.all.size(), nn = g->g.num_nodes;
  std::vector<double> w((size_t)std::max(m, 1));
  dpgo_edge_eval_t *ev = nullptr;
  dpgo_graph_t *gw = nullptr;
  dpgo_group_t *grp = nullptr;
  int rc = dpgo_edge_eval_create(g, device, &ev);
  if (rc == 0) rc = dpgo_edge_eval_run(ev, X, ld, loss, loss_reg, nullptr, nullptr, nullptr, w.data(), edge_summary);
  dpgo_edge_eval_free(ev);
  if (rc == 0) rc = dpgo_graph_scale_edges(g, w.data(), &gw);
  if (rc == 0) {
    dpgo_options_t opt;
    dpgo_options_driver(&opt, 0, 1);
    opt.max_iterations = 0;
    std::vector<int> ids(nn);
    std::iota(ids.begin(), ids.end(), 0);
    rc = dpgo_group_create(gw, ids.data(), nn, &opt, device, &grp);
  }
  if (rc == 0) rc = call(grp, gw);
  dpgo_group_free(grp);
  dpgo_graph_free(gw);
  return rc == 0 ? 0 : -1;
}

int dpgo_graph_verify_reweighted(const dpgo_graph_t *g, int device, const double *X, int ld, int loss, double loss_reg,
                                 const dpgo_cert_options_t *cert_opts, long long max_factor_bytes,
                                 dpgo_cert_result_t *cert_result, dpgo_cert_factor_t *cert_factor,
                                 dpgo_edge_summary_t *edge_summary, double *x, int ldx) {
  if (!g || !X || !cert_result || !cert_factor) return -1;
  dpgo_cert_options_t co;
  dpgo_cert_options_default(&co);
  if (cert_opts) co = *cert_opts;
  return with_reweighted_group(g, device, X, ld, loss, loss_reg, edge_summary, [&](dpgo_group_t *grp, const dpgo_graph_t *) {
    return dpgo_group_verify(grp, X, ld, &co, max_factor_bytes, nullptr, 0, cert_result, x, ldx, cert_factor);
  });
}

// ---- marginal pose covariances (cov.h) ----
int dpgo_group_covariance(dpgo_group_t *h, const double *X, int ld, int anchor, long long max_bytes, const int *pairs,
                          int npairs, double *marginals, double *cross, dpgo_cov_result_t *result) {
  if (!h || !h->grp || !X || !marginals || !result || npairs < 0 || (npairs > 0 && (!pairs || !cross))) return -1;
  return guarded([&] {
    dpgo::CovResult r;
    const int rc = h->grp->covariance(X, ld, anchor, max_bytes, pairs, npairs, marginals, cross, r);
    to_c(r, result);
    return rc;
  });
}

int dpgo_group_cov_hessian(dpgo_group_t *h, const double *X, int ld, int anchor, int *ptr, int *col, double *val, long long cap,
                           long long *nnz) {
  if (!h || !h->grp || !X || !nnz) return -1;
  return guarded([&] { return h->grp->cov_hessian(X, ld, anchor, ptr, col, val, cap, nnz); });
}

int dpgo_graph_covariance_reweighted(const dpgo_graph_t *g, int device, const double *X, int ld, int loss, double loss_reg,
                                     int anchor, long long max_bytes, const int *pairs, int npairs, double *marginals,
                                     double *cross, dpgo_cov_result_t *result, dpgo_edge_summary_t *edge_summary) {
  if (!g || !X || !marginals || !result || npairs < 0 || (npairs > 0 && (!pairs || !cross))) return -1;
  return with_reweighted_group(g, device, X, ld, loss, loss_reg, edge_summary, [&](dpgo_group_t *grp, const dpgo_graph_t *) {
    return dpgo_group_covariance(grp, X, ld, anchor, max_bytes, pairs, npairs, marginals, cross, result);
  });
}

// ---- joint covariances of arbitrary pose pairs and the gate (pairs.h) ----
int dpgo_group_pair_covariance(dpgo_group_t *h, const double *X, int ld, int anchor, long long max_bytes, const int *pairs,
                               int npairs, const double *candidates, double *joint, double *rel, double *gate,
                               dpgo_pairs_result_t *result) {
  if (!h || !h->grp || !X || !result || npairs < 0 || (npairs > 0 && (!pairs || !joint || !rel)) || (candidates && !gate)) return -1;
  return guarded([&] {
    dpgo::PairsResult r;
    const int rc = h->grp->pair_covariance(X, ld, anchor, max_bytes, pairs, npairs, candidates, joint, rel, gate, r);
    to_c(r, result);
    return rc;
  });
}

int dpgo_graph_pair_covariance_reweighted(const dpgo_graph_t *g, int device, const double *X, int ld, int loss, double loss_reg,
                                          int anchor, long long max_bytes, const int *pairs, int npairs, const double *candidates,
                                          double *joint, double *rel, double *gate, dpgo_pairs_result_t *result,
                                          dpgo_edge_summary_t *edge_summary) {
  if (!g || !X || !result || npairs < 0 || (npairs > 0 && (!pairs || !joint || !rel)) || (candidates && !gate)) return -1;
  return with_reweighted_group(g, device, X, ld, loss, loss_reg, edge_summary, [&](dpgo_group_t *grp, const dpgo_graph_t *) {
    return dpgo_group_pair_covariance(grp, X, ld, anchor, max_bytes, pairs, npairs, candidates, joint, rel, gate, result);
  });
}

// ---- joint marginals of a pose set (marg.h) ----
int dpgo_group_joint_marginal(dpgo_group_t *h, const double *X, int ld, const int *keep, int nkeep, int anchor, int base,
                              int want_info, long long max_bytes, double *cov, double *info, double *logdet,
                              dpgo_marg_result_t *result) {
  if (!h || !h->grp || !X || !result || !keep || nkeep < 1 || !cov || !logdet || (want_info && !info)) return -1;
  return guarded([&] {
    dpgo::MargResult r;
    const int rc = h->grp->joint_marginal(X, ld, keep, nkeep, anchor, base, want_info != 0, max_bytes, cov, info, logdet, r);
    to_c(r, result);
    return rc;
  });
}

int dpgo_graph_joint_marginal_reweighted(const dpgo_graph_t *g, int device, const double *X, int ld, int loss, double loss_reg,
                                         const int *keep, int nkeep, int anchor, int base, int want_info, long long max_bytes,
                                         double *cov, double *info, double *logdet, dpgo_marg_result_t *result,
                                         dpgo_edge_summary_t *edge_summary) {
  if (!g || !X || !result || !keep || nkeep < 1 || !cov || !logdet || (want_info && !info)) return -1;
  return with_reweighted_group(g, device, X, ld, loss, loss_reg, edge_summary, [&](dpgo_group_t *grp, const dpgo_graph_t *) {
    return dpgo_group_joint_marginal(grp, X, ld, keep, nkeep, anchor, base, want_info, max_bytes, cov, info, logdet, result);
  });
}

// ---- joint compatibility and budgeted selection of loop-closure candidates (cand.h) ----
int dpgo_group_candidate_set(dpgo_group_t *h, const double *X, int ld, const int *pairs, int ncand, const double *candidates,
                             int anchor, int budget, double d2_max, int want_joint, long long max_bytes, double *cov, double *S,
                             double *residual, double *info, double *scalars, int *selected, double *steps, int *poses,
                             dpgo_cand_result_t *result) {
  if (!h || !h->grp || !X || !result) return -1;
  return guarded([&] {
    dpgo::CandResult r;
    dpgo::CandOut o;
    o.cov = cov; o.S = S; o.residual = residual; o.info = info; o.scalars = scalars; o.selected = selected; o.steps = steps;
    o.poses = poses;
    const int rc = h->grp->candidate_set(X, ld, pairs, ncand, candidates, anchor, budget, d2_max, want_joint != 0, max_bytes, o, r);
    to_c(r, result);
    return rc;
  });
}

int dpgo_graph_candidate_set_reweighted(const dpgo_graph_t *g, int device, const double *X, int ld, int loss, double loss_reg,
                                        const int *pairs, int ncand, const double *candidates, int anchor, int budget, double d2_max,
                                        int want_joint, long long max_bytes, double *cov, double *S, double *residual, double *info,
                                        double *scalars, int *selected, double *steps, int *poses, dpgo_cand_result_t *result,
                                        dpgo_edge_summary_t *edge_summary) {
  if (!g || !X || !result) return -1;
  return with_reweighted_group(g, device, X, ld, loss, loss_reg, edge_summary, [&](dpgo_group_t *grp, const dpgo_graph_t *) {
    return dpgo_group_candidate_set(grp, X, ld, pairs, ncand, candidates, anchor, budget, d2_max, want_joint, max_bytes, cov, S,
                                    residual, info, scalars, selected, steps, poses, result);
  });
}

// ---- measurement sensitivities (sens.h) ----
int dpgo_group_sensitivity(dpgo_group_t *h, const dpgo_graph_t *g, const double *X, int ld, int anchor, long long max_bytes,
                           const double *upstream, int ldu, int k, double *adjoint, double *sens, dpgo_sens_result_t *result) {
  if (!h || !h->grp || !g || !X || !upstream || !sens || !result || k < 1) return -1;
  return guarded([&] {
    dpgo::SensResult r;
    const int rc = h->grp->sensitivity(g->g, X, ld, anchor, max_bytes, upstream, ldu, k, adjoint, sens, r);
    to_c(r, result);
    return rc;
  });
}

// ---- per-edge reliability (rely.h) ----
int dpgo_group_edge_reliability(dpgo_group_t *h, const dpgo_graph_t *g, const double *X, int ld, int anchor, long long max_bytes,
                                int method, const int *edges, int nedges, double *records, double *rel, double *joint,
                                dpgo_rely_result_t *result) {
  if (!h || !h->grp || !g || !X || !records || !result || (edges && nedges < 0)) return -1;
  return guarded([&] {
    dpgo::RelyResult r;
    const int rc = h->grp->edge_reliability(g->g, X, ld, anchor, max_bytes, method, edges, nedges, records, rel, joint, r);
    to_c(r, result);
    return rc;
  });
}

int dpgo_graph_edge_reliability_reweighted(const dpgo_graph_t *g, int device, const double *X, int ld, int loss, double loss_reg,
                                           int anchor, long long max_bytes, int method, const int *edges, int nedges, double *records,
                                           double *rel, double *joint, dpgo_rely_result_t *result, dpgo_edge_summary_t *edge_summary) {
  if (!g || !X || !records || !result || (edges && nedges < 0)) return -1;
  // (the scaled graph has the edges of g in g's order, so the list means the same on both)
  return with_reweighted_group(g, device, X, ld, loss, loss_reg, edge_summary, [&](dpgo_group_t *grp, const dpgo_graph_t *gw) {
    return dpgo_group_edge_reliability(grp, gw, X, ld, anchor, max_bytes, method, edges, nedges, records, rel, joint, result);
  });
}

// ---- Newton polish (polish.h) ----
void dpgo_polish_options_default(dpgo_polish_options_t *opt) {
  if (!opt) return;
  const dpgo::PolishOptions o;
  opt->max_steps = o.max_steps; opt->max_tries = o.max_tries; opt->rel_tol = o.rel_tol; opt->grad_tol = o.grad_tol;
  opt->anchor = 0;
}

int dpgo_group_polish(dpgo_group_t *h, const double *X, int ld, const dpgo_polish_options_t *opt, long long max_bytes,
                      double *Xout, int ldout, double *log, int log_cap, dpgo_polish_result_t *result) {
  if (!h || !h->grp || !X || !Xout || !result || log_cap < 0 || (log_cap > 0 && !log)) return -1;
  return guarded([&] {
    dpgo::PolishResult r;
    const int rc = h->grp->polish(X, ld, opt ? opt->anchor : 0, to_cpp(opt), max_bytes, Xout, ldout, log, log_cap, r);
    to_c(r, result);
    return rc;
  });
}

// ---- Hessian modes (modes.h) ----
void dpgo_modes_options_default(dpgo_modes_options_t *opt) {
  if (!opt) return;
  const dpgo::ModesOptions o;
  opt->guard = o.guard; opt->max_iters = o.max_iters; opt->max_tries = o.max_tries; opt->want_escape = o.want_escape;
  opt->rel_tol = o.rel_tol; opt->shift = o.shift; opt->seed = o.seed;
}

int dpgo_group_hessian_modes(dpgo_group_t *h, const double *X, int ld, int anchor, int k, const dpgo_modes_options_t *opts,
                             long long max_bytes, double *values, double *residuals, double *vectors, double *energy,
                             double *X_escape, dpgo_modes_result_t *result) {
  if (!h || !h->grp || !X || !values || !residuals || !vectors || !energy || !result) return -1;
  return guarded([&] {
    dpgo::ModesResult r;
    const int rc = h->grp->hessian_modes(X, ld, anchor, k, to_cpp(opts), max_bytes, values, residuals, vectors, energy, X_escape, r);
    to_c(r, result);
    return rc;
  });
}

// ---- the robust objective: polish, covariances, the matrices behind them (robust.h) ----
int dpgo_group_robust_polish(dpgo_group_t *h, const dpgo_graph_t *g, const double *X, int ld, int loss, double loss_reg, int curvature,
                             const dpgo_polish_options_t *opt, long long max_bytes, double *Xout, int ldout, double *log, int log_cap,
                             dpgo_polish_result_t *result, dpgo_edge_summary_t *edge_summary) {
  if (!h || !h->grp || !g || !X || !Xout || !result || log_cap < 0 || (log_cap > 0 && !log)) return -1;
  return guarded([&] {
    dpgo::PolishResult r;
    dpgo::EdgeSummary s;
    const int rc = h->grp->robust_polish(g->g, X, ld, loss, loss_reg, curvature, opt ? opt->anchor : 0, to_cpp(opt), max_bytes, Xout,
                                         ldout, log, log_cap, r, edge_summary ? &s : nullptr);
    to_c(r, result);
    if (rc == 0 && edge_summary && r.outcome != dpgo::POLISH_SKIPPED) to_c(s, edge_summary);
    return rc;
  });
}

int dpgo_group_robust_covariance(dpgo_group_t *h, const dpgo_graph_t *g, const double *X, int ld, int loss, double loss_reg,
                                 int curvature, int anchor, long long max_bytes, const int *pairs, int npairs, double *marginals,
                                 double *cross, dpgo_cov_result_t *result) {
  if (!h || !h->grp || !g || !X || !marginals || !result || npairs < 0 || (npairs > 0 && (!pairs || !cross))) return -1;
  return guarded([&] {
    dpgo::CovResult r;
    const int rc = h->grp->robust_covariance(g->g, X, ld, loss, loss_reg, curvature, anchor, max_bytes, pairs, npairs, marginals,
                                             cross, r);
    to_c(r, result);
    return rc;
  });
}

int dpgo_group_robust_sensitivity(dpgo_group_t *h, const dpgo_graph_t *g, const double *X, int ld, int loss, double loss_reg, int anchor,
                                  long long max_bytes, const double *upstream, int ldu, int k, double *adjoint, double *sens,
                                  double *dloss_reg, dpgo_sens_result_t *result) {
  if (!h || !h->grp || !g || !X || !upstream || !sens || !dloss_reg || !result || k < 1) return -1;
  return guarded([&] {
    dpgo::SensResult r;
    const int rc = h->grp->robust_sensitivity(g->g, X, ld, loss, loss_reg, anchor, max_bytes, upstream, ldu, k, adjoint, sens,
                                              dloss_reg, r);
    to_c(r, result);
    return rc;
  });
}

int dpgo_group_robust_hessian(dpgo_group_t *h, const dpgo_graph_t *g, const double *X, int ld, int loss, double loss_reg, int curvature,
                              int anchor, int *ptr, int *col, double *val, long long cap, long long *nnz, double *grad, double *F,
                              double *w, double *c, double *s_rot, double *s_trans, double *rho) {
  if (!h || !h->grp || !g || !X || !nnz) return -1;
  return guarded([&] {
    return h->grp->robust_hessian(g->g, X, ld, loss, loss_reg, curvature, anchor, ptr, col, val, cap, nnz, grad, F, w, c, s_rot, s_trans,
                                  rho);
  });
}

int dpgo_group_robust_matrix(dpgo_group_t *h, const dpgo_graph_t *g, const double *X, int ld, int loss, double loss_reg, int *ptr,
                             int *col, double *val, long long cap, long long *nnz) {
  if (!h || !h->grp || !g || !X || !nnz) return -1;
  return guarded([&] { return h->grp->robust_matrix(g->g, X, ld, loss, loss_reg, ptr, col, val, cap, nnz); });
}

// ---- maximum-likelihood refinement on the full information matrices (ml.h) ----
int dpgo_group_ml_polish(dpgo_group_t *h, const dpgo_graph_t *g, const double *X, int ld, const dpgo_polish_options_t *opt,
                         long long max_bytes, double *Xout, int ldout, double *log, int log_cap, dpgo_ml_result_t *result) {
  if (!h || !h->grp || !g || !X || !Xout || !result || log_cap < 0 || (log_cap > 0 && !log)) return -1;
  return guarded([&] {
    dpgo::MlResult r;
    const int rc = h->grp->ml_polish(g->g, X, ld, opt ? opt->anchor : 0, to_cpp(opt), max_bytes, Xout, ldout, log, log_cap, r);
    to_c(r, &result->polish);
    result->near_pi = r.near_pi;
    result->chi2_initial = r.chi2_initial;
    result->chi2_final = r.chi2_final;
    return rc;
  });
}

int dpgo_group_ml_covariance(dpgo_group_t *h, const dpgo_graph_t *g, const double *X, int ld, int anchor, long long max_bytes,
                             const int *pairs, int npairs, double *marginals, double *cross, dpgo_cov_result_t *result) {
  if (!h || !h->grp || !g || !X || !marginals || !result || npairs < 0 || (npairs > 0 && (!pairs || !cross))) return -1;
  return guarded([&] {
    dpgo::CovResult r;
    const int rc = h->grp->ml_covariance(g->g, X, ld, anchor, max_bytes, pairs, npairs, marginals, cross, r);
    to_c(r, result);
    return rc;
  });
}

// ---- edge reliability and candidate gating on the full information matrices (ml_rely.h) ----
int dpgo_group_ml_edge_reliability(dpgo_group_t *h, const dpgo_graph_t *g, const double *X, int ld, int anchor, long long max_bytes,
                                   int method, const int *edges, int nedges, double *records, double *rel, double *joint,
                                   dpgo_rely_result_t *result) {
  if (!h || !h->grp || !g || !X || !records || !result || (edges && nedges < 0)) return -1;
  return guarded([&] {
    dpgo::RelyResult r;
    const int rc = h->grp->ml_edge_reliability(g->g, X, ld, anchor, max_bytes, method, edges, nedges, records, rel, joint, r);
    to_c(r, result);
    return rc;
  });
}

int dpgo_group_ml_pair_gate(dpgo_group_t *h, const dpgo_graph_t *g, const double *X, int ld, int anchor, long long max_bytes,
                            const int *pairs, int npairs, const double *cand_R, const double *cand_t, const double *cand_info,
                            double *joint, double *rel, double *gate, dpgo_pairs_result_t *result) {
  if (!h || !h->grp || !g || !X || !result || npairs < 0) return -1;
  if (npairs > 0 && (!pairs || !cand_R || !cand_t || !cand_info || !joint || !rel || !gate)) return -1;
  return guarded([&] {
    dpgo::PairsResult r;
    const int rc = h->grp->ml_pair_gate(g->g, X, ld, anchor, max_bytes, pairs, npairs, cand_R, cand_t, cand_info, joint, rel, gate, r);
    to_c(r, result);
    return rc;
  });
}

int dpgo_group_ml_hessian(dpgo_group_t *h, const dpgo_graph_t *g, const double *X, int ld, int anchor, int *ptr, int *col, double *val,
                          long long cap, long long *nnz, double *grad, double *F) {
  if (!h || !h->grp || !g || !X || !nnz) return -1;
  return guarded([&] { return h->grp->ml_hessian(g->g, X, ld, anchor, ptr, col, val, cap, nnz, grad, F); });
}

int dpgo_group_ml_eval(dpgo_group_t *h, const dpgo_graph_t *g, const double *X, int ld, double *F, long long *near_pi, double *r,
                       double *chi2, double *wr, double *grad, double *jw) {
  if (!h || !h->grp || !g || !X) return -1;
  return guarded([&] { return h->grp->ml_eval(g->g, X, ld, F, near_pi, r, chi2, wr, grad, jw); });
}

// ---- graduated non-convexity (gnc.h) ----
void dpgo_gnc_options_default(dpgo_gnc_options_t *opt) {
  if (!opt) return;
  const dpgo::GncOptions o;
  opt->kind = o.kind; opt->barc2 = o.barc2; opt->mu_step = o.mu_step; opt->max_levels = o.max_levels;
  dpgo_polish_options_default(&opt->inner);
}

static void to_c(const dpgo::GncResult &r, dpgo_gnc_result_t *result) {
  result->outcome = r.outcome; result->levels = r.levels; result->steps = r.steps; result->factorisations = r.factorisations;
  result->inner_outcome = r.inner_outcome; result->mu_initial = r.mu_initial; result->mu_final = r.mu_final;
  result->s_max_initial = r.s_max_initial; result->F_initial = r.F_initial; result->F_weighted_final = r.F_weighted_final;
  result->F_surrogate_final = r.F_surrogate_final; result->num_robust = r.num_robust; result->num_zero = r.num_zero;
  result->num_one = r.num_one; result->num_between = r.num_between; result->num_outliers = r.num_outliers;
  result->device_bytes = r.device_bytes; result->symbolic_s = r.symbolic_s; result->total_ms = r.total_ms;
  result->edge_ms = r.edge_ms; result->inner_ms = r.inner_ms;
}

static dpgo::GncOptions to_cpp(const dpgo_gnc_options_t *opt) {
  dpgo::GncOptions o;
  if (opt) {
    o.kind = opt->kind; o.barc2 = opt->barc2; o.mu_step = opt->mu_step; o.max_levels = opt->max_levels;
    o.inner = to_cpp(&opt->inner); o.anchor = opt->inner.anchor;
  }
  return o;
}

int dpgo_group_gnc(dpgo_group_t *h, const dpgo_graph_t *g, const double *X, int ld, const dpgo_gnc_options_t *opt,
                   const int *robust_set, long long max_bytes, double *Xout, int ldout, double *weights, double *log, int log_cap,
                   dpgo_gnc_result_t *result) {
  if (!h || !h->grp || !g || !X || !Xout || !weights || !result || log_cap < 0 || (log_cap > 0 && !log)) return -1;
  return guarded([&] {
    const dpgo::GncOptions o = to_cpp(opt);
    dpgo::GncResult r;
    const int rc = h->grp->gnc(g->g, X, ld, o, robust_set, max_bytes, Xout, ldout, weights, log, log_cap, r);
    to_c(r, result);
    return rc;
  });
}

// ---- graduated non-convexity on the maximum-likelihood objective (ml_gnc.h) ----
int dpgo_group_ml_gnc(dpgo_group_t *h, const dpgo_graph_t *g, const double *X, int ld, const dpgo_gnc_options_t *opt,
                      const int *robust_set, long long max_bytes, double *Xout, int ldout, double *weights, double *log, int log_cap,
                      dpgo_ml_gnc_result_t *result) {
  if (!h || !h->grp || !g || !X || !Xout || !weights || !result || log_cap < 0 || (log_cap > 0 && !log)) return -1;
  return guarded([&] {
    dpgo::MlGncResult r;
    const int rc = h->grp->ml_gnc(g->g, X, ld, to_cpp(opt), robust_set, max_bytes, Xout, ldout, weights, log, log_cap, r);
    to_c(r, &result->gnc);
    result->near_pi = r.near_pi;
    result->near_pi_all = r.near_pi_all;
    return rc;
  });
}

// ---- the Riemannian staircase (stair.h) ----
void dpgo_staircase_options_default(dpgo_staircase_options_t *opt) {
  if (!opt) return;
  const dpgo::StairOptions o;
  opt->grad_norm_tol = o.grad_norm_tol; opt->preconditioned_grad_norm_tol = o.preconditioned_grad_norm_tol;
  opt->rel_func_decrease_tol = o.rel_func_decrease_tol; opt->stepsize_tol = o.stepsize_tol;
  opt->max_iterations = o.max_iterations; opt->max_tCG_iterations = o.max_tCG_iterations;
  opt->STPCG_kappa = o.STPCG_kappa; opt->STPCG_theta = o.STPCG_theta; opt->r_max = o.r_max; opt->precondition = o.precondition;
  opt->polish = o.polish; opt->reserved = 0; opt->min_eig_num_tol = o.min_eig_num_tol; opt->max_factor_bytes = o.max_factor_bytes;
}

int dpgo_group_staircase(dpgo_group_t *h, const double *X, int ld, const dpgo_staircase_options_t *opt, long long max_bytes,
                         double *Xhat, int ldx, double *Y, int ldy, double *log, int log_cap, dpgo_staircase_result_t *result) {
  if (!h || !h->grp || !X || !Xhat || !result || log_cap < 0 || (log_cap > 0 && !log)) return -1;
  return guarded([&] {
    dpgo::StairOptions o;
    if (opt) {
      o.grad_norm_tol = opt->grad_norm_tol; o.preconditioned_grad_norm_tol = opt->preconditioned_grad_norm_tol;
      o.rel_func_decrease_tol = opt->rel_func_decrease_tol; o.stepsize_tol = opt->stepsize_tol;
      o.max_iterations = opt->max_iterations; o.max_tCG_iterations = opt->max_tCG_iterations;
      o.STPCG_kappa = opt->STPCG_kappa; o.STPCG_theta = opt->STPCG_theta; o.r_max = opt->r_max; o.precondition = opt->precondition;
      o.polish = opt->polish; o.min_eig_num_tol = opt->min_eig_num_tol; o.max_factor_bytes = opt->max_factor_bytes;
    }
    dpgo::StairResult r;
    const int rc = h->grp->staircase(X, ld, o, max_bytes, Xhat, ldx, Y, ldy, log, log_cap, r);
    result->outcome = r.outcome; result->cert_status = r.cert_status; result->final_rank = r.final_rank; result->levels = r.levels;
    result->tnt_iterations = r.tnt_iterations; result->hess_products = r.hess_products;
    result->replaced_by_input = r.replaced_by_input; result->polish_outcome = r.polish_outcome; result->theta = r.theta;
    result->stationarity = r.stationarity; result->F_initial = r.F_initial; result->F_sdp = r.F_sdp;
    result->F_rounded = r.F_rounded; result->F_final = r.F_final; result->gap = r.gap;
    for (int i = 0; i < 6; i++) result->sigma[i] = r.sigma[i];
    result->device_bytes = r.device_bytes; result->optimise_ms = r.optimise_ms; result->verify_ms = r.verify_ms;
    result->round_ms = r.round_ms; result->total_ms = r.total_ms;
    return rc;
  });
}

int dpgo_group_stair_eval(dpgo_group_t *h, const double *Y, int ldy, double *F, double *grad_norm, double *Lambda, double *grad,
                          int ldg) {
  if (!h || !h->grp || !Y || !F || !grad_norm) return -1;
  return guarded([&] { return h->grp->stair_eval(Y, ldy, F, grad_norm, Lambda, grad, ldg); });
}
int dpgo_group_stair_hess(dpgo_group_t *h, const double *Y, int ldy, const double *V, int ldv, double *out, int ldo) {
  if (!h || !h->grp || !Y || !V || !out) return -1;
  return guarded([&] { return h->grp->stair_hess(Y, ldy, V, ldv, out, ldo); });
}
int dpgo_group_stair_retract(dpgo_group_t *h, const double *Y, int ldy, const double *V, int ldv, double *Z, int ldz) {
  if (!h || !h->grp || !Y || !V || !Z) return -1;
  return guarded([&] { return h->grp->stair_retract(Y, ldy, V, ldv, Z, ldz); });
}
int dpgo_group_stair_round(dpgo_group_t *h, const double *Y, int ldy, double *B, double *sigma, double *Xhat, int ldx) {
  if (!h || !h->grp || !Y || !B || !sigma || !Xhat) return -1;
  return guarded([&] { return h->grp->stair_round(Y, ldy, B, sigma, Xhat, ldx); });
}

}  // extern "C"
