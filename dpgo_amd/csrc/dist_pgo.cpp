// dist_pgo -- command-line driver with the reference's flags and outputs, on top of the C ABI.
//
// Mirrors C++/examples/dist_pgo.cpp:
//   flags      --dataset --num_nodes --iters[1000] --dist_init[true] --loss[trivial|huber|welsch]
//              --accelerated[true] --save[true]                                     (:23-47)
//   options    the hard-coded overrides of :103-120 (dpgo_options_driver)
//   loop       iterate -> gather -> communicate -> update, timing iterate + update only (:492-531)
//   stdout     "<iter>: <fobj> <grad>" with 20 digits, then the final summary         (:493-494, 533-536)
//   files      results_chordal_<N>_<amm|mm>.txt  (iter time fobj grad, 16 digits)     (:538-552)
//              estimates_<loss>.txt  (X with t <- t - t_0, X <- X R_0)                (:554-567)
// One process hosts all nodes on one GPU (--gpu), or -- one process per GPU -- rank r of n (--rank / --world, or
// RANK / WORLD_SIZE / LOCAL_RANK from a launcher) hosts nodes [r num_nodes / n, (r + 1) num_nodes / n) and the
// boundary poses travel by RCCL (dpgo_comm_exchange); the 128-byte RCCL id goes from rank 0 to the others through
// the private directory --rdv (default: named after the launcher's run id / MASTER_PORT) with a nonce handshake.  fobj = 2 F and grad = 2 |grad F| come from the per-node
// device reductions (sum_a fobj^a = F, sum_a |Proj(Dfobj^a)|^2 = |grad F|^2; DPGOStar.cpp:713-829), summed over
// the ranks.
// --dist_init true runs the distributed chordal initialisation (:144-416, C++/DChordal) through
// dpgo_group_dist_chordal_initialization and prints the stage objectives the reference prints every 20
// iterations (:206-210); its stage 0 (a per-node SE-Sync solve in the reference) is the library's stand-in.
// --dist_init false is the centralised chordal initialisation (:416-444).
//
// The flags below are not in the reference's driver; off, every output is as without them.  Each is one step after the loop
// and the summary, documented above its function; main() runs the steps in this order, each on the point the ones before it left:
//   --gnc tls|gm [--gnc_barc2 V] [--gnc_report FILE] [--gnc_filtered FILE]                          step_gnc
//   --polish                                                                                        step_polish
//   --hessian_modes K --modes_report FILE [--modes_escape]                                          step_modes
//   --staircase                                                                                     step_staircase
//   --robust_polish                                                                                 step_robust_polish
//   --ml_polish                                                                                     step_ml_polish
//   --ml_gnc tls|gm [--ml_gnc_barc2 V] [--ml_gnc_report FILE]                                       step_ml_gnc
//   --certify                                                                                       step_certify
//   --verify                                                                                        step_verify
//   --edge_report FILE, --verify_reweighted                                                         step_edges
//   --covariance FILE                                                                               step_covariance
//   --robust_covariance FILE                                                                        step_robust_covariance
//   --ml_covariance FILE, --ml_report FILE                                                          step_ml_covariance, step_ml_report
//   --ml_edge_reliability FILE                                                                      step_ml_reliability
//   --ml_gate_candidates FILE --ml_gate_report FILE                                                 step_ml_gate
//   --gate_candidates FILE --gate_report FILE                                                       step_gate
//   --sensitivity_pose P --sensitivity_report FILE                                                  step_sensitivity
//   --edge_reliability FILE                                                                         step_reliability
//   --marginal_set FILE --marginal_report FILE [--marginal_base P]                                  step_marginal
//   --select_candidates FILE --select_report FILE [--select_budget K] [--select_d2_max V]           step_candidates
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include <unistd.h>

#include "../../include/dpgo_amd.h"
#include "dist_pgo_report.h"
#include "rdv.h"

using namespace report;

// ---------------------------------------------------------------- arguments

struct Args {
  std::string dataset, loss_type = "trivial", rdv;
  int num_nodes = -1, iters = 1000, gpu = -1, rank = 0, world = 1;
  int loss = 0;   // loss_type as the library's number
  bool dist_init = true, accelerated = true, save = true;
  // the steps after the loop
  std::string gnc, gnc_report, gnc_filtered, modes_report, edge_report, covariance, robust_covariance, gate_candidates, gate_report,
      sensitivity_report, edge_reliability, marginal_set, marginal_report, select_candidates, select_report, ml_covariance, ml_report,
      ml_gnc, ml_gnc_report, ml_edge_reliability, ml_gate_candidates, ml_gate_report;
  bool polish = false, modes_escape = false, staircase = false, robust_polish = false, ml_polish = false, certify = false,
       verify = false, verify_reweighted = false;
  int hessian_modes = 0, sensitivity_pose = -1, marginal_base = -1, select_budget = -1;
  double gnc_barc2 = 4.0, select_d2_max = 0.0, ml_gnc_barc2 = 0.0;   // (ml_gnc_barc2 0: the chi2_dof quantile at 0.999)
};

static bool parse_bool(const char *s) { return !(strcmp(s, "false") == 0 || strcmp(s, "0") == 0); }

// One command-line flag: a switch is "--name" or "--name=BOOL" (never "--name BOOL"), every other kind "--name=V" or "--name V".
struct Flag {
  enum Kind { SWITCH, BOOL, INT, REAL, TEXT };
  const char *name;
  Kind kind;
  void *to;
  void set(const char *v) const {
    switch (kind) {
      case SWITCH:
      case BOOL: *(bool *)to = parse_bool(v); break;
      case INT: *(int *)to = atoi(v); break;
      case REAL: *(double *)to = atof(v); break;
      case TEXT: *(std::string *)to = v; break;
    }
  }
};
static Flag on(const char *name, bool &to) { return {name, Flag::SWITCH, &to}; }
static Flag val(const char *name, bool &to) { return {name, Flag::BOOL, &to}; }
static Flag val(const char *name, int &to) { return {name, Flag::INT, &to}; }
static Flag val(const char *name, double &to) { return {name, Flag::REAL, &to}; }
static Flag val(const char *name, std::string &to) { return {name, Flag::TEXT, &to}; }

static const char *const HELP =
    "Program options:\n  --dataset arg\n  --num_nodes arg\n  --iters arg (=1000)\n  --dist_init arg (=true)\n"
    "  --loss arg (=trivial)   trivial, huber or welsch\n  --accelerated arg (=true)\n  --save arg (=true)\n  --gpu arg (=0)\n"
    "  --robust_polish         robust loss, one rank: Newton polish of the robust objective after the loop; builds a second,\n"
    "                          trivial-loss group of the graph (seconds of set-up at 100 000 poses)\n"
    "  --robust_covariance arg likewise: marginal covariances on the robust Hessian, written to the file named\n"
    "  --gnc arg               tls or gm, one rank: graduated non-convexity after the loop (outlier rejection on the inter-node\n"
    "                          edges); --gnc_barc2 arg (=4) the inlier threshold, --gnc_report arg / --gnc_filtered arg its files\n"
    "  --edge_reliability arg  trivial loss, one rank, behind --polish: redundancy and leave-one-out chi-square of every edge,\n"
    "                          written to the file named\n"
    "  --marginal_set arg      trivial loss, one rank: a file of pose ids, one per line; with --marginal_report arg the joint\n"
    "                          covariance, information matrix and log-determinant of that set at the final point are written\n"
    "                          there; --marginal_base arg: a member of the set, for the relative form\n"
    "  --select_candidates arg trivial loss, one rank: a .g2o of candidate edges; with --select_report arg their joint\n"
    "                          compatibility and the greedy choice of --select_budget arg (= all) of them by information\n"
    "                          gain, gated by --select_d2_max arg (= 0: no gate), are written there\n"
    "  --hessian_modes arg     trivial loss, one rank: the arg (1 ... 60) smallest eigenpairs of the anchored Hessian at the\n"
    "                          final point (behind --polish: the polished one), written to --modes_report arg; with\n"
    "                          --modes_escape a lower point along the most negative mode replaces the point\n";

// Fills `a` from the launcher's environment and the command line, then checks it.  0: go on; 1: --help was printed; -1: an error was.
// An unknown argument is ignored, and so is a value flag that is the last argument; a later occurrence of a flag wins.
static int parse_args(int argc, char **argv, Args &a) {
  const Flag flags[] = {
      val("--dataset", a.dataset), val("--num_nodes", a.num_nodes), val("--iters", a.iters), val("--dist_init", a.dist_init),
      val("--loss", a.loss_type), val("--accelerated", a.accelerated), val("--save", a.save), val("--gpu", a.gpu), val("--rank", a.rank),
      val("--world", a.world), val("--rdv", a.rdv),
      val("--gnc", a.gnc), val("--gnc_barc2", a.gnc_barc2), val("--gnc_report", a.gnc_report), val("--gnc_filtered", a.gnc_filtered),
      on("--polish", a.polish), val("--hessian_modes", a.hessian_modes), val("--modes_report", a.modes_report),
      on("--modes_escape", a.modes_escape), on("--staircase", a.staircase), on("--robust_polish", a.robust_polish),
      on("--certify", a.certify), on("--verify", a.verify), val("--edge_report", a.edge_report),
      on("--verify_reweighted", a.verify_reweighted), val("--covariance", a.covariance), val("--robust_covariance", a.robust_covariance),
      val("--gate_candidates", a.gate_candidates), val("--gate_report", a.gate_report), val("--sensitivity_pose", a.sensitivity_pose),
      val("--sensitivity_report", a.sensitivity_report), val("--edge_reliability", a.edge_reliability),
      val("--marginal_set", a.marginal_set), val("--marginal_report", a.marginal_report), val("--marginal_base", a.marginal_base),
      val("--select_candidates", a.select_candidates), val("--select_report", a.select_report), val("--select_budget", a.select_budget),
      val("--select_d2_max", a.select_d2_max), on("--ml_polish", a.ml_polish), val("--ml_covariance", a.ml_covariance),
      val("--ml_report", a.ml_report), val("--ml_gnc", a.ml_gnc), val("--ml_gnc_barc2", a.ml_gnc_barc2),
      val("--ml_gnc_report", a.ml_gnc_report), val("--ml_edge_reliability", a.ml_edge_reliability),
      val("--ml_gate_candidates", a.ml_gate_candidates), val("--ml_gate_report", a.ml_gate_report)};
  if (getenv("RANK")) a.rank = atoi(getenv("RANK"));
  if (getenv("WORLD_SIZE")) a.world = atoi(getenv("WORLD_SIZE"));
  for (int i = 1; i < argc; i++) {
    const std::string s = argv[i];
    if (s == "--help") {
      fputs(HELP, stdout);
      return 1;
    }
    for (const Flag &f : flags) {
      const size_t n = strlen(f.name);
      const char *v = nullptr;
      if (s.compare(0, n, f.name) == 0 && s.size() > n && s[n] == '=') v = argv[i] + n + 1;
      else if (s == f.name && f.kind == Flag::SWITCH) v = "true";
      else if (s == f.name && i + 1 < argc) v = argv[++i];
      if (v) {
        f.set(v);
        break;
      }
    }
  }
  if (a.gpu < 0) a.gpu = getenv("LOCAL_RANK") ? atoi(getenv("LOCAL_RANK")) : (a.world > 1 ? a.rank : 0);
  if (a.world < 1 || a.rank < 0 || a.rank >= a.world) { fprintf(stderr, "Inconsistent --rank / --world.\n"); return -1; }
  if (a.world > 1 && a.rdv.empty()) {
    // a name all ranks of this launch -- and no other launch -- agree on: the launcher's run id / port
    const char *run = getenv("TORCHELASTIC_RUN_ID"), *port = getenv("MASTER_PORT");
    if (!run && !port) { fprintf(stderr, "Several ranks need --rdv <directory> (or a launcher that sets MASTER_PORT).\n"); return -1; }
    a.rdv = std::string("/tmp/dpgo_rdv_") + std::to_string((long)geteuid()) + "_" + (run ? run : "none") + "_" + (port ? port : "0");
  }
  if (a.dataset.empty()) { fprintf(stderr, "No dataset has been specfied.\n"); return -1; }
  if (a.num_nodes < 1) { fprintf(stderr, "No number of nodes has been specfied.\n"); return -1; }
  if (a.loss_type == "trivial") a.loss = 0;
  else if (a.loss_type == "huber") a.loss = 1;
  else if (a.loss_type == "welsch") a.loss = 3;
  else { fprintf(stderr, " The loss type can only be \"trivial\", \"huber\" or \"welsch\".\n"); return -1; }
  return 0;
}

// ---------------------------------------------------------------- the run

enum Loss { ANY_LOSS, TRIVIAL_LOSS, ROBUST_LOSS };
enum { ANYWHERE = 0, BEHIND_POLISH = 1 };

// What every part of a run shares.  No destructor: an error leaves without freeing (with several ranks a dpgo_comm_free on one
// rank's error path could block); main() frees at its end.
struct Run {
  const Args &a;   // (with loss, loss_type and world)
  dpgo_graph_t *g = nullptr;
  dpgo_group_t *grp = nullptr;
  dpgo_group_t *post = nullptr;   // see post_group()
  dpgo_comm_t *comm = nullptr;
  dpgo_options_t opt;
  int d = 0, N = 0, nn = 0, graph_edges = 0, ld = 0, dof = 0, per = 0;
  bool root = true;
  std::vector<int> ids;          // the nodes this rank hosts
  std::vector<double> Xnow;      // the point a step after the loop has put in the optimiser's place (empty: none has)
  std::vector<int> I, J;         // the graph's edges in file order, and whether each joins two nodes: see load_edges()
  std::vector<unsigned char> inter;
  dpgo_graph_t *ml_kept = nullptr;   // behind --ml_gnc: the graph without the edges of weight 0, for --ml_covariance / --ml_report
  std::vector<int> ml_kept_edges;    // their numbers in the graph

  // the graph the maximum-likelihood covariance and report act on, and the graph's number of its edge e
  dpgo_graph_t *ml_graph() const { return ml_kept ? ml_kept : g; }
  int ml_edges() const { return ml_kept ? (int)ml_kept_edges.size() : graph_edges; }
  int ml_edge(int e) const { return ml_kept ? ml_kept_edges[e] : e; }

  explicit Run(const Args &args) : a(args) {}

  size_t point_size() const { return (size_t)ld * d; }

  // the point every later step acts on: the optimiser's, or the one a step (gnc, a polish, an escape, the staircase) left
  int final_point(double *out) {
    if (!Xnow.empty()) {
      std::copy(Xnow.begin(), Xnow.end(), out);
      return 0;
    }
    return dpgo_group_scatter_global(grp, out, ld);
  }
  int point(std::vector<double> &Xc) {
    Xc.assign(point_size(), 0.0);
    return final_point(Xc.data());
  }

  // the robust objective and graduated non-convexity: a trivial-loss group of the same graph, built once for all their flags
  int post_group() {
    if (post) return 0;
    dpgo_options_t po;
    dpgo_options_driver(&po, 0, a.accelerated);
    po.max_iterations = 0;
    return dpgo_group_create(g, ids.data(), per, &po, a.gpu, &post);
  }

  // The one place a step says why it is not computed.  Every such step needs the group to host every node; `need` is the loss
  // it is defined for, `word` what is the trivial loss's (TRIVIAL_LOSS) or the flag that is the call instead (ROBUST_LOSS);
  // BEHIND_POLISH: it is taken at a critical point.  Asked in this order: loss, ranks, polish.
  bool refused(const char *label, Loss need = ANY_LOSS, const char *word = "", int where = ANYWHERE) const {
    if (need == TRIVIAL_LOSS && a.loss != 0) {
      if (root) printf("%s: not computed (the %s is that of the trivial loss; --loss %s)\n", label, word, a.loss_type.c_str());
    } else if (need == ROBUST_LOSS && a.loss == 0) {
      if (root) printf("%s: not computed (the loss is trivial: %s is the call)\n", label, word);
    } else if (a.world > 1) {
      if (root) printf("%s: not computed (the group must host every node; %d ranks)\n", label, a.world);
    } else if (where == BEHIND_POLISH && !a.polish) {
      if (root) printf("%s: not computed (it is taken at a critical point: --polish)\n", label);
    } else {
      return false;
    }
    return true;
  }

  // The graph's edge list, read on first use.  inter[e]: the edge joins two nodes -- the partition's flag, from the node ranges
  // (the weight of an intra-node edge is 1 by definition).  A pose belongs to the last node whose first pose is not behind it;
  // first[a] is -1 for a node without an edge.  (Walking up while dpgo_graph_node_offset(g, a + 1) <= p numbers the nodes
  // differently past such a node, but a node without an edge owns no pose, so both maps are injective on the nodes that do and
  // "the two ends lie in different nodes" is the same under either.)
  int load_edges() {
    if (!inter.empty() || graph_edges == 0) return 0;
    I.resize(graph_edges);
    J.resize(graph_edges);
    if (dpgo_graph_edges(g, I.data(), J.data(), nullptr, nullptr, nullptr, nullptr) != 0) return -1;
    std::vector<int> first(nn);
    for (int n = 0; n < nn; n++) first[n] = dpgo_graph_node_offset(g, n);
    auto node_of = [&](int p) {
      int r = 0;
      for (int n = 0; n < nn; n++)
        if (first[n] >= 0 && p >= first[n]) r = n;
      return r;
    };
    inter.resize(graph_edges);
    for (int e = 0; e < graph_edges; e++) inter[e] = node_of(I[e]) != node_of(J[e]) ? 1 : 0;
    return 0;
  }

  void evaluate(double &fobj, double &grad) {
    double v[2] = {0, 0};
    for (int n = 0; n < per; n++) {
      dpgo_results_t r;
      dpgo_group_results(grp, n, &r);
      v[0] += r.fobj;
      v[1] += r.gradFnorm * r.gradFnorm;
    }
    if (comm) dpgo_comm_allreduce_sum(comm, v, 2);
    fobj = 2 * v[0];
    grad = 2 * std::sqrt(v[1]);
  }
};

// load the graph, build this rank's group and, with several ranks, the communicator
static int setup(Run &r) {
  const Args &a = r.a;
  if (dpgo_read_g2o(a.dataset.c_str(), a.num_nodes, &r.g) != 0) return -1;
  dpgo_graph_info(r.g, &r.d, &r.N, &r.nn, &r.graph_edges);
  dpgo_options_driver(&r.opt, a.loss, a.accelerated);
  r.ld = (r.d + 1) * r.N;
  r.dof = r.d + r.d * (r.d - 1) / 2;
  if (a.num_nodes % a.world != 0) { fprintf(stderr, "The number of nodes must be a multiple of the number of ranks.\n"); return -1; }
  r.per = a.num_nodes / a.world;
  r.ids.resize(r.per);
  for (int n = 0; n < r.per; n++) r.ids[n] = a.rank * r.per + n;
  r.root = a.rank == 0;
  if (dpgo_group_create(r.g, r.ids.data(), r.per, &r.opt, a.gpu, &r.grp) != 0) return -1;
  if (a.world > 1 || getenv("DPGO_FORCE_COMM")) {   // (DPGO_FORCE_COMM: a world of one rank still runs the whole protocol)
    unsigned char id[128];
    if (r.root && dpgo_comm_unique_id(id) != 0) return -1;
    if (a.world > 1 && dpgo_rdv::rendezvous(a.rdv, a.rank, a.world, id) != 0) return -1;
    if (dpgo_comm_create(r.grp, a.rank, a.world, id, &r.comm) != 0) return -1;
    dpgo_comm_barrier(r.comm);
  }
  return 0;
}

// the chordal initialisation, distributed or centralised, into X and from there into the group
static int initialise(Run &r, std::vector<double> &X) {
  X.assign(r.point_size(), 0.0);
  if (r.a.dist_init) {
    // every node of the graph takes part in the distributed initialisation; with several ranks each runs the schedule
    // for its own nodes and the stage halos travel through the communicator (dchordal.cpp)
    dpgo_dchordal_options_t co;
    dpgo_dchordal_options_default(&co);
    int cap = 0;
    for (int k = 0; k < 4; k++) cap += (co.iters[k] + 19) / 20;
    std::vector<double> obj(cap);
    if (dpgo_group_dist_chordal_initialization(r.grp, &co, nullptr, 0, X.data(), r.ld, obj.data(), &cap) != 0) return -1;
    const char *names[4] = {"Initialize the reduced rotation", "Initialize the rotation", "Initialize the reduced translation",
                            "Initialize the translation"};
    int at = 0;
    for (int k = 0; k < 4 && r.root; k++) {
      printf("===============================================\n%s\n-----------------------------------------------\n", names[k]);
      for (int it = 0; it < co.iters[k]; it += 20) printf("%d: %.16g\n", it, obj[at++]);
    }
  } else {
    if (r.root) printf("===============================================\nInitialization\n-----------------------------------------------\n");
    if (dpgo_chordal_initialization(r.g, X.data(), r.ld) != 0) return -1;
  }
  if (dpgo_group_initialize_global(r.grp, X.data(), r.ld) != 0) return -1;
  return dpgo_group_update(r.grp, nullptr, 0) != 0 ? -1 : 0;
}

// the loop and the summary; results gets one row (iter time fobj grad) per evaluation
static int solve(Run &r, std::vector<std::vector<double>> &results) {
  double fobj, grad, time = 0;
  r.evaluate(fobj, grad);
  results.push_back({0, 0, fobj, grad});
  if (r.root) printf("===============================================\nDistributed PGO\n-----------------------------------------------\n");
  using clk = std::chrono::steady_clock;
  for (int iter = 0; iter < r.a.iters; iter++) {
    if (r.root) printf("%d: %.20g %.20g\n", iter, fobj, grad);
    auto t0 = clk::now();
    if (dpgo_group_iterate(r.grp, nullptr, 0) != 0) return -1;
    dpgo_group_sync(r.grp);
    time += std::chrono::duration<double>(clk::now() - t0).count();
    if (r.comm && dpgo_comm_exchange(r.comm) != 0) return -1;   // neighbours on other GPUs: RCCL, joined by update()
    dpgo_group_communicate_local(r.grp);
    t0 = clk::now();
    if (dpgo_group_update(r.grp, nullptr, 0) != 0) return -1;
    dpgo_group_sync(r.grp);
    time += std::chrono::duration<double>(clk::now() - t0).count();
    r.evaluate(fobj, grad);
    results.push_back({double(iter) + 1, time, fobj, grad});
  }
  if (r.root)
    printf("---------------------------------------\nfinal objective: %.20g\nfinal gradient: %.20g\ntime: %.20g s/node.\n", fobj,
           grad, time / r.per);
  return 0;
}

// the result files: the iteration table, and the final point in the gauge of pose 0
static int save(Run &r, std::vector<double> &X, const std::vector<std::vector<double>> &results) {
  const int d = r.d, ld = r.ld, N = r.N;
  std::fill(X.begin(), X.end(), 0.0);
  r.final_point(X.data());
  if (r.comm) dpgo_comm_allreduce_sum(r.comm, X.data(), (long)X.size());   // every rank contributes its own poses
  if (!r.root) return 0;
  const std::string resfile = "results_chordal_" + std::to_string(r.a.num_nodes) + "_" + (r.a.accelerated ? "amm" : "mm") + ".txt";
  FILE *f = fopen(resfile.c_str(), "w");
  if (!f) return -1;
  for (const auto &row : results) fprintf(f, "%d %.16g %.16g %.16g\n", (int)row[0], row[1], row[2], row[3]);
  fclose(f);
  // gauge fix (:554-558): t <- t - t_0 ; X <- X * R with R = X.middleRows(num_poses, d)^T
  std::vector<double> R(d * d), t0v(d);
  for (int c = 0; c < d; c++) {
    t0v[c] = X[(size_t)c * ld + 0];
    for (int k = 0; k < d; k++) R[k * d + c] = X[(size_t)k * ld + N + c];   // R(k,c) = block(c,k)
  }
  for (int i = 0; i < N; i++)
    for (int c = 0; c < d; c++) X[(size_t)c * ld + i] -= t0v[c];
  f = fopen(("./estimates_" + r.a.loss_type + ".txt").c_str(), "w");
  if (!f) return -1;
  std::vector<double> row(d);
  for (int i = 0; i < ld; i++) {
    for (int c = 0; c < d; c++) {
      double s = 0;
      for (int k = 0; k < d; k++) s += X[(size_t)k * ld + i] * R[k * d + c];
      row[c] = s;
    }
    for (int c = 0; c < d; c++) fprintf(f, "%s%g", c ? " " : "", row[c]);
    fprintf(f, "\n");
  }
  fclose(f);
  return 0;
}

// ---------------------------------------------------------------- the steps after the loop
// Each returns 0 when it is off, refused or done, and -1 after an error (main() then returns -1).

// --gnc tls|gm (likewise; empty: off) --gnc_barc2 V (default 4)  after the loop and ahead of --polish / --staircase /
// --certify / --verify / --covariance and the robust flags, which then act on its point, for a world of one rank and any
// --loss: dpgo_group_gnc (graduated non-convexity, the inter-node edges as the robust set, pose 0 the anchor) on the
// second, trivial-loss group of --robust_polish, from the final X, and one more line on stdout
//     gnc: <outcome> <levels> <steps> <factorisations> <num_robust> <num_zero> <num_between> <num_outliers>
//          <mu_initial> <mu_final> <F_initial> <F_weighted_final> <F_surrogate_final>
// the result files then hold its point.  --gnc_report FILE: one line per edge, "i j in_R w s" (17 digits), s at that
// point; --gnc_filtered FILE: the graph without the edges of weight 0 (dpgo_graph_filter_edges) with that point, as a
// .g2o (dpgo_write_g2o).  With several ranks a line that says why not
static int step_gnc(Run &r) {
  const Args &a = r.a;
  if (a.gnc.empty()) return 0;
  if (a.gnc != "tls" && a.gnc != "gm") {
    fprintf(stderr, "--gnc takes tls or gm.\n");
    return -1;
  }
  if (r.refused("gnc")) return 0;
  const int m = r.graph_edges, ld = r.ld;
  std::vector<double> Xc, Z(r.point_size(), 0.0), w(m, 1.0);
  dpgo_gnc_options_t go;
  dpgo_gnc_options_default(&go);
  go.kind = a.gnc == "tls" ? DPGO_GNC_TLS : DPGO_GNC_GM;
  go.barc2 = a.gnc_barc2;
  dpgo_gnc_result_t gr;
  if (r.point(Xc) != 0 || r.post_group() != 0 ||
      dpgo_group_gnc(r.post, r.g, Xc.data(), ld, &go, nullptr, 0, Z.data(), ld, w.data(), nullptr, 0, &gr) != 0)
    return -1;
  printf("gnc: %s %d %d %d %d %d %d %d %.17g %.17g %.17g %.17g %.17g\n", gnc_name(gr.outcome), gr.levels, gr.steps, gr.factorisations,
         gr.num_robust, gr.num_zero, gr.num_between, gr.num_outliers, gr.mu_initial, gr.mu_final, gr.F_initial, gr.F_weighted_final,
         gr.F_surrogate_final);
  if (gr.outcome == DPGO_GNC_SKIPPED) return 0;
  if (!a.gnc_report.empty()) {
    std::vector<double> sr(m), st(m), wb(m), sums(8);
    if (r.load_edges() != 0 ||
        dpgo_group_gnc_eval(r.post, r.g, Z.data(), ld, go.kind, gr.mu_final > 0 ? gr.mu_final : 1.0, go.barc2, nullptr, w.data(), sr.data(),
                            st.data(), wb.data(), sums.data()) != 0)
      return -1;
    FILE *f = open_report(a.gnc_report.c_str());
    if (!f) return -1;
    for (int e = 0; e < m; e++) fprintf(f, "%d %d %d %.17g %.17g\n", r.I[e], r.J[e], (int)r.inter[e], w[e], sr[e] + st[e]);
    fclose(f);
  }
  if (!a.gnc_filtered.empty()) {
    std::vector<unsigned char> keep(m);
    for (int e = 0; e < m; e++) keep[e] = w[e] != 0.0;
    dpgo_graph_t *kept = nullptr;
    if (dpgo_graph_filter_edges(r.g, keep.data(), &kept) != 0) return -1;
    const int rc = dpgo_write_g2o(kept, Z.data(), ld, a.gnc_filtered.c_str());
    dpgo_graph_free(kept);
    if (rc != 0) return -1;
  }
  r.Xnow.swap(Z);
  return 0;
}

// --polish (likewise)  after the loop and ahead of --certify / --verify / --covariance, which then act on the polished
// point, for the trivial loss and a world of one rank: dpgo_group_polish (damped Riemannian Newton steps, pose 0
// the anchor) from the final X, and one more line on stdout
//     polish: <outcome> <steps> <factorisations> <indefinite> <F_initial> <F_final> <grad_initial> <grad_final>
// the result files then hold the polished X; the same reasons as --covariance when it is not computed
// --robust_polish (likewise)  after the loop and ahead of --edge_report / --verify_reweighted / --robust_covariance, which
// then act on its point, for a robust --loss and a world of one rank: dpgo_group_robust_polish (the Newton polish of
// the robust objective on its true Hessian, pose 0 the anchor) on a second, trivial-loss group of the same graph
// built for it (max_iterations = 0; seconds of set-up at 100 000 poses), one more line on stdout
//     robust polish: <the fields of polish:>
// with the F fields those of the robust objective; the result files then hold the polished X; with the trivial loss
// (--polish is the call then) or several ranks a line "robust polish: not computed (...)" that says why not
static int newton_polish(Run &r, bool robust) {
  const char *label = robust ? "robust polish" : "polish";
  if (robust ? r.refused(label, ROBUST_LOSS, "--polish") : r.refused(label, TRIVIAL_LOSS, "Hessian")) return 0;
  std::vector<double> Xc, Z(r.point_size(), 0.0);
  dpgo_polish_result_t pr;
  if (r.point(Xc) != 0) return -1;
  if (robust ? r.post_group() != 0 || dpgo_group_robust_polish(r.post, r.g, Xc.data(), r.ld, r.a.loss, r.opt.loss_reg, 1, nullptr, 0, Z.data(),
                                                               r.ld, nullptr, 0, &pr, nullptr) != 0
             : dpgo_group_polish(r.grp, Xc.data(), r.ld, nullptr, 0, Z.data(), r.ld, nullptr, 0, &pr) != 0)
    return -1;
  printf("%s: %s %d %d %d %.17g %.17g %.17g %.17g\n", label, polish_name(pr.outcome), pr.steps, pr.factorisations, pr.indefinite,
         pr.F_initial, pr.F_final, pr.grad_initial, pr.grad_final);
  if (pr.outcome != DPGO_POLISH_SKIPPED) r.Xnow.swap(Z);
  return 0;
}
static int step_polish(Run &r) { return r.a.polish ? newton_polish(r, false) : 0; }
static int step_robust_polish(Run &r) { return r.a.robust_polish ? newton_polish(r, true) : 0; }

// --hessian_modes K --modes_report FILE [--modes_escape] (likewise; K and FILE both or neither)  behind --polish and
// ahead of --staircase / --certify / --verify / --covariance, for the trivial loss and a world of one rank:
// dpgo_group_hessian_modes (pose 0 the anchor) gives the K smallest eigenpairs of the anchored Hessian at the
// point so far -- at a saddle how negative the curvature is and along which poses, at a minimum 1 / lambda_0, the
// largest eigenvalue of the covariance.  The report (17 digits): a line "k <K> n <n> mu <mu> hmax <hmax>", then per
// pair a line "<j> <lambda_j> <residual_j> <the pose with the largest share of |v_j|^2> <that share>" and a line
// with the n entries of v_j; and one more line on stdout
//     modes: <outcome> <iterations> <factorisations> <shift_tries> <block> <negative> <lambda_0> <mu> <device_bytes> <escaped> <F> <F_escape>
// (STALLED or SKIPPED: the report is not written).  With --modes_escape and lambda_0 < 0 the lower point along
// v_0 becomes the point every later step acts on and the result files hold; "modes: not computed (...)" says why not
static int step_modes(Run &r) {
  const Args &a = r.a;
  if (a.hessian_modes == 0 && a.modes_report.empty()) return 0;
  if (a.hessian_modes == 0 || a.modes_report.empty()) {
    fprintf(stderr, "--hessian_modes and --modes_report go together.\n");
    return -1;
  }
  if (r.refused("modes", TRIVIAL_LOSS, "Hessian")) return 0;
  const int N = r.N, n = r.dof * N, k = a.hessian_modes, kk = std::max(k, 1);
  std::vector<double> Xc, Z(r.point_size(), 0.0), lam((size_t)kk), res((size_t)kk), vec((size_t)kk * n), en((size_t)kk * N);
  dpgo_modes_options_t mo;
  dpgo_modes_options_default(&mo);
  mo.want_escape = a.modes_escape ? 1 : 0;
  dpgo_modes_result_t mr;
  if (r.point(Xc) != 0 ||
      dpgo_group_hessian_modes(r.grp, Xc.data(), r.ld, 0, k, &mo, 0, lam.data(), res.data(), vec.data(), en.data(), Z.data(), &mr) != 0) {
    fprintf(stderr, "--hessian_modes takes 1 ... 60, at most dof (num_poses - 1).\n");
    return -1;
  }
  printf("modes: %s %d %d %d %d %d %.17g %.17g %lld %d %.17g %.17g\n", modes_name(mr.outcome), mr.iterations, mr.factorisations,
         mr.shift_tries, mr.block, mr.negative, lam[0], mr.mu, mr.device_bytes, mr.escaped, mr.F, mr.F_escape);
  if (mr.outcome == DPGO_MODES_CONVERGED || mr.outcome == DPGO_MODES_MAX_ITERS) {
    FILE *f = open_report(a.modes_report.c_str());
    if (!f) return -1;
    fprintf(f, "k %d n %d mu %.17g hmax %.17g\n", k, n, mr.mu, mr.hmax);
    for (int j = 0; j < k; j++) {
      const double *e = &en[(size_t)j * N];
      const int top = (int)(std::max_element(e, e + N) - e);
      fprintf(f, "%d %.17g %.17g %d %.17g\n", j, lam[j], res[j], top, e[top]);
      for (int i = 0; i < n; i++) fprintf(f, "%s%.17g", i ? " " : "", vec[(size_t)j * n + i]);
      fprintf(f, "\n");
    }
    fclose(f);
  }
  if (mr.escaped) r.Xnow.swap(Z);
  return 0;
}

// --staircase (likewise)  after --polish and ahead of --certify / --verify / --covariance, which then act on its
// result, for the trivial loss and a world of one rank: dpgo_group_staircase (the Riemannian staircase: TNT at rank
// r, verify, an escape along the certificate's direction, the rounding and a polish) from the point so far, and
// one more line on stdout
//     staircase: <outcome> <final_rank> <F_initial> <F_sdp> <F_final> <gap>
// the result files then hold its Xhat; the same reasons as --polish when it is not computed
static int step_staircase(Run &r) {
  if (!r.a.staircase || r.refused("staircase", TRIVIAL_LOSS, "relaxation")) return 0;
  std::vector<double> Xc, Z(r.point_size(), 0.0);
  dpgo_staircase_result_t sr;
  if (r.point(Xc) != 0 || dpgo_group_staircase(r.grp, Xc.data(), r.ld, nullptr, 0, Z.data(), r.ld, nullptr, 0, nullptr, 0, &sr) != 0)
    return -1;
  printf("staircase: %s %d %.17g %.17g %.17g %.17g\n", staircase_name(sr.outcome), sr.final_rank, sr.F_initial, sr.F_sdp, sr.F_final,
         sr.gap);
  if (sr.outcome != DPGO_STAIR_SKIPPED) r.Xnow.swap(Z);
  return 0;
}

// --certify (not in the reference's driver; off: every output is as without it)  after the loop, for the trivial
// loss and a world of one rank, one more line on stdout
//     certificate: <status> <theta> <residual> <iterations> <stationarity>
// from dpgo_group_certify (SESyncProblem::verify_solution, C++/SESync/src/SESyncProblem.cpp:397-468); with a
// robust loss or several ranks a line that says why not
static int step_certify(Run &r) {
  if (!r.a.certify || r.refused("certificate", TRIVIAL_LOSS, "certificate")) return 0;
  std::vector<double> Xc;
  dpgo_cert_options_t co;
  dpgo_cert_options_default(&co);
  dpgo_cert_result_t cr;
  if (r.point(Xc) != 0 || dpgo_group_certify(r.grp, Xc.data(), r.ld, &co, nullptr, 0, &cr, nullptr, 0) != 0) return -1;
  printf("certificate: %s %.16g %.16g %d %.16g\n", cert_status_name(cr.status), cr.theta, cr.residual, cr.iterations, cr.stationarity);
  return 0;
}

// the fields the two verifications print alike
static void print_verdict(const char *label, const dpgo_cert_result_t &cr, const dpgo_cert_factor_t &cf, const char *end) {
  printf("%s: %s %s %.16g %.16g %.16g %d %.16g%s", label, cert_status_name(cr.status), cert_factor_name(cf.outcome), cf.pivot_min, cr.theta,
         cr.residual, cr.iterations, cr.stationarity, end);
}

// --verify (likewise)  after the summary (and after --certify's line), one more line on stdout
//     verification: <status> <outcome> <pivot_min> <theta> <residual> <iterations> <stationarity>
// from dpgo_group_verify (fast_verification, C++/SESync/src/SESync_utils.cpp:721-830: the Cholesky factorisation
// of S + eta I first, the search only when it does not succeed); the same reasons when it is not computed
static int step_verify(Run &r) {
  if (!r.a.verify || r.refused("verification", TRIVIAL_LOSS, "certificate")) return 0;
  std::vector<double> Xc;
  dpgo_cert_options_t co;
  dpgo_cert_options_default(&co);
  dpgo_cert_result_t cr;
  dpgo_cert_factor_t cf;
  if (r.point(Xc) != 0 || dpgo_group_verify(r.grp, Xc.data(), r.ld, &co, 0, nullptr, 0, &cr, nullptr, 0, &cf) != 0) return -1;
  print_verdict("verification", cr, cf, "\n");
  return 0;
}

// --edge_report FILE (likewise; empty: off)  after the loop, one row per edge of the graph in file order,
//     edge i j inter s_rot s_trans rho weight        (16 digits)
// from dpgo_edge_eval_run at the final X with the run's loss: what the robust loss did to every measurement
// --verify_reweighted (likewise)  after the summary (and the lines above), one more line on stdout
//     reweighted verification: <status> <outcome> <pivot_min> <theta> <residual> <iterations> <stationarity>
//                              <num_downweighted>/<num_inter> <weight_min>
// from dpgo_graph_verify_reweighted: the certificate of the problem re-weighted by the loss weights at the
// final X (any loss); with several ranks a line that says why not
static int step_edges(Run &r) {
  const Args &a = r.a;
  if (a.edge_report.empty() && !a.verify_reweighted) return 0;
  if (a.world > 1) {
    if (r.root && !a.edge_report.empty())
      printf("edge report: not written (the edge evaluation needs the whole X on one rank; %d ranks)\n", a.world);
    if (a.verify_reweighted) r.refused("reweighted verification");
    return 0;
  }
  std::vector<double> Xc;
  if (r.point(Xc) != 0) return -1;
  if (!a.edge_report.empty()) {
    const int m = r.graph_edges;
    std::vector<double> sr(m), st(m), rho(m), w(m);
    dpgo_edge_eval_t *ev = nullptr;
    if (r.load_edges() != 0 || dpgo_edge_eval_create(r.g, a.gpu, &ev) != 0) return -1;
    const int rc = dpgo_edge_eval_run(ev, Xc.data(), r.ld, a.loss, r.opt.loss_reg, sr.data(), st.data(), rho.data(), w.data(), nullptr);
    dpgo_edge_eval_free(ev);
    if (rc != 0) return -1;
    FILE *f = open_report(a.edge_report.c_str());
    if (!f) return -1;
    for (int e = 0; e < m; e++)
      fprintf(f, "%d %d %d %d %.16g %.16g %.16g %.16g\n", e, r.I[e], r.J[e], (int)r.inter[e], sr[e], st[e], rho[e], w[e]);
    fclose(f);
  }
  if (a.verify_reweighted) {
    dpgo_cert_options_t co;
    dpgo_cert_options_default(&co);
    dpgo_cert_result_t cr;
    dpgo_cert_factor_t cf;
    dpgo_edge_summary_t es;
    if (dpgo_graph_verify_reweighted(r.g, a.gpu, Xc.data(), r.ld, a.loss, r.opt.loss_reg, &co, 0, &cr, &cf, &es, nullptr, 0) != 0) return -1;
    print_verdict("reweighted verification", cr, cf, "");
    printf(" %d/%d %.16g\n", es.num_downweighted, es.num_inter, es.weight_min);
  }
  return 0;
}

// --covariance FILE (likewise; empty: off)  after the summary (and the lines above), for the trivial loss and a
// world of one rank, one line per pose in FILE,
//     p  S[0][0] S[0][1] ... S[dof-1][dof-1]       (the upper triangle of Sigma_pp row by row, 17 digits)
// -- the marginal covariance of pose p relative to pose 0 from dpgo_group_covariance at the final X, tangent
// coordinates (translation in the world frame, rotation in the body frame) -- and one more line on stdout
//     covariance: <outcome> <unknowns> <fronts> <levels> <max_front> <device_bytes> <pivot_min> <stationarity>
// (NOT_PD or SKIPPED: FILE is not written); the same reasons as --certify when it is not computed
// --robust_covariance FILE (likewise; empty: off)  in --covariance's file format and with its line on stdout under
// the prefix "robust covariance:", from dpgo_group_robust_covariance at the final X
static int covariance(Run &r, bool robust, const std::string &file) {
  const char *label = robust ? "robust covariance" : "covariance";
  if (robust ? r.refused(label, ROBUST_LOSS, "--covariance") : r.refused(label, TRIVIAL_LOSS, "Hessian")) return 0;
  const int dof = r.dof;
  std::vector<double> Xc, marg((size_t)r.N * dof * dof, 0.0);
  dpgo_cov_result_t cv;
  if (r.point(Xc) != 0) return -1;
  if (robust ? r.post_group() != 0 || dpgo_group_robust_covariance(r.post, r.g, Xc.data(), r.ld, r.a.loss, r.opt.loss_reg, 1, 0, 0, nullptr, 0,
                                                                   marg.data(), nullptr, &cv) != 0
             : dpgo_group_covariance(r.grp, Xc.data(), r.ld, 0, 0, nullptr, 0, marg.data(), nullptr, &cv) != 0)
    return -1;
  printf("%s: %s %d %d %d %d %lld %.16g %.16g\n", label, cov_name(cv.outcome), cv.unknowns, cv.fronts, cv.levels, cv.max_front,
         cv.device_bytes, cv.pivot_min, cv.stationarity);
  if (cv.outcome != DPGO_COV_OK) return 0;
  FILE *f = open_report(file.c_str());
  if (!f) return -1;
  for (int p = 0; p < r.N; p++) {
    fprintf(f, "%d", p);
    write_upper(f, &marg[(size_t)p * dof * dof], dof);
    fprintf(f, "\n");
  }
  fclose(f);
  return 0;
}
static int step_covariance(Run &r) { return r.a.covariance.empty() ? 0 : covariance(r, false, r.a.covariance); }
static int step_robust_covariance(Run &r) { return r.a.robust_covariance.empty() ? 0 : covariance(r, true, r.a.robust_covariance); }

// The maximum-likelihood refinement on the file's full information matrices, for any --loss and a world of one rank; on the
// group that iterated for the trivial loss, on the second, trivial-loss group of --robust_polish otherwise.
static dpgo_group_t *ml_group(Run &r) {
  if (r.a.loss == 0) return r.grp;
  return r.post_group() == 0 ? r.post : nullptr;
}

// --ml_polish (likewise)  behind --polish / --robust_polish and ahead of every later step, which then acts on its point:
// dpgo_group_ml_polish (pose 0 the anchor) from the final X, and one more line on stdout
//     ml polish: <the fields of polish:> <chi2_initial> <chi2_final> <near_pi>
// with the F fields F_ml; the result files then hold the refined X; with several ranks a line that says why not
static int step_ml_polish(Run &r) {
  if (!r.a.ml_polish || r.refused("ml polish")) return 0;
  std::vector<double> Xc, Z(r.point_size(), 0.0);
  dpgo_ml_result_t mr;
  dpgo_group_t *grp = ml_group(r);
  if (!grp || r.point(Xc) != 0) return -1;
  if (dpgo_group_ml_polish(grp, r.g, Xc.data(), r.ld, nullptr, 0, Z.data(), r.ld, nullptr, 0, &mr) != 0) return -1;
  const dpgo_polish_result_t &pr = mr.polish;
  printf("ml polish: %s %d %d %d %.17g %.17g %.17g %.17g %.17g %.17g %lld\n", polish_name(pr.outcome), pr.steps, pr.factorisations,
         pr.indefinite, pr.F_initial, pr.F_final, pr.grad_initial, pr.grad_final, mr.chi2_initial, mr.chi2_final, mr.near_pi);
  if (pr.outcome != DPGO_POLISH_SKIPPED) r.Xnow.swap(Z);
  return 0;
}

// --ml_gnc tls|gm (likewise; empty: off) --ml_gnc_barc2 V (default: the chi2_dof quantile at 0.999, 16.266 for d = 2 and 22.458
// for d = 3)  behind --ml_polish and ahead of every later step, which then acts on its point: dpgo_group_ml_gnc (graduated
// non-convexity on chi2_e = r_e' Omega_e r_e with the file's information matrices, the inter-node edges as the robust set, pose 0
// the anchor) from the final X, and one more line on stdout, in gnc:'s format with the two near_pi counts behind it
//     ml gnc: <outcome> <levels> <steps> <factorisations> <num_robust> <num_zero> <num_between> <num_outliers>
//             <mu_initial> <mu_final> <F_initial> <F_weighted_final> <F_surrogate_final> <near_pi> <near_pi_all>
// --ml_gnc_report FILE: one header line
//     # ml_gnc <outcome> barc2 <V> edges <m> robust <num_robust> zero <num_zero> outliers <num_outliers>
// then per edge, in the graph's order,   i j in_R w chi2   (17 digits), chi2 at that point.  --ml_covariance and --ml_report
// behind it act on the graph without the edges of weight 0 (dpgo_graph_filter_edges): the covariance of the inlier set.
// (No filtered .g2o is written: the g2o writer does not export Omega.)
static int step_ml_gnc(Run &r) {
  const Args &a = r.a;
  if (a.ml_gnc.empty()) return 0;
  if (a.ml_gnc != "tls" && a.ml_gnc != "gm") {
    fprintf(stderr, "--ml_gnc takes tls or gm.\n");
    return -1;
  }
  if (r.refused("ml gnc")) return 0;
  const int m = r.graph_edges, ld = r.ld;
  std::vector<double> Xc, Z(r.point_size(), 0.0), w(m, 1.0);
  dpgo_gnc_options_t go;
  dpgo_gnc_options_default(&go);
  go.kind = a.ml_gnc == "tls" ? DPGO_GNC_TLS : DPGO_GNC_GM;
  go.barc2 = a.ml_gnc_barc2 > 0 ? a.ml_gnc_barc2 : (r.d == 2 ? 16.266 : 22.458);
  dpgo_ml_gnc_result_t mr;
  dpgo_group_t *grp = ml_group(r);
  if (!grp || r.point(Xc) != 0) return -1;
  if (dpgo_group_ml_gnc(grp, r.g, Xc.data(), ld, &go, nullptr, 0, Z.data(), ld, w.data(), nullptr, 0, &mr) != 0) return -1;
  const dpgo_gnc_result_t &gr = mr.gnc;
  printf("ml gnc: %s %d %d %d %d %d %d %d %.17g %.17g %.17g %.17g %.17g %lld %lld\n", gnc_name(gr.outcome), gr.levels, gr.steps,
         gr.factorisations, gr.num_robust, gr.num_zero, gr.num_between, gr.num_outliers, gr.mu_initial, gr.mu_final, gr.F_initial,
         gr.F_weighted_final, gr.F_surrogate_final, mr.near_pi, mr.near_pi_all);
  if (gr.outcome == DPGO_GNC_SKIPPED) return 0;
  if (!a.ml_gnc_report.empty()) {
    std::vector<double> chi2(m), wb(m), sums(10);
    if (r.load_edges() != 0 ||
        dpgo_group_ml_gnc_eval(grp, r.g, Z.data(), ld, go.kind, gr.mu_final > 0 ? gr.mu_final : 1.0, go.barc2, nullptr, w.data(), 0,
                               chi2.data(), wb.data(), sums.data(), nullptr, nullptr, nullptr, nullptr) != 0)
      return -1;
    FILE *f = open_report(a.ml_gnc_report.c_str());
    if (!f) return -1;
    fprintf(f, "# ml_gnc %s barc2 %.17g edges %d robust %d zero %d outliers %d\n", gnc_name(gr.outcome), go.barc2, m, gr.num_robust,
            gr.num_zero, gr.num_outliers);
    for (int e = 0; e < m; e++) fprintf(f, "%d %d %d %.17g %.17g\n", r.I[e], r.J[e], (int)r.inter[e], w[e], chi2[e]);
    fclose(f);
  }
  std::vector<unsigned char> keep(m);
  if (r.ml_kept) dpgo_graph_free(r.ml_kept);
  r.ml_kept = nullptr;
  r.ml_kept_edges.clear();
  for (int e = 0; e < m; e++) {
    keep[e] = w[e] > 0.0;
    if (keep[e]) r.ml_kept_edges.push_back(e);
  }
  if ((int)r.ml_kept_edges.size() < m && dpgo_graph_filter_edges(r.g, keep.data(), &r.ml_kept) != 0) return -1;
  r.Xnow.swap(Z);
  return 0;
}

// --ml_covariance FILE (likewise; empty: off)  in --covariance's file format and with its line on stdout under the prefix
// "ml covariance:", from dpgo_group_ml_covariance at the final X: the marginals of the Fisher information sum J' Omega J (behind
// --ml_gnc: over the edges of positive weight)
static int step_ml_covariance(Run &r) {
  if (r.a.ml_covariance.empty() || r.refused("ml covariance")) return 0;
  const int dof = r.dof;
  std::vector<double> Xc, marg((size_t)r.N * dof * dof, 0.0);
  dpgo_cov_result_t cv;
  dpgo_group_t *grp = ml_group(r);
  if (!grp || r.point(Xc) != 0) return -1;
  if (dpgo_group_ml_covariance(grp, r.ml_graph(), Xc.data(), r.ld, 0, 0, nullptr, 0, marg.data(), nullptr, &cv) != 0) return -1;
  printf("ml covariance: %s %d %d %d %d %lld %.16g %.16g\n", cov_name(cv.outcome), cv.unknowns, cv.fronts, cv.levels, cv.max_front,
         cv.device_bytes, cv.pivot_min, cv.stationarity);
  if (cv.outcome != DPGO_COV_OK) return 0;
  FILE *f = open_report(r.a.ml_covariance.c_str());
  if (!f) return -1;
  for (int p = 0; p < r.N; p++) {
    fprintf(f, "%d", p);
    write_upper(f, &marg[(size_t)p * dof * dof], dof);
    fprintf(f, "\n");
  }
  fclose(f);
  return 0;
}

// --ml_report FILE (likewise; empty: off)  from dpgo_group_ml_eval at the final X: one header line
//     # F_ml <F_ml> chi2_total <2 F_ml> edges <m> near_pi <count>
// then per edge of the graph, in its order,   i j chi2     (17 digits); behind --ml_gnc: of the graph without the edges of weight 0
static int step_ml_report(Run &r) {
  if (r.a.ml_report.empty() || r.refused("ml report")) return 0;
  const int m = r.ml_edges();
  std::vector<double> Xc, chi2(m, 0.0);
  double F = 0;
  long long near = 0;
  dpgo_group_t *grp = ml_group(r);
  if (!grp || r.point(Xc) != 0 || r.load_edges() != 0) return -1;
  if (dpgo_group_ml_eval(grp, r.ml_graph(), Xc.data(), r.ld, &F, &near, nullptr, chi2.data(), nullptr, nullptr, nullptr) != 0) return -1;
  FILE *f = open_report(r.a.ml_report.c_str());
  if (!f) return -1;
  fprintf(f, "# F_ml %.17g chi2_total %.17g edges %d near_pi %lld\n", F, 2 * F, m, near);
  for (int e = 0; e < m; e++) fprintf(f, "%d %d %.17g\n", r.I[r.ml_edge(e)], r.J[r.ml_edge(e)], chi2[e]);
  fclose(f);
  return 0;
}

// A .g2o of candidate edges p -> q, read by the loader's edge parser, as dpgo_group_pair_covariance and
// dpgo_group_candidate_set take it: pairs (p, q) and per candidate R, t, kappa, tau.
struct Candidates {
  int m = 0;
  std::vector<int> pairs;       // p, q of candidate k at 2 k, 2 k + 1
  std::vector<double> cand;
};

// `reasons` is the caller's list of what makes the file unusable, for its error; at least min_count candidates.  info
// (optional): the candidates' information matrices as the file has them (dof^2 each; Omega_iso for a file without).
static int load_candidates(const Run &r, const std::string &file, int min_count, const char *reasons, Candidates &c,
                           std::vector<double> *info = nullptr) {
  const int d = r.d, nc = d * d + d + 2;
  dpgo_graph_t *cg = nullptr;
  int cd = 0, cN = 0, cn = 0, m = 0;
  if (dpgo_read_g2o(file.c_str(), 1, &cg) != 0 || dpgo_graph_info(cg, &cd, &cN, &cn, &m) != 0 || cd != d || cN > r.N || m < min_count) {
    fprintf(stderr, "Cannot use the candidates in %s (%s).\n", file.c_str(), reasons);
    dpgo_graph_free(cg);
    return -1;
  }
  c.m = m;
  c.pairs.resize((size_t)2 * m);
  c.cand.resize((size_t)m * nc);
  std::vector<int> I(m), J(m);
  std::vector<double> R((size_t)m * d * d), t((size_t)m * d), kappa(m), tau(m);
  int got = dpgo_graph_edges(cg, I.data(), J.data(), R.data(), t.data(), kappa.data(), tau.data());
  if (got == 0 && info) {
    info->assign((size_t)m * r.dof * r.dof, 0.0);
    got = dpgo_graph_edge_information(cg, info->data(), nullptr);
  }
  dpgo_graph_free(cg);
  if (got != 0) {
    fprintf(stderr, "Cannot read the edges of %s.\n", file.c_str());
    return -1;
  }
  for (int k = 0; k < m; k++) {
    c.pairs[2 * k] = I[k]; c.pairs[2 * k + 1] = J[k];
    double *row = &c.cand[(size_t)k * nc];
    std::copy_n(&R[(size_t)k * d * d], d * d, row);
    std::copy_n(&t[(size_t)k * d], d, row + d * d);
    row[d * d + d] = kappa[k];
    row[d * d + d + 1] = tau[k];
  }
  return 0;
}

// --gate_candidates FILE --gate_report FILE (likewise; both or neither)  beside --covariance, for the trivial loss
// and a world of one rank: FILE is a .g2o of candidate edges p -> q, read by the loader's edge parser; every
// candidate is tested against the final X with dpgo_group_pair_covariance (pose 0 the anchor), one line per
// candidate in the report,
//     p q d2 dof not_pd  S[0][0] S[0][1] ... S[dof-1][dof-1]   (the upper triangle of Sigma_rel, 17 digits)
// and one more line on stdout
//     gate: <outcome> <candidates> <columns> <batches> <device_bytes> <pivot_min> <stationarity>
// (NOT_PD or SKIPPED: the report is not written); the same reasons as --covariance when it is not computed
static int step_gate(Run &r) {
  const Args &a = r.a;
  if (a.gate_candidates.empty() && a.gate_report.empty()) return 0;
  if (a.gate_candidates.empty() || a.gate_report.empty()) {
    fprintf(stderr, "--gate_candidates and --gate_report go together.\n");
    return -1;
  }
  if (r.refused("gate", TRIVIAL_LOSS, "Hessian")) return 0;
  Candidates c;
  if (load_candidates(r, a.gate_candidates, 0, "unreadable, another dimension, or a pose that is not in the graph", c) != 0) return -1;
  const int dof = r.dof, m = c.m;
  std::vector<double> Xc, joint((size_t)m * 3 * dof * dof), rel((size_t)m * dof * dof), gate((size_t)m * (2 + dof));
  dpgo_pairs_result_t pr;
  if (r.point(Xc) != 0 ||
      dpgo_group_pair_covariance(r.grp, Xc.data(), r.ld, 0, 0, c.pairs.data(), m, c.cand.data(), joint.data(), rel.data(), gate.data(), &pr) != 0)
    return -1;
  printf("gate: %s %d %d %d %lld %.16g %.16g\n", pairs_name(pr.outcome), m, pr.columns, pr.batches, pr.device_bytes, pr.pivot_min,
         pr.stationarity);
  if (pr.outcome != DPGO_PAIRS_OK) return 0;
  FILE *f = open_report(a.gate_report.c_str());
  if (!f) return -1;
  for (int k = 0; k < m; k++) {
    const double *gk = &gate[(size_t)k * (2 + dof)];
    fprintf(f, "%d %d %.17g %d %d", c.pairs[2 * k], c.pairs[2 * k + 1], gk[0], dof, gk[1] != 0.0 ? 1 : 0);
    write_upper(f, &rel[(size_t)k * dof * dof], dof);
    fprintf(f, "\n");
  }
  fclose(f);
  return 0;
}

// --ml_edge_reliability FILE (for any --loss and a world of one rank; empty: off)  at the final X -- behind --ml_polish its
// point: dpgo_group_ml_edge_reliability of every edge (pose 0 the anchor, DPGO_RELY_AUTO) on the file's information matrices;
// behind --ml_gnc of the graph without the edges of weight 0, as --ml_covariance.  One more line on stdout
//     ml reliability: <outcome> <method> <edges> <flagged> <redundancy_sum> <device_bytes> <pivot_min> <stationarity>
// and, for OK, one line per edge in FILE, in --edge_reliability's format (17 digits; e: the edge's index in the whole graph):
//     e p q redundancy redundancy_trans d2_own d2_loo flag influence
static int step_ml_reliability(Run &r) {
  const Args &a = r.a;
  if (a.ml_edge_reliability.empty() || r.refused("ml reliability")) return 0;
  const int m = r.ml_edges(), w = 6 + 2 * r.dof;
  std::vector<double> Xc, rec((size_t)std::max(m, 1) * w, 0.0);
  dpgo_rely_result_t rr;
  dpgo_group_t *grp = ml_group(r);
  if (!grp || r.point(Xc) != 0 || r.load_edges() != 0) return -1;
  if (dpgo_group_ml_edge_reliability(grp, r.ml_graph(), Xc.data(), r.ld, 0, 0, DPGO_RELY_AUTO, nullptr, 0, rec.data(), nullptr, nullptr,
                                     &rr) != 0)
    return -1;
  printf("ml reliability: %s %s %d %d %.17g %lld %.16g %.16g\n", rely_name(rr.outcome), rely_method_name(rr.method_used), rr.edges,
         rr.flagged, rr.redundancy_sum, rr.device_bytes, rr.pivot_min, rr.stationarity);
  if (rr.outcome != DPGO_RELY_OK) return 0;
  FILE *f = open_report(a.ml_edge_reliability.c_str());
  if (!f) return -1;
  for (int e = 0; e < m; e++) {
    const double *q = &rec[(size_t)e * w];
    fprintf(f, "%d %d %d %.17g %.17g %.17g %.17g %d %.17g\n", r.ml_edge(e), r.I[r.ml_edge(e)], r.J[r.ml_edge(e)], q[2], q[3], q[4], q[0],
            (int)q[1], q[5]);
  }
  fclose(f);
  return 0;
}

// --ml_gate_candidates FILE --ml_gate_report FILE (likewise; both or neither)  FILE is a .g2o of candidate edges p -> q, read as
// --gate_candidates reads it, with its information matrices kept; every candidate is tested against the final X with
// dpgo_group_ml_pair_gate (pose 0 the anchor; behind --ml_gnc against the graph without the edges of weight 0), one line per
// candidate in the report, in --gate_report's format,
//     p q d2 dof not_pd  S[0][0] S[0][1] ... S[dof-1][dof-1]   (the upper triangle of rel, 17 digits)
// and one more line on stdout
//     ml gate: <outcome> <candidates> <columns> <batches> <device_bytes> <pivot_min> <stationarity>
// (NOT_PD or SKIPPED: the report is not written)
static int step_ml_gate(Run &r) {
  const Args &a = r.a;
  if (a.ml_gate_candidates.empty() && a.ml_gate_report.empty()) return 0;
  if (a.ml_gate_candidates.empty() || a.ml_gate_report.empty()) {
    fprintf(stderr, "--ml_gate_candidates and --ml_gate_report go together.\n");
    return -1;
  }
  if (r.refused("ml gate")) return 0;
  Candidates c;
  std::vector<double> info;
  if (load_candidates(r, a.ml_gate_candidates, 0, "unreadable, another dimension, or a pose that is not in the graph", c, &info) != 0)
    return -1;
  const int d = r.d, dof = r.dof, m = c.m, nc = d * d + d + 2;
  std::vector<double> Xc, cR((size_t)m * d * d), ct((size_t)m * d), joint((size_t)m * 3 * dof * dof), rel((size_t)m * dof * dof),
      gate((size_t)m * (2 + dof));
  for (int k = 0; k < m; k++) {
    std::copy_n(&c.cand[(size_t)k * nc], d * d, &cR[(size_t)k * d * d]);
    std::copy_n(&c.cand[(size_t)k * nc + d * d], d, &ct[(size_t)k * d]);
  }
  dpgo_pairs_result_t pr;
  dpgo_group_t *grp = ml_group(r);
  if (!grp || r.point(Xc) != 0) return -1;
  if (dpgo_group_ml_pair_gate(grp, r.ml_graph(), Xc.data(), r.ld, 0, 0, c.pairs.data(), m, cR.data(), ct.data(), info.data(), joint.data(),
                              rel.data(), gate.data(), &pr) != 0)
    return -1;
  printf("ml gate: %s %d %d %d %lld %.16g %.16g\n", pairs_name(pr.outcome), m, pr.columns, pr.batches, pr.device_bytes, pr.pivot_min,
         pr.stationarity);
  if (pr.outcome != DPGO_PAIRS_OK) return 0;
  FILE *f = open_report(a.ml_gate_report.c_str());
  if (!f) return -1;
  for (int k = 0; k < m; k++) {
    const double *gk = &gate[(size_t)k * (2 + dof)];
    fprintf(f, "%d %d %.17g %d %d", c.pairs[2 * k], c.pairs[2 * k + 1], gk[0], dof, gk[1] != 0.0 ? 1 : 0);
    write_upper(f, &rel[(size_t)k * dof * dof], dof);
    fprintf(f, "\n");
  }
  fclose(f);
  return 0;
}

// --sensitivity_pose P --sensitivity_report FILE (likewise; both or neither)  behind --polish, on the polished
// point, for the trivial loss and a world of one rank: dpgo_group_sensitivity with the dof unit columns of pose P
// (pose 0 the anchor) -- how every measurement moves that pose -- one more line on stdout
//     sensitivity: <outcome> <P> <edges> <columns> <batches> <device_bytes> <pivot_min> <stationarity>
// and, for OK, one line per edge in FILE: e i j inter, then dof x (2 + dof) values, row a the derivatives of
// coordinate a of the pose in (kappa, tau, t~, eta); "sensitivity: not computed (...)" says why not
// With a robust --loss behind --robust_polish (one rank): dpgo_group_robust_sensitivity with the run's loss and
// loss_reg on the robust polish's point and group; the line's prefix is "robust sensitivity:", every row of FILE
// has dof x (3 + dof) values -- one more per row, the edge's term of the derivative in the loss threshold -- and
// a last line "delta" with the dof values of d x_pose / d delta
static int step_sensitivity(Run &r) {
  const Args &a = r.a;
  const int pose = a.sensitivity_pose;
  if (pose < 0 && a.sensitivity_report.empty()) return 0;
  if (pose < 0 || pose >= r.N || a.sensitivity_report.empty()) {
    fprintf(stderr, "--sensitivity_pose (a pose of the graph) and --sensitivity_report go together.\n");
    return -1;
  }
  const bool robust = a.loss != 0 && a.robust_polish && a.world == 1;
  if (!robust && r.refused("sensitivity", TRIVIAL_LOSS, "Hessian", BEHIND_POLISH)) return 0;
  const int dof = r.dof, m = r.graph_edges, no = (robust ? 3 : 2) + dof;
  const size_t n = (size_t)dof * r.N;
  if (r.load_edges() != 0) return -1;
  // the dof unit columns of the pose: row a of the report's block of an edge is d x_pose[a] / d (kappa, tau, t~, eta)
  std::vector<double> Xc, up(n * dof, 0.0), sens((size_t)dof * m * no, 0.0), dreg(dof, 0.0);
  for (int c = 0; c < dof; c++) up[(size_t)c * n + (size_t)dof * pose + c] = 1.0;
  dpgo_sens_result_t sr;
  if (r.point(Xc) != 0) return -1;
  if (robust ? r.post_group() != 0 || dpgo_group_robust_sensitivity(r.post, r.g, Xc.data(), r.ld, a.loss, r.opt.loss_reg, 0, 0, up.data(), (int)n,
                                                                    dof, nullptr, sens.data(), dreg.data(), &sr) != 0
             : dpgo_group_sensitivity(r.grp, r.g, Xc.data(), r.ld, 0, 0, up.data(), (int)n, dof, nullptr, sens.data(), &sr) != 0)
    return -1;
  printf("%ssensitivity: %s %d %d %d %d %lld %.16g %.16g\n", robust ? "robust " : "", sens_name(sr.outcome), pose, sr.edges, sr.columns,
         sr.batches, sr.device_bytes, sr.pivot_min, sr.stationarity);
  if (sr.outcome != DPGO_SENS_OK) return 0;
  FILE *f = open_report(a.sensitivity_report.c_str());
  if (!f) return -1;
  write_sensitivity_rows(f, m, r.I.data(), r.J.data(), r.inter.data(), sens.data(), dof, no);
  if (robust) {
    fprintf(f, "delta");
    for (int c = 0; c < dof; c++) fprintf(f, " %.17g", dreg[c]);
    fprintf(f, "\n");
  }
  fclose(f);
  return 0;
}

// --edge_reliability FILE (likewise; empty: off)  behind --polish, on the polished point, for the trivial loss and a
// world of one rank: dpgo_group_edge_reliability of every edge (pose 0 the anchor, DPGO_RELY_AUTO) -- how well each
// measurement is checked by the others and whether it agrees with them -- one more line on stdout
//     reliability: <outcome> <method> <edges> <flagged> <unweighted> <redundancy_sum> <device_bytes> <pivot_min> <stationarity>
// and, for OK, one line per edge in FILE (17 digits):
//     e p q redundancy redundancy_trans d2_own d2_loo flag influence
// "reliability: not computed (...)" says why not
static int step_reliability(Run &r) {
  const Args &a = r.a;
  if (a.edge_reliability.empty() || r.refused("reliability", TRIVIAL_LOSS, "Hessian", BEHIND_POLISH)) return 0;
  const int m = r.graph_edges, w = 6 + 2 * r.dof;
  if (r.load_edges() != 0) return -1;
  std::vector<double> Xc, rec((size_t)m * w, 0.0);
  dpgo_rely_result_t rr;
  if (r.point(Xc) != 0 ||
      dpgo_group_edge_reliability(r.grp, r.g, Xc.data(), r.ld, 0, 0, DPGO_RELY_AUTO, nullptr, 0, rec.data(), nullptr, nullptr, &rr) != 0)
    return -1;
  printf("reliability: %s %s %d %d %d %.17g %lld %.16g %.16g\n", rely_name(rr.outcome), rely_method_name(rr.method_used), rr.edges,
         rr.flagged, rr.unweighted, rr.redundancy_sum, rr.device_bytes, rr.pivot_min, rr.stationarity);
  if (rr.outcome != DPGO_RELY_OK) return 0;
  FILE *f = open_report(a.edge_reliability.c_str());
  if (!f) return -1;
  for (int e = 0; e < m; e++) {
    const double *q = &rec[(size_t)e * w];
    fprintf(f, "%d %d %d %.17g %.17g %.17g %.17g %d %.17g\n", e, r.I[e], r.J[e], q[2], q[3], q[4], q[0], (int)q[1], q[5]);
  }
  fclose(f);
  return 0;
}

// --marginal_set FILE --marginal_report FILE [--marginal_base P] (likewise; the two files both or neither)  for the
// trivial loss and a world of one rank, on the final point -- the polished one behind --polish, where it belongs:
// FILE lists one pose id per line, the kept set in that order; dpgo_group_joint_marginal (pose 0 the anchor)
// gives the set's joint covariance, its inverse and log-determinant -- with --marginal_base P, a member of the
// set, those of the relative poses T_P^-1 T_k.  The report (17 digits): a line "n <n> logdet <logdet>", a line
// with the poses of the dof-blocks in order, n rows of cov, n rows of info; and one more line on stdout
//     marginal: <outcome> <poses> <n> <columns> <batches> <device_bytes> <info_not_pd> <logdet> <stationarity>
// (NOT_PD or SKIPPED: the report is not written); "marginal: not computed (...)" says why not
static int step_marginal(Run &r) {
  const Args &a = r.a;
  if (a.marginal_set.empty() && a.marginal_report.empty()) return 0;
  if (a.marginal_set.empty() || a.marginal_report.empty()) {
    fprintf(stderr, "--marginal_set and --marginal_report go together.\n");
    return -1;
  }
  if (r.refused("marginal", TRIVIAL_LOSS, "Hessian")) return 0;
  std::vector<int> keep;
  FILE *in = fopen(a.marginal_set.c_str(), "r");
  if (!in) { fprintf(stderr, "Cannot read %s.\n", a.marginal_set.c_str()); return -1; }
  for (int p; fscanf(in, "%d", &p) == 1;) keep.push_back(p);
  fclose(in);
  const int K = (int)keep.size(), n = r.dof * (K - (a.marginal_base >= 0 ? 1 : 0));
  if (K < 1 || n < 1) { fprintf(stderr, "%s holds no kept set.\n", a.marginal_set.c_str()); return -1; }
  std::vector<double> Xc, cov((size_t)n * n, 0.0), info((size_t)n * n, 0.0);
  double logdet = 0.0;
  dpgo_marg_result_t mr;
  if (r.point(Xc) != 0 ||
      dpgo_group_joint_marginal(r.grp, Xc.data(), r.ld, keep.data(), K, 0, a.marginal_base, 1, 0, cov.data(), info.data(), &logdet, &mr) != 0)
    return -1;
  printf("marginal: %s %d %d %d %d %lld %d %.17g %.16g\n", marg_name(mr.outcome), K, mr.n, mr.columns, mr.batches, mr.device_bytes,
         mr.info_not_pd, logdet, mr.stationarity);
  if (mr.outcome != DPGO_MARG_OK) return 0;
  FILE *f = open_report(a.marginal_report.c_str());
  if (!f) return -1;
  fprintf(f, "n %d logdet %.17g\n", n, logdet);
  bool first = true;
  for (int p : keep)
    if (p != a.marginal_base) { fprintf(f, "%s%d", first ? "" : " ", p); first = false; }
  fprintf(f, "\n");
  write_matrix(f, cov.data(), n);
  write_matrix(f, info.data(), n);
  fclose(f);
  return 0;
}

// --select_candidates FILE --select_report FILE [--select_budget K] [--select_d2_max V] (likewise; the two files both
// or neither)  for the trivial loss and a world of one rank, on the final point -- the polished one behind --polish:
// FILE is a .g2o of candidate edges, read as --gate_candidates reads it; dpgo_group_candidate_set (pose 0 the
// anchor) judges them TOGETHER -- d2_joint = r^T S^-1 r, gain_all -- and chooses at most K (default: all) by
// conditional information gain, a candidate being eligible while its conditional d2 <= V (default 0: no gate).
// The report (17 digits): a line "n <n> logdet <logdet> d2_joint <d2> gain_all <gain>", a line "selected <k>
// gain <gain_selected> d2 <d2_selected>", k lines "<candidate> <p> <q> <gain> <d2> <eligible>", n rows of S, n rows
// of S^-1; and one more line on stdout
//     candidates: <outcome> <candidates> <n> <poses> <columns> <batches> <device_bytes> <joint_not_pd> <selected> <d2_joint> <gain_all> <stationarity>
// (NOT_PD or SKIPPED: the report is not written); "candidates: not computed (...)" says why not
static int step_candidates(Run &r) {
  const Args &a = r.a;
  if (a.select_candidates.empty() && a.select_report.empty()) return 0;
  if (a.select_candidates.empty() || a.select_report.empty()) {
    fprintf(stderr, "--select_candidates and --select_report go together.\n");
    return -1;
  }
  if (r.refused("candidates", TRIVIAL_LOSS, "Hessian")) return 0;
  Candidates c;
  if (load_candidates(r, a.select_candidates, 1, "unreadable, empty, another dimension, or a pose that is not in the graph", c) != 0) return -1;
  const int m = c.m, n = r.dof * m, budget = a.select_budget < 0 ? m : a.select_budget;
  std::vector<double> Xc, S((size_t)n * n), res((size_t)n), info((size_t)n * n), steps((size_t)4 * std::max(budget, 1));
  std::vector<int> selected((size_t)std::max(budget, 1), -1), poses((size_t)2 * m);
  double sc[5] = {0, 0, 0, 0, 0};
  dpgo_cand_result_t cr;
  if (r.point(Xc) != 0 ||
      dpgo_group_candidate_set(r.grp, Xc.data(), r.ld, c.pairs.data(), m, c.cand.data(), 0, budget, a.select_d2_max, 1, 0, nullptr, S.data(),
                               res.data(), info.data(), sc, selected.data(), steps.data(), poses.data(), &cr) != 0)
    return -1;
  printf("candidates: %s %d %d %d %d %d %lld %d %d %.17g %.17g %.16g\n", cand_name(cr.outcome), m, cr.n, cr.poses, cr.columns, cr.batches,
         cr.device_bytes, cr.joint_not_pd, cr.n_selected, sc[1], sc[2], cr.stationarity);
  if (cr.outcome != DPGO_CAND_OK) return 0;
  FILE *f = open_report(a.select_report.c_str());
  if (!f) return -1;
  fprintf(f, "n %d logdet %.17g d2_joint %.17g gain_all %.17g\n", n, sc[0], sc[1], sc[2]);
  fprintf(f, "selected %d gain %.17g d2 %.17g\n", cr.n_selected, sc[3], sc[4]);
  for (int k = 0; k < cr.n_selected; k++) {
    const double *s = &steps[4 * (size_t)k];
    fprintf(f, "%d %d %d %.17g %.17g %d\n", selected[k], c.pairs[2 * selected[k]], c.pairs[2 * selected[k] + 1], s[1], s[2], (int)s[3]);
  }
  write_matrix(f, S.data(), n);
  write_matrix(f, info.data(), n);
  fclose(f);
  return 0;
}

int main(int argc, char **argv) {
  Args a;
  if (const int rc = parse_args(argc, argv, a)) return rc > 0 ? 0 : -1;
  Run r(a);
  std::vector<double> X;
  std::vector<std::vector<double>> results;
  if (setup(r) != 0 || initialise(r, X) != 0 || solve(r, results) != 0) return -1;
  for (int (*step)(Run &) : {step_gnc, step_polish, step_modes, step_staircase, step_robust_polish, step_ml_polish, step_ml_gnc,
                             step_certify, step_verify, step_edges, step_covariance, step_robust_covariance, step_ml_covariance,
                             step_ml_report, step_ml_reliability, step_ml_gate, step_gate, step_sensitivity, step_reliability, step_marginal, step_candidates})
    if (step(r) != 0) return -1;
  if (r.ml_kept) dpgo_graph_free(r.ml_kept);
  if (r.post) dpgo_group_free(r.post);
  if (a.save && save(r, X, results) != 0) return -1;
  if (r.comm) dpgo_comm_free(r.comm);
  dpgo_group_free(r.grp);
  dpgo_graph_free(r.g);
  return 0;
}
