// dist_pgo -- command-line driver with the reference's flags and outputs, on top of the C ABI.
//
// Mirrors C++/examples/dist_pgo.cpp:
//   flags      --dataset --num_nodes --iters[1000] --dist_init[true] --loss[trivial|huber|welsch]
//              --accelerated[true] --save[true]                                     (:23-47)
//              --certify (not in the reference's driver; off: every output is as without it)  after the loop, for the trivial
//              loss and a world of one rank, one more line on stdout
//                  certificate: <status> <theta> <residual> <iterations> <stationarity>
//              from dpgo_group_certify (SESyncProblem::verify_solution, C++/SESync/src/SESyncProblem.cpp:397-468); with a
//              robust loss or several ranks a line that says why not
//              --verify (likewise)  after the summary (and after --certify's line), one more line on stdout
//                  verification: <status> <outcome> <pivot_min> <theta> <residual> <iterations> <stationarity>
//              from dpgo_group_verify (fast_verification, C++/SESync/src/SESync_utils.cpp:721-830: the Cholesky factorisation
//              of S + eta I first, the search only when it does not succeed); the same reasons when it is not computed
//              --edge_report FILE (likewise; empty: off)  after the loop, one row per edge of the graph in file order,
//                  edge i j inter s_rot s_trans rho weight        (16 digits)
//              from dpgo_edge_eval_run at the final X with the run's loss: what the robust loss did to every measurement
//              --verify_reweighted (likewise)  after the summary (and the lines above), one more line on stdout
//                  reweighted verification: <status> <outcome> <pivot_min> <theta> <residual> <iterations> <stationarity>
//                                           <num_downweighted>/<num_inter> <weight_min>
//              from dpgo_graph_verify_reweighted: the certificate of the problem re-weighted by the loss weights at the
//              final X (any loss); with several ranks a line that says why not
//              --covariance FILE (likewise; empty: off)  after the summary (and the lines above), for the trivial loss and a
//              world of one rank, one line per pose in FILE,
//                  p  S[0][0] S[0][1] ... S[dof-1][dof-1]       (the upper triangle of Sigma_pp row by row, 17 digits)
//              -- the marginal covariance of pose p relative to pose 0 from dpgo_group_covariance at the final X, tangent
//              coordinates (translation in the world frame, rotation in the body frame) -- and one more line on stdout
//                  covariance: <outcome> <unknowns> <fronts> <levels> <max_front> <device_bytes> <pivot_min> <stationarity>
//              (NOT_PD or SKIPPED: FILE is not written); the same reasons as --certify when it is not computed
//              --polish (likewise)  after the loop and ahead of --certify / --verify / --covariance, which then act on the polished
//              point, for the trivial loss and a world of one rank: dpgo_group_polish (damped Riemannian Newton steps, pose 0
//              the anchor) from the final X, and one more line on stdout
//                  polish: <outcome> <steps> <factorisations> <indefinite> <F_initial> <F_final> <grad_initial> <grad_final>
//              the result files then hold the polished X; the same reasons as --covariance when it is not computed
//              --robust_polish (likewise)  after the loop and ahead of --edge_report / --verify_reweighted / --robust_covariance, which
//              then act on its point, for a robust --loss and a world of one rank: dpgo_group_robust_polish (the Newton polish of
//              the robust objective on its true Hessian, pose 0 the anchor) on a second, trivial-loss group of the same graph
//              built for it (max_iterations = 0; seconds of set-up at 100 000 poses), one more line on stdout
//                  robust polish: <the fields of polish:>
//              with the F fields those of the robust objective; the result files then hold the polished X; with the trivial loss
//              (--polish is the call then) or several ranks a line "robust polish: not computed (...)" that says why not
//              --robust_covariance FILE (likewise; empty: off)  in --covariance's file format and with its line on stdout under
//              the prefix "robust covariance:", from dpgo_group_robust_covariance at the final X
//              --gnc tls|gm (likewise; empty: off) --gnc_barc2 V (default 4)  after the loop and ahead of --polish / --staircase /
//              --certify / --verify / --covariance and the robust flags, which then act on its point, for a world of one rank and any
//              --loss: dpgo_group_gnc (graduated non-convexity, the inter-node edges as the robust set, pose 0 the anchor) on the
//              second, trivial-loss group of --robust_polish, from the final X, and one more line on stdout
//                  gnc: <outcome> <levels> <steps> <factorisations> <num_robust> <num_zero> <num_between> <num_outliers>
//                       <mu_initial> <mu_final> <F_initial> <F_weighted_final> <F_surrogate_final>
//              the result files then hold its point.  --gnc_report FILE: one line per edge, "i j in_R w s" (17 digits), s at that
//              point; --gnc_filtered FILE: the graph without the edges of weight 0 (dpgo_graph_filter_edges) with that point, as a
//              .g2o (dpgo_write_g2o).  With several ranks a line that says why not
//              --staircase (likewise)  after --polish and ahead of --certify / --verify / --covariance, which then act on its
//              result, for the trivial loss and a world of one rank: dpgo_group_staircase (the Riemannian staircase: TNT at rank
//              r, verify, an escape along the certificate's direction, the rounding and a polish) from the point so far, and
//              one more line on stdout
//                  staircase: <outcome> <final_rank> <F_initial> <F_sdp> <F_final> <gap>
//              the result files then hold its Xhat; the same reasons as --polish when it is not computed
//              --sensitivity_pose P --sensitivity_report FILE (likewise; both or neither)  behind --polish, on the polished
//              point, for the trivial loss and a world of one rank: dpgo_group_sensitivity with the dof unit columns of pose P
//              (pose 0 the anchor) -- how every measurement moves that pose -- one more line on stdout
//                  sensitivity: <outcome> <P> <edges> <columns> <batches> <device_bytes> <pivot_min> <stationarity>
//              and, for OK, one line per edge in FILE: e i j inter, then dof x (2 + dof) values, row a the derivatives of
//              coordinate a of the pose in (kappa, tau, t~, eta); "sensitivity: not computed (...)" says why not
//              With a robust --loss behind --robust_polish (one rank): dpgo_group_robust_sensitivity with the run's loss and
//              loss_reg on the robust polish's point and group; the line's prefix is "robust sensitivity:", every row of FILE
//              has dof x (3 + dof) values -- one more per row, the edge's term of the derivative in the loss threshold -- and
//              a last line "delta" with the dof values of d x_pose / d delta
//              --edge_reliability FILE (likewise; empty: off)  behind --polish, on the polished point, for the trivial loss and a
//              world of one rank: dpgo_group_edge_reliability of every edge (pose 0 the anchor, DPGO_RELY_AUTO) -- how well each
//              measurement is checked by the others and whether it agrees with them -- one more line on stdout
//                  reliability: <outcome> <method> <edges> <flagged> <unweighted> <redundancy_sum> <device_bytes> <pivot_min> <stationarity>
//              and, for OK, one line per edge in FILE (17 digits):
//                  e p q redundancy redundancy_trans d2_own d2_loo flag influence
//              "reliability: not computed (...)" says why not
//              --gate_candidates FILE --gate_report FILE (likewise; both or neither)  beside --covariance, for the trivial loss
//              and a world of one rank: FILE is a .g2o of candidate edges p -> q, read by the loader's edge parser; every
//              candidate is tested against the final X with dpgo_group_pair_covariance (pose 0 the anchor), one line per
//              candidate in the report,
//                  p q d2 dof not_pd  S[0][0] S[0][1] ... S[dof-1][dof-1]   (the upper triangle of Sigma_rel, 17 digits)
//              and one more line on stdout
//                  gate: <outcome> <candidates> <columns> <batches> <device_bytes> <pivot_min> <stationarity>
//              (NOT_PD or SKIPPED: the report is not written); the same reasons as --covariance when it is not computed
//              --marginal_set FILE --marginal_report FILE [--marginal_base P] (likewise; the two files both or neither)  for the
//              trivial loss and a world of one rank, on the final point -- the polished one behind --polish, where it belongs:
//              FILE lists one pose id per line, the kept set in that order; dpgo_group_joint_marginal (pose 0 the anchor)
//              gives the set's joint covariance, its inverse and log-determinant -- with --marginal_base P, a member of the
//              set, those of the relative poses T_P^-1 T_k.  The report (17 digits): a line "n <n> logdet <logdet>", a line
//              with the poses of the dof-blocks in order, n rows of cov, n rows of info; and one more line on stdout
//                  marginal: <outcome> <poses> <n> <columns> <batches> <device_bytes> <info_not_pd> <logdet> <stationarity>
//              (NOT_PD or SKIPPED: the report is not written); "marginal: not computed (...)" says why not
//              --select_candidates FILE --select_report FILE [--select_budget K] [--select_d2_max V] (likewise; the two files both
//              or neither)  for the trivial loss and a world of one rank, on the final point -- the polished one behind --polish:
//              FILE is a .g2o of candidate edges, read as --gate_candidates reads it; dpgo_group_candidate_set (pose 0 the
//              anchor) judges them TOGETHER -- d2_joint = r^T S^-1 r, gain_all -- and chooses at most K (default: all) by
//              conditional information gain, a candidate being eligible while its conditional d2 <= V (default 0: no gate).
//              The report (17 digits): a line "n <n> logdet <logdet> d2_joint <d2> gain_all <gain>", a line "selected <k>
//              gain <gain_selected> d2 <d2_selected>", k lines "<candidate> <p> <q> <gain> <d2> <eligible>", n rows of S, n rows
//              of S^-1; and one more line on stdout
//                  candidates: <outcome> <candidates> <n> <poses> <columns> <batches> <device_bytes> <joint_not_pd> <selected> <d2_joint> <gain_all> <stationarity>
//              (NOT_PD or SKIPPED: the report is not written); "candidates: not computed (...)" says why not
//              --hessian_modes K --modes_report FILE [--modes_escape] (likewise; K and FILE both or neither)  behind --polish and
//              ahead of --staircase / --certify / --verify / --covariance, for the trivial loss and a world of one rank:
//              dpgo_group_hessian_modes (pose 0 the anchor) gives the K smallest eigenpairs of the anchored Hessian at the
//              point so far -- at a saddle how negative the curvature is and along which poses, at a minimum 1 / lambda_0, the
//              largest eigenvalue of the covariance.  The report (17 digits): a line "k <K> n <n> mu <mu> hmax <hmax>", then per
//              pair a line "<j> <lambda_j> <residual_j> <the pose with the largest share of |v_j|^2> <that share>" and a line
//              with the n entries of v_j; and one more line on stdout
//                  modes: <outcome> <iterations> <factorisations> <shift_tries> <block> <negative> <lambda_0> <mu> <device_bytes> <escaped> <F> <F_escape>
//              (STALLED or SKIPPED: the report is not written).  With --modes_escape and lambda_0 < 0 the lower point along
//              v_0 becomes the point every later step acts on and the result files hold; "modes: not computed (...)" says why not
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
#include "rdv.h"


static bool parse_bool(const char *s) { return !(strcmp(s, "false") == 0 || strcmp(s, "0") == 0); }

int main(int argc, char **argv) {
  std::string dataset, loss_type = "trivial";
  int num_nodes = -1, iters = 1000, gpu = -1;
  bool dist_init = true, accelerated = true, save = true, certify = false, verify = false, verify_reweighted = false, polish = false, staircase = false, robust_polish = false;
  std::string edge_report, covariance, edge_reliability, gate_candidates, gate_report, robust_covariance, gnc, gnc_report, gnc_filtered;
  std::string sensitivity_report, marginal_set, marginal_report, select_candidates, select_report;
  std::string modes_report;
  int sensitivity_pose = -1, marginal_base = -1, select_budget = -1, hessian_modes = 0;
  bool modes_escape = false;
  double gnc_barc2 = 4.0, select_d2_max = 0.0;
  int rank = getenv("RANK") ? atoi(getenv("RANK")) : 0, world = getenv("WORLD_SIZE") ? atoi(getenv("WORLD_SIZE")) : 1;
  std::string rdv;
  for (int i = 1; i < argc; i++) {
    std::string a = argv[i];
    auto val = [&](const char *name) -> const char * {
      const size_t n = strlen(name);
      if (a.compare(0, n, name) == 0 && a.size() > n && a[n] == '=') return argv[i] + n + 1;
      if (a == name && i + 1 < argc) return argv[++i];
      return nullptr;
    };
    if (a == "--help") {
      printf("Program options:\n  --dataset arg\n  --num_nodes arg\n  --iters arg (=1000)\n  --dist_init arg (=true)\n"
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
             "                          --modes_escape a lower point along the most negative mode replaces the point\n");
      return 0;
    } else if (a == "--certify") certify = true;
    else if (a.compare(0, 10, "--certify=") == 0) certify = parse_bool(argv[i] + 10);
    else if (a == "--polish") polish = true;
    else if (a.compare(0, 9, "--polish=") == 0) polish = parse_bool(argv[i] + 9);
    else if (a == "--robust_polish") robust_polish = true;
    else if (a.compare(0, 16, "--robust_polish=") == 0) robust_polish = parse_bool(argv[i] + 16);
    else if (const char *v = val("--robust_covariance")) robust_covariance = v;
    else if (const char *v = val("--gnc_barc2")) gnc_barc2 = atof(v);
    else if (const char *v = val("--gnc_report")) gnc_report = v;
    else if (const char *v = val("--gnc_filtered")) gnc_filtered = v;
    else if (const char *v = val("--gnc")) gnc = v;
    else if (a == "--staircase") staircase = true;
    else if (a.compare(0, 12, "--staircase=") == 0) staircase = parse_bool(argv[i] + 12);
    else if (a == "--verify") verify = true;
    else if (a.compare(0, 9, "--verify=") == 0) verify = parse_bool(argv[i] + 9);
    else if (a == "--verify_reweighted") verify_reweighted = true;
    else if (a.compare(0, 20, "--verify_reweighted=") == 0) verify_reweighted = parse_bool(argv[i] + 20);
    else if (const char *v = val("--edge_report")) edge_report = v;
    else if (const char *v = val("--covariance")) covariance = v;
    else if (const char *v = val("--edge_reliability")) edge_reliability = v;
    else if (const char *v = val("--gate_candidates")) gate_candidates = v;
    else if (const char *v = val("--gate_report")) gate_report = v;
    else if (const char *v = val("--marginal_set")) marginal_set = v;
    else if (const char *v = val("--marginal_report")) marginal_report = v;
    else if (const char *v = val("--marginal_base")) marginal_base = atoi(v);
    else if (const char *v = val("--select_candidates")) select_candidates = v;
    else if (const char *v = val("--select_report")) select_report = v;
    else if (const char *v = val("--select_budget")) select_budget = atoi(v);
    else if (const char *v = val("--select_d2_max")) select_d2_max = atof(v);
    else if (const char *v = val("--hessian_modes")) hessian_modes = atoi(v);
    else if (const char *v = val("--modes_report")) modes_report = v;
    else if (a == "--modes_escape") modes_escape = true;
    else if (a.compare(0, 15, "--modes_escape=") == 0) modes_escape = parse_bool(argv[i] + 15);
    else if (const char *v = val("--sensitivity_pose")) sensitivity_pose = atoi(v);
    else if (const char *v = val("--sensitivity_report")) sensitivity_report = v;
    else if (const char *v = val("--dataset")) dataset = v;
    else if (const char *v = val("--num_nodes")) num_nodes = atoi(v);
    else if (const char *v = val("--iters")) iters = atoi(v);
    else if (const char *v = val("--dist_init")) dist_init = parse_bool(v);
    else if (const char *v = val("--loss")) loss_type = v;
    else if (const char *v = val("--accelerated")) accelerated = parse_bool(v);
    else if (const char *v = val("--save")) save = parse_bool(v);
    else if (const char *v = val("--gpu")) gpu = atoi(v);
    else if (const char *v = val("--rank")) rank = atoi(v);
    else if (const char *v = val("--world")) world = atoi(v);
    else if (const char *v = val("--rdv")) rdv = v;
  }
  if (gpu < 0) gpu = getenv("LOCAL_RANK") ? atoi(getenv("LOCAL_RANK")) : (world > 1 ? rank : 0);
  if (world < 1 || rank < 0 || rank >= world) { fprintf(stderr, "Inconsistent --rank / --world.\n"); return -1; }
  if (world > 1 && rdv.empty()) {
    // a name all ranks of this launch -- and no other launch -- agree on: the launcher's run id / port
    const char *run = getenv("TORCHELASTIC_RUN_ID"), *port = getenv("MASTER_PORT");
    if (!run && !port) { fprintf(stderr, "Several ranks need --rdv <directory> (or a launcher that sets MASTER_PORT).\n"); return -1; }
    rdv = std::string("/tmp/dpgo_rdv_") + std::to_string((long)geteuid()) + "_" + (run ? run : "none") + "_" + (port ? port : "0");
  }
  if (dataset.empty()) { fprintf(stderr, "No dataset has been specfied.\n"); return -1; }
  if (num_nodes < 1) { fprintf(stderr, "No number of nodes has been specfied.\n"); return -1; }
  int loss;
  if (loss_type == "trivial") loss = 0;
  else if (loss_type == "huber") loss = 1;
  else if (loss_type == "welsch") loss = 3;
  else { fprintf(stderr, " The loss type can only be \"trivial\", \"huber\" or \"welsch\".\n"); return -1; }

  dpgo_graph_t *g = nullptr;
  if (dpgo_read_g2o(dataset.c_str(), num_nodes, &g) != 0) return -1;
  int d, N, nn, m;
  dpgo_graph_info(g, &d, &N, &nn, &m);
  dpgo_options_t opt;
  dpgo_options_driver(&opt, loss, accelerated);
  const int ld = (d + 1) * N;
  std::vector<double> X((size_t)ld * d, 0.0);
  if (num_nodes % world != 0) { fprintf(stderr, "The number of nodes must be a multiple of the number of ranks.\n"); return -1; }
  const int per = num_nodes / world;
  std::vector<int> ids(per);
  for (int a = 0; a < per; a++) ids[a] = rank * per + a;
  const bool root = rank == 0;
  dpgo_group_t *grp = nullptr;
  if (dpgo_group_create(g, ids.data(), per, &opt, gpu, &grp) != 0) return -1;
  dpgo_comm_t *comm = nullptr;
  if (world > 1 || getenv("DPGO_FORCE_COMM")) {   // (DPGO_FORCE_COMM: a world of one rank still runs the whole protocol)
    unsigned char id[128];
    if (root && dpgo_comm_unique_id(id) != 0) return -1;
    if (world > 1 && dpgo_rdv::rendezvous(rdv, rank, world, id) != 0) return -1;
    if (dpgo_comm_create(grp, rank, world, id, &comm) != 0) return -1;
    dpgo_comm_barrier(comm);
  }
  if (dist_init) {
    // every node of the graph takes part in the distributed initialisation; with several ranks each runs the schedule
    // for its own nodes and the stage halos travel through the communicator (dchordal.cpp)
    dpgo_dchordal_options_t co;
    dpgo_dchordal_options_default(&co);
    int cap = 0;
    for (int k = 0; k < 4; k++) cap += (co.iters[k] + 19) / 20;
    std::vector<double> obj(cap);
    if (dpgo_group_dist_chordal_initialization(grp, &co, nullptr, 0, X.data(), ld, obj.data(), &cap) != 0) return -1;
    const char *names[4] = {"Initialize the reduced rotation", "Initialize the rotation", "Initialize the reduced translation",
                            "Initialize the translation"};
    int at = 0;
    for (int k = 0; k < 4 && root; k++) {
      printf("===============================================\n%s\n-----------------------------------------------\n", names[k]);
      for (int it = 0; it < co.iters[k]; it += 20) printf("%d: %.16g\n", it, obj[at++]);
    }
  } else {
    if (root) printf("===============================================\nInitialization\n-----------------------------------------------\n");
    if (dpgo_chordal_initialization(g, X.data(), ld) != 0) return -1;
  }
  if (dpgo_group_initialize_global(grp, X.data(), ld) != 0) return -1;
  if (dpgo_group_update(grp, nullptr, 0) != 0) return -1;

  auto evaluate = [&](double &fobj, double &grad) {
    double v[2] = {0, 0};
    for (int a = 0; a < per; a++) {
      dpgo_results_t r;
      dpgo_group_results(grp, a, &r);
      v[0] += r.fobj;
      v[1] += r.gradFnorm * r.gradFnorm;
    }
    if (comm) dpgo_comm_allreduce_sum(comm, v, 2);
    fobj = 2 * v[0];
    grad = 2 * std::sqrt(v[1]);
  };
  double fobj, grad, time = 0;
  evaluate(fobj, grad);
  std::vector<std::vector<double>> results;
  results.push_back({0, 0, fobj, grad});
  if (root) printf("===============================================\nDistributed PGO\n-----------------------------------------------\n");
  using clk = std::chrono::steady_clock;
  for (int iter = 0; iter < iters; iter++) {
    if (root) printf("%d: %.20g %.20g\n", iter, fobj, grad);
    auto t0 = clk::now();
    if (dpgo_group_iterate(grp, nullptr, 0) != 0) return -1;
    dpgo_group_sync(grp);
    time += std::chrono::duration<double>(clk::now() - t0).count();
    if (comm && dpgo_comm_exchange(comm) != 0) return -1;   // neighbours on other GPUs: RCCL, joined by update()
    dpgo_group_communicate_local(grp);
    t0 = clk::now();
    if (dpgo_group_update(grp, nullptr, 0) != 0) return -1;
    dpgo_group_sync(grp);
    time += std::chrono::duration<double>(clk::now() - t0).count();
    evaluate(fobj, grad);
    results.push_back({double(iter) + 1, time, fobj, grad});
  }
  if (root)
    printf("---------------------------------------\nfinal objective: %.20g\nfinal gradient: %.20g\ntime: %.20g s/node.\n", fobj,
           grad, time / per);
  // the point every later step acts on: the optimiser's, or the polished one
  std::vector<double> Xpol;
  auto final_point = [&](double *out) -> int {
    if (!Xpol.empty()) {
      std::copy(Xpol.begin(), Xpol.end(), out);
      return 0;
    }
    return dpgo_group_scatter_global(grp, out, ld);
  };
  // the robust objective and graduated non-convexity: a trivial-loss group of the same graph, built once for all their flags
  dpgo_group_t *post = nullptr;
  auto post_group = [&]() -> int {
    if (post) return 0;
    dpgo_options_t po;
    dpgo_options_driver(&po, 0, accelerated);
    po.max_iterations = 0;
    return dpgo_group_create(g, ids.data(), per, &po, gpu, &post);
  };
  if (!gnc.empty()) {
    if (gnc != "tls" && gnc != "gm") {
      fprintf(stderr, "--gnc takes tls or gm.\n");
      return -1;
    }
    if (world > 1) {
      if (root) printf("gnc: not computed (the group must host every node; %d ranks)\n", world);
    } else {
      std::vector<double> Xc((size_t)ld * d, 0.0), Z((size_t)ld * d, 0.0), w(m, 1.0);
      dpgo_gnc_options_t go;
      dpgo_gnc_options_default(&go);
      go.kind = gnc == "tls" ? DPGO_GNC_TLS : DPGO_GNC_GM;
      go.barc2 = gnc_barc2;
      dpgo_gnc_result_t gr;
      if (final_point(Xc.data()) != 0 || post_group() != 0 ||
          dpgo_group_gnc(post, g, Xc.data(), ld, &go, nullptr, 0, Z.data(), ld, w.data(), nullptr, 0, &gr) != 0)
        return -1;
      printf("gnc: %s %d %d %d %d %d %d %d %.17g %.17g %.17g %.17g %.17g\n",
             gr.outcome == DPGO_GNC_CONVERGED ? "CONVERGED" : gr.outcome == DPGO_GNC_ALL_INLIERS ? "ALL_INLIERS"
             : gr.outcome == DPGO_GNC_MAX_LEVELS ? "MAX_LEVELS" : gr.outcome == DPGO_GNC_INNER_FAILED ? "INNER_FAILED" : "SKIPPED",
             gr.levels, gr.steps, gr.factorisations, gr.num_robust, gr.num_zero, gr.num_between, gr.num_outliers, gr.mu_initial,
             gr.mu_final, gr.F_initial, gr.F_weighted_final, gr.F_surrogate_final);
      if (gr.outcome != DPGO_GNC_SKIPPED) {
        if (!gnc_report.empty()) {
          std::vector<int> I(m), J(m);
          std::vector<double> sr(m), st(m), wb(m), sums(8);
          if (dpgo_graph_edges(g, I.data(), J.data(), nullptr, nullptr, nullptr, nullptr) != 0 ||
              dpgo_group_gnc_eval(post, g, Z.data(), ld, go.kind, gr.mu_final > 0 ? gr.mu_final : 1.0, go.barc2, nullptr, w.data(), sr.data(),
                                  st.data(), wb.data(), sums.data()) != 0)
            return -1;
          std::vector<int> first(nn);
          for (int a = 0; a < nn; a++) first[a] = dpgo_graph_node_offset(g, a);   // (-1: a node without an edge)
          auto node_of = [&](int p) {
            int r = 0;
            for (int a = 0; a < nn; a++)
              if (first[a] >= 0 && p >= first[a]) r = a;
            return r;
          };
          FILE *f = fopen(gnc_report.c_str(), "w");
          if (!f) { fprintf(stderr, "Cannot write %s.\n", gnc_report.c_str()); return -1; }
          for (int e = 0; e < m; e++)
            fprintf(f, "%d %d %d %.17g %.17g\n", I[e], J[e], node_of(I[e]) != node_of(J[e]) ? 1 : 0, w[e], sr[e] + st[e]);
          fclose(f);
        }
        if (!gnc_filtered.empty()) {
          std::vector<unsigned char> keep(m);
          for (int e = 0; e < m; e++) keep[e] = w[e] != 0.0;
          dpgo_graph_t *kept = nullptr;
          if (dpgo_graph_filter_edges(g, keep.data(), &kept) != 0) return -1;
          const int rc = dpgo_write_g2o(kept, Z.data(), ld, gnc_filtered.c_str());
          dpgo_graph_free(kept);
          if (rc != 0) return -1;
        }
        Xpol.swap(Z);
      }
    }
  }
  if (polish) {
    if (loss != 0) {
      if (root) printf("polish: not computed (the Hessian is that of the trivial loss; --loss %s)\n", loss_type.c_str());
    } else if (world > 1) {
      if (root) printf("polish: not computed (the group must host every node; %d ranks)\n", world);
    } else {
      std::vector<double> Xc((size_t)ld * d, 0.0), Z((size_t)ld * d, 0.0);
      dpgo_polish_result_t pr;
      if (final_point(Xc.data()) != 0 ||
          dpgo_group_polish(grp, Xc.data(), ld, nullptr, 0, Z.data(), ld, nullptr, 0, &pr) != 0)
        return -1;
      printf("polish: %s %d %d %d %.17g %.17g %.17g %.17g\n",
             pr.outcome == DPGO_POLISH_CONVERGED ? "CONVERGED" : pr.outcome == DPGO_POLISH_MAX_STEPS ? "MAX_STEPS"
             : pr.outcome == DPGO_POLISH_STALLED ? "STALLED" : "SKIPPED",
             pr.steps, pr.factorisations, pr.indefinite, pr.F_initial, pr.F_final, pr.grad_initial, pr.grad_final);
      if (pr.outcome != DPGO_POLISH_SKIPPED) Xpol.swap(Z);
    }
  }
  if (hessian_modes != 0 || !modes_report.empty()) {
    if (hessian_modes == 0 || modes_report.empty()) {
      fprintf(stderr, "--hessian_modes and --modes_report go together.\n");
      return -1;
    }
    if (loss != 0) {
      if (root) printf("modes: not computed (the Hessian is that of the trivial loss; --loss %s)\n", loss_type.c_str());
    } else if (world > 1) {
      if (root) printf("modes: not computed (the group must host every node; %d ranks)\n", world);
    } else {
      const int dof = d + d * (d - 1) / 2, n = dof * N, k = hessian_modes, kk = std::max(k, 1);
      std::vector<double> Xc((size_t)ld * d, 0.0), Z((size_t)ld * d, 0.0), val((size_t)kk), res((size_t)kk), vec((size_t)kk * n),
          en((size_t)kk * N);
      dpgo_modes_options_t mo;
      dpgo_modes_options_default(&mo);
      mo.want_escape = modes_escape ? 1 : 0;
      dpgo_modes_result_t mr;
      if (final_point(Xc.data()) != 0 ||
          dpgo_group_hessian_modes(grp, Xc.data(), ld, 0, k, &mo, 0, val.data(), res.data(), vec.data(), en.data(), Z.data(), &mr) != 0) {
        fprintf(stderr, "--hessian_modes takes 1 ... 60, at most dof (num_poses - 1).\n");
        return -1;
      }
      printf("modes: %s %d %d %d %d %d %.17g %.17g %lld %d %.17g %.17g\n",
             mr.outcome == DPGO_MODES_CONVERGED ? "CONVERGED" : mr.outcome == DPGO_MODES_MAX_ITERS ? "MAX_ITERS"
             : mr.outcome == DPGO_MODES_STALLED ? "STALLED" : "SKIPPED",
             mr.iterations, mr.factorisations, mr.shift_tries, mr.block, mr.negative, val[0], mr.mu, mr.device_bytes, mr.escaped, mr.F,
             mr.F_escape);
      if (mr.outcome == DPGO_MODES_CONVERGED || mr.outcome == DPGO_MODES_MAX_ITERS) {
        FILE *f = fopen(modes_report.c_str(), "w");
        if (!f) { fprintf(stderr, "Cannot write %s.\n", modes_report.c_str()); return -1; }
        fprintf(f, "k %d n %d mu %.17g hmax %.17g\n", k, n, mr.mu, mr.hmax);
        for (int j = 0; j < k; j++) {
          const double *e = &en[(size_t)j * N];
          const int top = (int)(std::max_element(e, e + N) - e);
          fprintf(f, "%d %.17g %.17g %d %.17g\n", j, val[j], res[j], top, e[top]);
          for (int i = 0; i < n; i++) fprintf(f, "%s%.17g", i ? " " : "", vec[(size_t)j * n + i]);
          fprintf(f, "\n");
        }
        fclose(f);
      }
      if (mr.escaped) Xpol.swap(Z);
    }
  }
  if (staircase) {
    if (loss != 0) {
      if (root) printf("staircase: not computed (the relaxation is that of the trivial loss; --loss %s)\n", loss_type.c_str());
    } else if (world > 1) {
      if (root) printf("staircase: not computed (the group must host every node; %d ranks)\n", world);
    } else {
      std::vector<double> Xc((size_t)ld * d, 0.0), Z((size_t)ld * d, 0.0);
      dpgo_staircase_result_t sr;
      if (final_point(Xc.data()) != 0 ||
          dpgo_group_staircase(grp, Xc.data(), ld, nullptr, 0, Z.data(), ld, nullptr, 0, nullptr, 0, &sr) != 0)
        return -1;
      printf("staircase: %s %d %.17g %.17g %.17g %.17g\n",
             sr.outcome == DPGO_STAIR_SOLVED ? "SOLVED" : sr.outcome == DPGO_STAIR_MAX_RANK ? "MAX_RANK"
             : sr.outcome == DPGO_STAIR_SADDLE ? "SADDLE" : "SKIPPED",
             sr.final_rank, sr.F_initial, sr.F_sdp, sr.F_final, sr.gap);
      if (sr.outcome != DPGO_STAIR_SKIPPED) Xpol.swap(Z);
    }
  }
  if (robust_polish) {
    if (loss == 0) {
      if (root) printf("robust polish: not computed (the loss is trivial: --polish is the call)\n");
    } else if (world > 1) {
      if (root) printf("robust polish: not computed (the group must host every node; %d ranks)\n", world);
    } else {
      std::vector<double> Xc((size_t)ld * d, 0.0), Z((size_t)ld * d, 0.0);
      dpgo_polish_result_t pr;
      if (final_point(Xc.data()) != 0 || post_group() != 0 ||
          dpgo_group_robust_polish(post, g, Xc.data(), ld, loss, opt.loss_reg, 1, nullptr, 0, Z.data(), ld, nullptr, 0, &pr, nullptr) != 0)
        return -1;
      printf("robust polish: %s %d %d %d %.17g %.17g %.17g %.17g\n",
             pr.outcome == DPGO_POLISH_CONVERGED ? "CONVERGED" : pr.outcome == DPGO_POLISH_MAX_STEPS ? "MAX_STEPS"
             : pr.outcome == DPGO_POLISH_STALLED ? "STALLED" : "SKIPPED",
             pr.steps, pr.factorisations, pr.indefinite, pr.F_initial, pr.F_final, pr.grad_initial, pr.grad_final);
      if (pr.outcome != DPGO_POLISH_SKIPPED) Xpol.swap(Z);
    }
  }
  if (certify) {
    if (loss != 0) {
      if (root) printf("certificate: not computed (the certificate is that of the trivial loss; --loss %s)\n", loss_type.c_str());
    } else if (world > 1) {
      if (root) printf("certificate: not computed (the group must host every node; %d ranks)\n", world);
    } else {
      std::vector<double> Xc((size_t)ld * d, 0.0);
      dpgo_cert_options_t co;
      dpgo_cert_options_default(&co);
      dpgo_cert_result_t cr;
      if (final_point(Xc.data()) != 0 || dpgo_group_certify(grp, Xc.data(), ld, &co, nullptr, 0, &cr, nullptr, 0) != 0)
        return -1;
      printf("certificate: %s %.16g %.16g %d %.16g\n",
             cr.status == DPGO_CERT_NEGATIVE ? "NEGATIVE" : cr.status == DPGO_CERT_NONNEGATIVE ? "NONNEGATIVE" : "UNDECIDED", cr.theta,
             cr.residual, cr.iterations, cr.stationarity);
    }
  }
  if (verify) {
    if (loss != 0) {
      if (root) printf("verification: not computed (the certificate is that of the trivial loss; --loss %s)\n", loss_type.c_str());
    } else if (world > 1) {
      if (root) printf("verification: not computed (the group must host every node; %d ranks)\n", world);
    } else {
      std::vector<double> Xc((size_t)ld * d, 0.0);
      dpgo_cert_options_t co;
      dpgo_cert_options_default(&co);
      dpgo_cert_result_t cr;
      dpgo_cert_factor_t cf;
      if (final_point(Xc.data()) != 0 ||
          dpgo_group_verify(grp, Xc.data(), ld, &co, 0, nullptr, 0, &cr, nullptr, 0, &cf) != 0)
        return -1;
      printf("verification: %s %s %.16g %.16g %.16g %d %.16g\n",
             cr.status == DPGO_CERT_PROVEN ? "PROVEN" : cr.status == DPGO_CERT_NEGATIVE ? "NEGATIVE"
             : cr.status == DPGO_CERT_NONNEGATIVE ? "NONNEGATIVE" : "UNDECIDED",
             cf.outcome == DPGO_CERT_FACTOR_PD ? "PD" : cf.outcome == DPGO_CERT_FACTOR_NOT_PD ? "NOT_PD" : "SKIPPED", cf.pivot_min,
             cr.theta, cr.residual, cr.iterations, cr.stationarity);
    }
  }
  if (!edge_report.empty() || verify_reweighted) {
    if (world > 1) {
      if (root && !edge_report.empty()) printf("edge report: not written (the edge evaluation needs the whole X on one rank; %d ranks)\n", world);
      if (root && verify_reweighted) printf("reweighted verification: not computed (the group must host every node; %d ranks)\n", world);
    } else {
      std::vector<double> Xc((size_t)ld * d, 0.0);
      if (final_point(Xc.data()) != 0) return -1;
      if (!edge_report.empty()) {
        std::vector<int> I(m), J(m);
        std::vector<double> sr(m), st(m), rho(m), w(m);
        dpgo_edge_eval_t *ev = nullptr;
        if (dpgo_graph_edges(g, I.data(), J.data(), nullptr, nullptr, nullptr, nullptr) != 0 || dpgo_edge_eval_create(g, gpu, &ev) != 0) return -1;
        const int rc = dpgo_edge_eval_run(ev, Xc.data(), ld, loss, opt.loss_reg, sr.data(), st.data(), rho.data(), w.data(), nullptr);
        dpgo_edge_eval_free(ev);
        if (rc != 0) return -1;
        // (inter: the weight of an intra-node edge is 1 by definition, so the flag is the partition's, from the node ranges)
        std::vector<int> first(nn);
        for (int a = 0; a < nn; a++) first[a] = dpgo_graph_node_offset(g, a);   // (-1: a node without an edge)
        auto node_of = [&](int p) {
          int r = 0;
          for (int a = 0; a < nn; a++)
            if (first[a] >= 0 && p >= first[a]) r = a;
          return r;
        };
        FILE *f = fopen(edge_report.c_str(), "w");
        if (!f) { fprintf(stderr, "Cannot write %s.\n", edge_report.c_str()); return -1; }
        for (int e = 0; e < m; e++)
          fprintf(f, "%d %d %d %d %.16g %.16g %.16g %.16g\n", e, I[e], J[e], node_of(I[e]) != node_of(J[e]) ? 1 : 0, sr[e], st[e], rho[e], w[e]);
        fclose(f);
      }
      if (verify_reweighted) {
        dpgo_cert_options_t co;
        dpgo_cert_options_default(&co);
        dpgo_cert_result_t cr;
        dpgo_cert_factor_t cf;
        dpgo_edge_summary_t es;
        if (dpgo_graph_verify_reweighted(g, gpu, Xc.data(), ld, loss, opt.loss_reg, &co, 0, &cr, &cf, &es, nullptr, 0) != 0) return -1;
        printf("reweighted verification: %s %s %.16g %.16g %.16g %d %.16g %d/%d %.16g\n",
               cr.status == DPGO_CERT_PROVEN ? "PROVEN" : cr.status == DPGO_CERT_NEGATIVE ? "NEGATIVE"
               : cr.status == DPGO_CERT_NONNEGATIVE ? "NONNEGATIVE" : "UNDECIDED",
               cf.outcome == DPGO_CERT_FACTOR_PD ? "PD" : cf.outcome == DPGO_CERT_FACTOR_NOT_PD ? "NOT_PD" : "SKIPPED", cf.pivot_min,
               cr.theta, cr.residual, cr.iterations, cr.stationarity, es.num_downweighted, es.num_inter, es.weight_min);
      }
    }
  }
  if (!covariance.empty()) {
    if (loss != 0) {
      if (root) printf("covariance: not computed (the Hessian is that of the trivial loss; --loss %s)\n", loss_type.c_str());
    } else if (world > 1) {
      if (root) printf("covariance: not computed (the group must host every node; %d ranks)\n", world);
    } else {
      const int dof = d + d * (d - 1) / 2;
      std::vector<double> Xc((size_t)ld * d, 0.0), marg((size_t)N * dof * dof, 0.0);
      dpgo_cov_result_t cv;
      if (final_point(Xc.data()) != 0 ||
          dpgo_group_covariance(grp, Xc.data(), ld, 0, 0, nullptr, 0, marg.data(), nullptr, &cv) != 0)
        return -1;
      printf("covariance: %s %d %d %d %d %lld %.16g %.16g\n",
             cv.outcome == DPGO_COV_OK ? "OK" : cv.outcome == DPGO_COV_NOT_PD ? "NOT_PD" : "SKIPPED", cv.unknowns, cv.fronts, cv.levels,
             cv.max_front, cv.device_bytes, cv.pivot_min, cv.stationarity);
      if (cv.outcome == DPGO_COV_OK) {
        FILE *f = fopen(covariance.c_str(), "w");
        if (!f) { fprintf(stderr, "Cannot write %s.\n", covariance.c_str()); return -1; }
        for (int p = 0; p < N; p++) {
          fprintf(f, "%d", p);
          for (int a = 0; a < dof; a++)
            for (int b = a; b < dof; b++) fprintf(f, " %.17g", marg[((size_t)p * dof + a) * dof + b]);
          fprintf(f, "\n");
        }
        fclose(f);
      }
    }
  }
  if (!robust_covariance.empty()) {
    if (loss == 0) {
      if (root) printf("robust covariance: not computed (the loss is trivial: --covariance is the call)\n");
    } else if (world > 1) {
      if (root) printf("robust covariance: not computed (the group must host every node; %d ranks)\n", world);
    } else {
      const int dof = d + d * (d - 1) / 2;
      std::vector<double> Xc((size_t)ld * d, 0.0), marg((size_t)N * dof * dof, 0.0);
      dpgo_cov_result_t cv;
      if (final_point(Xc.data()) != 0 || post_group() != 0 ||
          dpgo_group_robust_covariance(post, g, Xc.data(), ld, loss, opt.loss_reg, 1, 0, 0, nullptr, 0, marg.data(), nullptr, &cv) != 0)
        return -1;
      printf("robust covariance: %s %d %d %d %d %lld %.16g %.16g\n",
             cv.outcome == DPGO_COV_OK ? "OK" : cv.outcome == DPGO_COV_NOT_PD ? "NOT_PD" : "SKIPPED", cv.unknowns, cv.fronts, cv.levels,
             cv.max_front, cv.device_bytes, cv.pivot_min, cv.stationarity);
      if (cv.outcome == DPGO_COV_OK) {
        FILE *f = fopen(robust_covariance.c_str(), "w");
        if (!f) { fprintf(stderr, "Cannot write %s.\n", robust_covariance.c_str()); return -1; }
        for (int p = 0; p < N; p++) {
          fprintf(f, "%d", p);
          for (int a = 0; a < dof; a++)
            for (int b = a; b < dof; b++) fprintf(f, " %.17g", marg[((size_t)p * dof + a) * dof + b]);
          fprintf(f, "\n");
        }
        fclose(f);
      }
    }
  }
  if (!gate_candidates.empty() || !gate_report.empty()) {
    if (gate_candidates.empty() || gate_report.empty()) {
      fprintf(stderr, "--gate_candidates and --gate_report go together.\n");
      return -1;
    }
    if (loss != 0) {
      if (root) printf("gate: not computed (the Hessian is that of the trivial loss; --loss %s)\n", loss_type.c_str());
    } else if (world > 1) {
      if (root) printf("gate: not computed (the group must host every node; %d ranks)\n", world);
    } else {
      dpgo_graph_t *cg = nullptr;
      int cd = 0, cN = 0, cn = 0, m = 0;
      if (dpgo_read_g2o(gate_candidates.c_str(), 1, &cg) != 0 || dpgo_graph_info(cg, &cd, &cN, &cn, &m) != 0 || cd != d || cN > N) {
        fprintf(stderr, "Cannot use the candidates in %s (unreadable, another dimension, or a pose that is not in the graph).\n",
                gate_candidates.c_str());
        dpgo_graph_free(cg);
        return -1;
      }
      const int dof = d + d * (d - 1) / 2, nc = d * d + d + 2;
      std::vector<int> I(m), J(m), pairs((size_t)2 * m);
      std::vector<double> R((size_t)m * d * d), t((size_t)m * d), kappa(m), tau(m), cand((size_t)m * nc);
      const int got = dpgo_graph_edges(cg, I.data(), J.data(), R.data(), t.data(), kappa.data(), tau.data());
      dpgo_graph_free(cg);
      if (got != 0) {
        fprintf(stderr, "Cannot read the edges of %s.\n", gate_candidates.c_str());
        return -1;
      }
      for (int k = 0; k < m; k++) {
        pairs[2 * k] = I[k]; pairs[2 * k + 1] = J[k];
        std::copy(&R[(size_t)k * d * d], &R[(size_t)(k + 1) * d * d], &cand[(size_t)k * nc]);
        std::copy(&t[(size_t)k * d], &t[(size_t)(k + 1) * d], &cand[(size_t)k * nc + d * d]);
        cand[(size_t)k * nc + d * d + d] = kappa[k];
        cand[(size_t)k * nc + d * d + d + 1] = tau[k];
      }
      std::vector<double> Xc((size_t)ld * d, 0.0), joint((size_t)m * 3 * dof * dof), rel((size_t)m * dof * dof), gate((size_t)m * (2 + dof));
      dpgo_pairs_result_t pr;
      if (final_point(Xc.data()) != 0 ||
          dpgo_group_pair_covariance(grp, Xc.data(), ld, 0, 0, pairs.data(), m, cand.data(), joint.data(), rel.data(), gate.data(), &pr) != 0)
        return -1;
      printf("gate: %s %d %d %d %lld %.16g %.16g\n",
             pr.outcome == DPGO_PAIRS_OK ? "OK" : pr.outcome == DPGO_PAIRS_NOT_PD ? "NOT_PD" : "SKIPPED", m, pr.columns, pr.batches,
             pr.device_bytes, pr.pivot_min, pr.stationarity);
      if (pr.outcome == DPGO_PAIRS_OK) {
        FILE *f = fopen(gate_report.c_str(), "w");
        if (!f) { fprintf(stderr, "Cannot write %s.\n", gate_report.c_str()); return -1; }
        for (int k = 0; k < m; k++) {
          fprintf(f, "%d %d %.17g %d %d", I[k], J[k], gate[(size_t)k * (2 + dof)], dof, gate[(size_t)k * (2 + dof) + 1] != 0.0 ? 1 : 0);
          for (int a = 0; a < dof; a++)
            for (int b = a; b < dof; b++) fprintf(f, " %.17g", rel[((size_t)k * dof + a) * dof + b]);
          fprintf(f, "\n");
        }
        fclose(f);
      }
    }
  }
  if (sensitivity_pose >= 0 || !sensitivity_report.empty()) {
    if (sensitivity_pose < 0 || sensitivity_pose >= N || sensitivity_report.empty()) {
      fprintf(stderr, "--sensitivity_pose (a pose of the graph) and --sensitivity_report go together.\n");
      return -1;
    }
    if (loss != 0 && robust_polish && world == 1) {
      // the robust objective at the robust polish's point: one more value per row, the edge's term of d/ddelta, and a last line
      // "delta" with the dof values of d x_pose / d delta
      int gd = 0, gN = 0, gn = 0, m = 0;
      if (dpgo_graph_info(g, &gd, &gN, &gn, &m) != 0) return -1;
      const int dof = d + d * (d - 1) / 2, no = 3 + dof;
      const size_t n = (size_t)dof * N;
      std::vector<int> I(m), J(m);
      std::vector<double> R((size_t)m * d * d), t((size_t)m * d), kappa(m), tau(m);
      if (dpgo_graph_edges(g, I.data(), J.data(), R.data(), t.data(), kappa.data(), tau.data()) != 0) return -1;
      std::vector<double> Xc((size_t)ld * d, 0.0), up(n * dof, 0.0), sens((size_t)dof * m * no, 0.0), dreg(dof, 0.0);
      for (int a = 0; a < dof; a++) up[(size_t)a * n + (size_t)dof * sensitivity_pose + a] = 1.0;
      dpgo_sens_result_t sr;
      if (final_point(Xc.data()) != 0 || post_group() != 0 ||
          dpgo_group_robust_sensitivity(post, g, Xc.data(), ld, loss, opt.loss_reg, 0, 0, up.data(), (int)n, dof, nullptr, sens.data(),
                                        dreg.data(), &sr) != 0)
        return -1;
      printf("robust sensitivity: %s %d %d %d %d %lld %.16g %.16g\n",
             sr.outcome == DPGO_SENS_OK ? "OK" : sr.outcome == DPGO_SENS_NOT_PD ? "NOT_PD" : "SKIPPED", sensitivity_pose, sr.edges,
             sr.columns, sr.batches, sr.device_bytes, sr.pivot_min, sr.stationarity);
      if (sr.outcome == DPGO_SENS_OK) {
        auto node_of = [&](int p) {
          int a = 0;
          while (a + 1 < num_nodes && dpgo_graph_node_offset(g, a + 1) <= p) a++;
          return a;
        };
        FILE *f = fopen(sensitivity_report.c_str(), "w");
        if (!f) { fprintf(stderr, "Cannot write %s.\n", sensitivity_report.c_str()); return -1; }
        for (int e = 0; e < m; e++) {
          fprintf(f, "%d %d %d %d", e, I[e], J[e], node_of(I[e]) != node_of(J[e]) ? 1 : 0);
          for (int a = 0; a < dof; a++)
            for (int b = 0; b < no; b++) fprintf(f, " %.17g", sens[((size_t)a * m + e) * no + b]);
          fprintf(f, "\n");
        }
        fprintf(f, "delta");
        for (int a = 0; a < dof; a++) fprintf(f, " %.17g", dreg[a]);
        fprintf(f, "\n");
        fclose(f);
      }
    } else if (loss != 0) {
      if (root) printf("sensitivity: not computed (the Hessian is that of the trivial loss; --loss %s)\n", loss_type.c_str());
    } else if (world > 1) {
      if (root) printf("sensitivity: not computed (the group must host every node; %d ranks)\n", world);
    } else if (!polish) {
      if (root) printf("sensitivity: not computed (it is taken at a critical point: --polish)\n");
    } else {
      int gd = 0, gN = 0, gn = 0, m = 0;
      if (dpgo_graph_info(g, &gd, &gN, &gn, &m) != 0) return -1;
      const int dof = d + d * (d - 1) / 2, no = 2 + dof;
      const size_t n = (size_t)dof * N;
      std::vector<int> I(m), J(m);
      std::vector<double> R((size_t)m * d * d), t((size_t)m * d), kappa(m), tau(m);
      if (dpgo_graph_edges(g, I.data(), J.data(), R.data(), t.data(), kappa.data(), tau.data()) != 0) return -1;
      // the dof unit columns of the pose: row a of the report's block of an edge is d x_pose[a] / d (kappa, tau, t~, eta)
      std::vector<double> Xc((size_t)ld * d, 0.0), up(n * dof, 0.0), sens((size_t)dof * m * no, 0.0);
      for (int a = 0; a < dof; a++) up[(size_t)a * n + (size_t)dof * sensitivity_pose + a] = 1.0;
      dpgo_sens_result_t sr;
      if (final_point(Xc.data()) != 0 ||
          dpgo_group_sensitivity(grp, g, Xc.data(), ld, 0, 0, up.data(), (int)n, dof, nullptr, sens.data(), &sr) != 0)
        return -1;
      printf("sensitivity: %s %d %d %d %d %lld %.16g %.16g\n",
             sr.outcome == DPGO_SENS_OK ? "OK" : sr.outcome == DPGO_SENS_NOT_PD ? "NOT_PD" : "SKIPPED", sensitivity_pose, sr.edges,
             sr.columns, sr.batches, sr.device_bytes, sr.pivot_min, sr.stationarity);
      if (sr.outcome == DPGO_SENS_OK) {
        auto node_of = [&](int p) {
          int a = 0;
          while (a + 1 < num_nodes && dpgo_graph_node_offset(g, a + 1) <= p) a++;
          return a;
        };
        FILE *f = fopen(sensitivity_report.c_str(), "w");
        if (!f) { fprintf(stderr, "Cannot write %s.\n", sensitivity_report.c_str()); return -1; }
        for (int e = 0; e < m; e++) {
          fprintf(f, "%d %d %d %d", e, I[e], J[e], node_of(I[e]) != node_of(J[e]) ? 1 : 0);
          for (int a = 0; a < dof; a++)
            for (int b = 0; b < no; b++) fprintf(f, " %.17g", sens[((size_t)a * m + e) * no + b]);
          fprintf(f, "\n");
        }
        fclose(f);
      }
    }
  }
  if (!edge_reliability.empty()) {
    if (loss != 0) {
      if (root) printf("reliability: not computed (the Hessian is that of the trivial loss; --loss %s)\n", loss_type.c_str());
    } else if (world > 1) {
      if (root) printf("reliability: not computed (the group must host every node; %d ranks)\n", world);
    } else if (!polish) {
      if (root) printf("reliability: not computed (it is taken at a critical point: --polish)\n");
    } else {
      int gd = 0, gN = 0, gn = 0, m = 0;
      if (dpgo_graph_info(g, &gd, &gN, &gn, &m) != 0) return -1;
      const int dof = d + d * (d - 1) / 2, w = 6 + 2 * dof;
      std::vector<int> I(m), J(m);
      std::vector<double> R((size_t)m * d * d), t((size_t)m * d), kappa(m), tau(m);
      if (dpgo_graph_edges(g, I.data(), J.data(), R.data(), t.data(), kappa.data(), tau.data()) != 0) return -1;
      std::vector<double> Xc((size_t)ld * d, 0.0), rec((size_t)m * w, 0.0);
      dpgo_rely_result_t rr;
      if (final_point(Xc.data()) != 0 ||
          dpgo_group_edge_reliability(grp, g, Xc.data(), ld, 0, 0, DPGO_RELY_AUTO, nullptr, 0, rec.data(), nullptr, nullptr, &rr) != 0)
        return -1;
      printf("reliability: %s %s %d %d %d %.17g %lld %.16g %.16g\n",
             rr.outcome == DPGO_RELY_OK ? "OK" : rr.outcome == DPGO_RELY_NOT_PD ? "NOT_PD" : "SKIPPED",
             rr.method_used == DPGO_RELY_SELINV ? "SELINV" : rr.method_used == DPGO_RELY_SOLVE ? "SOLVE" : "AUTO", rr.edges, rr.flagged,
             rr.unweighted, rr.redundancy_sum, rr.device_bytes, rr.pivot_min, rr.stationarity);
      if (rr.outcome == DPGO_RELY_OK) {
        FILE *f = fopen(edge_reliability.c_str(), "w");
        if (!f) { fprintf(stderr, "Cannot write %s.\n", edge_reliability.c_str()); return -1; }
        for (int e = 0; e < m; e++) {
          const double *q = &rec[(size_t)e * w];
          fprintf(f, "%d %d %d %.17g %.17g %.17g %.17g %d %.17g\n", e, I[e], J[e], q[2], q[3], q[4], q[0], (int)q[1], q[5]);
        }
        fclose(f);
      }
    }
  }
  if (!marginal_set.empty() || !marginal_report.empty()) {
    if (marginal_set.empty() || marginal_report.empty()) {
      fprintf(stderr, "--marginal_set and --marginal_report go together.\n");
      return -1;
    }
    if (loss != 0) {
      if (root) printf("marginal: not computed (the Hessian is that of the trivial loss; --loss %s)\n", loss_type.c_str());
    } else if (world > 1) {
      if (root) printf("marginal: not computed (the group must host every node; %d ranks)\n", world);
    } else {
      std::vector<int> keep;
      FILE *in = fopen(marginal_set.c_str(), "r");
      if (!in) { fprintf(stderr, "Cannot read %s.\n", marginal_set.c_str()); return -1; }
      for (int p; fscanf(in, "%d", &p) == 1;) keep.push_back(p);
      fclose(in);
      const int K = (int)keep.size(), dof = d + d * (d - 1) / 2, n = dof * (K - (marginal_base >= 0 ? 1 : 0));
      if (K < 1 || n < 1) { fprintf(stderr, "%s holds no kept set.\n", marginal_set.c_str()); return -1; }
      std::vector<double> Xc((size_t)ld * d, 0.0), cov((size_t)n * n, 0.0), info((size_t)n * n, 0.0);
      double logdet = 0.0;
      dpgo_marg_result_t mr;
      if (final_point(Xc.data()) != 0 ||
          dpgo_group_joint_marginal(grp, Xc.data(), ld, keep.data(), K, 0, marginal_base, 1, 0, cov.data(), info.data(), &logdet, &mr) != 0)
        return -1;
      printf("marginal: %s %d %d %d %d %lld %d %.17g %.16g\n",
             mr.outcome == DPGO_MARG_OK ? "OK" : mr.outcome == DPGO_MARG_NOT_PD ? "NOT_PD" : "SKIPPED", K, mr.n, mr.columns, mr.batches,
             mr.device_bytes, mr.info_not_pd, logdet, mr.stationarity);
      if (mr.outcome == DPGO_MARG_OK) {
        FILE *f = fopen(marginal_report.c_str(), "w");
        if (!f) { fprintf(stderr, "Cannot write %s.\n", marginal_report.c_str()); return -1; }
        fprintf(f, "n %d logdet %.17g\n", n, logdet);
        bool first = true;
        for (int p : keep)
          if (p != marginal_base) { fprintf(f, "%s%d", first ? "" : " ", p); first = false; }
        fprintf(f, "\n");
        for (const std::vector<double> *M : {&cov, &info})
          for (int i = 0; i < n; i++) {
            for (int j = 0; j < n; j++) fprintf(f, "%s%.17g", j ? " " : "", (*M)[(size_t)i * n + j]);
            fprintf(f, "\n");
          }
        fclose(f);
      }
    }
  }
  if (!select_candidates.empty() || !select_report.empty()) {
    if (select_candidates.empty() || select_report.empty()) {
      fprintf(stderr, "--select_candidates and --select_report go together.\n");
      return -1;
    }
    if (loss != 0) {
      if (root) printf("candidates: not computed (the Hessian is that of the trivial loss; --loss %s)\n", loss_type.c_str());
    } else if (world > 1) {
      if (root) printf("candidates: not computed (the group must host every node; %d ranks)\n", world);
    } else {
      dpgo_graph_t *cg = nullptr;
      int cd = 0, cN = 0, cn = 0, m = 0;
      if (dpgo_read_g2o(select_candidates.c_str(), 1, &cg) != 0 || dpgo_graph_info(cg, &cd, &cN, &cn, &m) != 0 || cd != d || cN > N || m < 1) {
        fprintf(stderr, "Cannot use the candidates in %s (unreadable, empty, another dimension, or a pose that is not in the graph).\n",
                select_candidates.c_str());
        dpgo_graph_free(cg);
        return -1;
      }
      const int dof = d + d * (d - 1) / 2, nc = d * d + d + 2, n = dof * m, budget = select_budget < 0 ? m : select_budget;
      std::vector<int> I(m), J(m), pairs((size_t)2 * m);
      std::vector<double> R((size_t)m * d * d), t((size_t)m * d), kappa(m), tau(m), cand((size_t)m * nc);
      const int got = dpgo_graph_edges(cg, I.data(), J.data(), R.data(), t.data(), kappa.data(), tau.data());
      dpgo_graph_free(cg);
      if (got != 0) {
        fprintf(stderr, "Cannot read the edges of %s.\n", select_candidates.c_str());
        return -1;
      }
      for (int k = 0; k < m; k++) {
        pairs[2 * k] = I[k]; pairs[2 * k + 1] = J[k];
        std::copy(&R[(size_t)k * d * d], &R[(size_t)(k + 1) * d * d], &cand[(size_t)k * nc]);
        std::copy(&t[(size_t)k * d], &t[(size_t)(k + 1) * d], &cand[(size_t)k * nc + d * d]);
        cand[(size_t)k * nc + d * d + d] = kappa[k];
        cand[(size_t)k * nc + d * d + d + 1] = tau[k];
      }
      std::vector<double> Xc((size_t)ld * d, 0.0), S((size_t)n * n), res((size_t)n), info((size_t)n * n), steps((size_t)4 * std::max(budget, 1));
      std::vector<int> selected((size_t)std::max(budget, 1), -1), poses((size_t)2 * m);
      double sc[5] = {0, 0, 0, 0, 0};
      dpgo_cand_result_t cr;
      if (final_point(Xc.data()) != 0 ||
          dpgo_group_candidate_set(grp, Xc.data(), ld, pairs.data(), m, cand.data(), 0, budget, select_d2_max, 1, 0, nullptr, S.data(),
                                   res.data(), info.data(), sc, selected.data(), steps.data(), poses.data(), &cr) != 0)
        return -1;
      printf("candidates: %s %d %d %d %d %d %lld %d %d %.17g %.17g %.16g\n",
             cr.outcome == DPGO_CAND_OK ? "OK" : cr.outcome == DPGO_CAND_NOT_PD ? "NOT_PD" : "SKIPPED", m, cr.n, cr.poses, cr.columns,
             cr.batches, cr.device_bytes, cr.joint_not_pd, cr.n_selected, sc[1], sc[2], cr.stationarity);
      if (cr.outcome == DPGO_CAND_OK) {
        FILE *f = fopen(select_report.c_str(), "w");
        if (!f) { fprintf(stderr, "Cannot write %s.\n", select_report.c_str()); return -1; }
        fprintf(f, "n %d logdet %.17g d2_joint %.17g gain_all %.17g\n", n, sc[0], sc[1], sc[2]);
        fprintf(f, "selected %d gain %.17g d2 %.17g\n", cr.n_selected, sc[3], sc[4]);
        for (int k = 0; k < cr.n_selected; k++)
          fprintf(f, "%d %d %d %.17g %.17g %d\n", selected[k], I[selected[k]], J[selected[k]], steps[4 * (size_t)k + 1],
                  steps[4 * (size_t)k + 2], (int)steps[4 * (size_t)k + 3]);
        for (const std::vector<double> *M : {&S, &info})
          for (int i = 0; i < n; i++) {
            for (int j = 0; j < n; j++) fprintf(f, "%s%.17g", j ? " " : "", (*M)[(size_t)i * n + j]);
            fprintf(f, "\n");
          }
        fclose(f);
      }
    }
  }
  if (post) dpgo_group_free(post);
  if (save) {
    std::fill(X.begin(), X.end(), 0.0);
    final_point(X.data());
    if (comm) dpgo_comm_allreduce_sum(comm, X.data(), (long)X.size());   // every rank contributes its own poses
  }
  if (save && root) {
    const std::string resfile = "results_chordal_" + std::to_string(num_nodes) + "_" + (accelerated ? "amm" : "mm") + ".txt";
    FILE *f = fopen(resfile.c_str(), "w");
    if (!f) return -1;
    for (const auto &r : results) fprintf(f, "%d %.16g %.16g %.16g\n", (int)r[0], r[1], r[2], r[3]);
    fclose(f);
    // gauge fix (:554-558): t <- t - t_0 ; X <- X * R with R = X.middleRows(num_poses, d)^T
    std::vector<double> R(d * d), t0v(d);
    for (int c = 0; c < d; c++) {
      t0v[c] = X[(size_t)c * ld + 0];
      for (int r = 0; r < d; r++) R[r * d + c] = X[(size_t)r * ld + N + c];   // R(r,c) = block(c,r)
    }
    for (int i = 0; i < N; i++)
      for (int c = 0; c < d; c++) X[(size_t)c * ld + i] -= t0v[c];
    f = fopen(("./estimates_" + loss_type + ".txt").c_str(), "w");
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
  }
  if (comm) dpgo_comm_free(comm);
  dpgo_group_free(grp);
  dpgo_graph_free(g);
  return 0;
}
