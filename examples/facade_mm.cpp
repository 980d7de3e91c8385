// The reference driver's main loop (C++/examples/dist_pgo.cpp:446-531) written against the C++ facade
// include/dpgo_amd.hpp: read_g2o -> chordal init -> { iterate; communicate; update } with all nodes on GPU 0.
//   facade_mm <file.g2o> <num_nodes> <iters> [loss: trivial|huber|gm|welsch] [accelerated: 0|1] [certify|verify|reweighted|covariance|polish|ml_polish|robust_polish|gnc|ml_gnc <tls|gm> <barc2>|staircase|pairs <candidates.g2o>|modes <k>|sensitivity <pose>|robust_sensitivity <pose>|reliability|ml_reliability]
//   facade_mm --info <file.g2o> <num_nodes>        (host only: partition sizes, no GPU needed)
// Prints "<iter>: <2F> <2|grad F|>" like the reference (dist_pgo.cpp:493-494).  With a sixth argument `certify` the final
// point goes through DPGOHashGroup::verify_solution and the outcome is printed to STDERR (stdout stays the trace):
//   certificate: <NEGATIVE|NONNEGATIVE|UNDECIDED|FAILED> <theta> <residual> <iterations> <stationarity>
// and with `verify` through DPGOHashGroup::fast_verification (the Cholesky proof first, the search only if it fails):
//   verification: <PROVEN|NEGATIVE|NONNEGATIVE|UNDECIDED|FAILED> <PD|NOT_PD|SKIPPED> <pivot_min> <theta> <residual> <iterations> <stationarity>
// and with `reweighted` (any loss) through DPGO::EdgeEvaluation, Graph::scale_edges and DPGO::fast_verification_reweighted:
//   reweighted verification: <status> <outcome> <pivot_min> <theta> <iterations> <stationarity> <num_downweighted>/<num_inter> <weight_min> <scaled edges>
// and with `covariance` through DPGOHashGroup::marginal_covariances (trivial loss; pose 0 is the anchor), one line per pose:
//   covariance: <p> <upper triangle of Sigma_pp row by row, 17 digits>       then   covariance: <OK|NOT_PD|SKIPPED|FAILED> <fronts> <levels> <stationarity>
// and with `polish` through DPGOHashGroup::newton_polish (trivial loss; pose 0 is the anchor), one line per row of the new point:
//   polish: x <row> <the d entries, 17 digits>       then
//   polish: <CONVERGED|MAX_STEPS|STALLED|SKIPPED|FAILED> <steps> <factorisations> <indefinite> <F_initial> <F_final> <grad_initial> <grad_final>
// and with `ml_polish` through DPGOHashGroup::newton_polish and, from its point, DPGOHashGroup::ml_polish (trivial loss; pose 0 is
// the anchor; the file's information matrices): the lines of `polish` with the prefix "ml polish:", the F fields F_ml
// then through DPGOHashGroup::ml_marginal_covariances at the refined point the lines of `covariance` with the prefix "ml covariance:"
// and with `robust_polish` (a robust loss) through DPGOHashGroup::robust_newton_polish on a second, trivial-loss group of the same
// graph (max_iterations = 0: nothing is factored for the optimiser), with the loss and loss_reg of the run; the lines of `polish`
// with the prefix "robust polish:", the F fields those of the robust objective
// and with `gnc` (any loss of the run) through DPGOHashGroup::graduated_non_convexity (GNC-TLS, barc2 = 4, the inter-node edges
// as the robust set) on a second, trivial-loss group of the same graph, one line per edge and one per row of the new point:
//   gnc: w <edge> <weight, 17 digits>        gnc: x <row> <the d entries, 17 digits>       then
//   gnc: <CONVERGED|ALL_INLIERS|MAX_LEVELS|INNER_FAILED|SKIPPED|FAILED> <levels> <steps> <factorisations> <num_zero> <num_outliers> <F_initial> <F_weighted_final> <F_surrogate_final>
// and with `ml_gnc <tls|gm> <barc2>` (any loss of the run) through DPGOHashGroup::ml_graduated_non_convexity -- the same levels on
// chi2_e = r_e' Omega_e r_e with the file's information matrices, barc2 a chi2 quantile -- on a second, trivial-loss group:
//   ml gnc: w <edge> <weight, 17 digits>        ml gnc: x <row> <the d entries, 17 digits>       then
//   ml gnc: <outcome as gnc> <levels> <steps> <factorisations> <num_zero> <num_outliers> <F_initial> <F_weighted_final> <F_surrogate_final> <near_pi> <near_pi_all>
// and with `staircase` through DPGOHashGroup::riemannian_staircase (trivial loss), one line per row of the result:
//   staircase: x <row> <the d entries, 17 digits>       then
//   staircase: <SOLVED|MAX_RANK|SADDLE|SKIPPED|FAILED> <final_rank> <F_initial> <F_sdp> <F_final> <gap>
// and with `pairs <candidates.g2o>` through DPGOHashGroup::pair_covariances (trivial loss; pose 0 is the anchor): the file's
// edges p -> q are the pairs and their measurements the candidates; per candidate three lines, all entries with 17 digits,
//   pairs: joint <k> <the 3 dof^2 entries>     pairs: rel <k> <the dof^2 entries>     pairs: gate <k> <d2 not_pd residual>
// then   pairs: <OK|NOT_PD|SKIPPED|FAILED> <columns> <batches> <stationarity>; a last call with candidates of the wrong length
// must fail:   pairs: short candidates <status>
// and with `marginal <poses.txt> [base]` through DPGOHashGroup::newton_polish and DPGOHashGroup::joint_marginal (trivial loss;
// pose 0 is the anchor): the file lists one pose id per line, the kept set in that order; with a base (a member of the set) the
// relative form.  Per row of the n x n matrices one line each, all entries with 17 digits,
//   marginal: cov <row> <the n entries>      marginal: info <row> <the n entries>
// then   marginal: <OK|NOT_PD|SKIPPED|FAILED> <n> <columns> <batches> <info_not_pd> <logdet, 17 digits>; a last call with the
// first pose listed twice must fail:   marginal: repeated pose <status>
// and with `candidates <candidates.g2o> <budget>` through DPGOHashGroup::newton_polish and DPGOHashGroup::candidate_set (trivial
// loss; pose 0 is the anchor): the file holds candidate edges between poses of the graph.  Per row of the n x n matrices one
// line each, all entries with 17 digits,
//   candidates: S <row> <the n entries>      candidates: info <row> <the n entries>
// per chosen candidate   candidates: step <k> <index> <gain> <d2> <eligible>
// then   candidates: <OK|NOT_PD|SKIPPED|FAILED> <n> <poses> <selected> <logdet> <d2_joint> <gain_all> <gain_selected> <d2_selected>;
// a last call with the first candidate joining a pose to itself must fail:   candidates: self pair <status>
// and with `modes <k>` through DPGOHashGroup::newton_polish and DPGOHashGroup::hessian_modes (trivial loss; pose 0 is the anchor):
// per eigenpair one line, all entries with 17 digits,
//   modes: v <j> <lambda_j> <residual_j> <the dof N entries of v_j by global pose>
// then   modes: <CONVERGED|MAX_ITERS|STALLED|SKIPPED|FAILED> <iterations> <factorisations> <shift_tries> <block> <negative> <mu> <hmax>;
// a last call with k = 61 must fail:   modes: k = 61 <status>
// and with `sensitivity <pose>` through DPGOHashGroup::newton_polish and DPGOHashGroup::measurement_sensitivities (trivial
// loss; pose 0 is the anchor) with the dof unit columns of the pose: per edge one line, all entries with 17 digits,
//   sensitivity: e <edge> <the dof x (2 + dof) entries, row a the derivatives of coordinate a of the pose>
// then   sensitivity: <OK|NOT_PD|SKIPPED|FAILED> <edges> <columns> <batches>; a last call with an upstream of the wrong length
// must fail:   sensitivity: short upstream <status> <size of sens>
// and with `robust_sensitivity <pose>` (a robust loss) through DPGOHashGroup::robust_newton_polish and
// DPGOHashGroup::robust_measurement_sensitivities on a second, trivial-loss group of the same graph, with the loss and loss_reg
// of the run and the dof unit columns of the pose: per edge one line, all entries with 17 digits,
//   robust sensitivity: e <edge> <the dof x (3 + dof) entries, the last of a row the edge's term of d/dloss_reg>
// then   robust sensitivity: delta <the dof values of d x_pose / d loss_reg>
// then   robust sensitivity: <OK|NOT_PD|SKIPPED|FAILED> <edges> <columns> <batches>
// and with `reliability` through DPGOHashGroup::newton_polish and DPGOHashGroup::edge_reliability (trivial loss; pose 0 is the
// anchor; every edge): per edge one line, all entries with 17 digits,
//   reliability: e <edge> <the 6 + 2 dof entries of its record>
// then   reliability: <OK|NOT_PD|SKIPPED|FAILED> <SELINV|SOLVE|AUTO> <edges> <flagged> <unweighted> <redundancy_sum, 17 digits>; a
// last call with an edge index outside the graph must fail:   reliability: bad edge <status>
// and with `ml_reliability` through DPGOHashGroup::newton_polish, ::ml_polish and, at its point, ::ml_edge_reliability (every edge,
// on the file's information matrices) and ::ml_pair_gate with every edge of the graph as its own candidate: per edge two lines,
// all entries with 17 digits,
//   ml reliability: e <edge> <the 6 + 2 dof entries of its record>
//   ml gate: e <edge> <d2> <not_pd> <the dof entries of the residual>
// then   ml reliability: <OK|NOT_PD|SKIPPED|FAILED> <SELINV|SOLVE|AUTO> <edges> <flagged> <redundancy_sum, 17 digits>
// and    ml gate: <OK|NOT_PD|SKIPPED|FAILED> <columns> <batches>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "dpgo_amd.hpp"

int main(int argc, char **argv) {
  if (argc >= 4 && !strcmp(argv[1], "--info")) {
    auto g = DPGO::Graph::read_g2o(argv[2], atoi(argv[3]));
    printf("d %d poses %d edges %d nodes %d\n", g->d(), g->num_poses(), g->num_edges(), g->num_nodes());
    for (int a = 0; a < g->num_nodes(); a++) {
      int n[2], m[2];
      g->sizes(a, n, m);
      printf("node %d: n %d %d m %d %d offset %d\n", a, n[0], n[1], m[0], m[1], g->offset(a));
    }
    return 0;
  }
  if (argc < 4) {
    fprintf(stderr, "usage: %s <file.g2o> <num_nodes> <iters> [loss] [accelerated] [certify|verify|reweighted|covariance|polish|ml_polish|robust_polish|gnc|ml_gnc <tls|gm> <barc2>|staircase|pairs <candidates.g2o>|modes <k>|sensitivity <pose>|robust_sensitivity <pose>|reliability|ml_reliability]\n", argv[0]);
    return 2;
  }
  const int num_nodes = atoi(argv[2]), iters = atoi(argv[3]);
  const std::string loss = argc > 4 ? argv[4] : "trivial";
  const bool acc = argc > 5 ? atoi(argv[5]) != 0 : true;
  const DPGO::Loss l = loss == "huber" ? DPGO::Loss::Huber : loss == "gm" ? DPGO::Loss::GemanMcClure
                       : loss == "welsch" ? DPGO::Loss::Welsch : DPGO::Loss::None;
  auto graph = DPGO::Graph::read_g2o(argv[1], num_nodes);
  std::vector<int> all(num_nodes);
  for (int a = 0; a < num_nodes; a++) all[a] = a;
  DPGO::DPGOHashGroup dpgo_hash(graph, all, DPGO::Options::driver(l, acc), 0);
  if (dpgo_hash.initialize(graph->chordal_initialization()) != 0 || dpgo_hash.update() != 0) return 1;
  auto report = [&](int it) {
    double F = 0, g2 = 0;
    for (int a = 0; a < num_nodes; a++) {
      const DPGO::DPGOResult r = dpgo_hash[a].results(false);
      F += r.fobj;
      g2 += r.gradFnorm * r.gradFnorm;
    }
    printf("%d: %.10e %.10e\n", it, 2 * F, 2 * std::sqrt(g2));
  };
  report(0);
  for (int it = 1; it <= iters; it++) {
    if (dpgo_hash.iterate() != 0 || dpgo_hash.communicate() != 0 || dpgo_hash.update() != 0) return 1;
    report(it);
  }
  if (argc > 6 && !strcmp(argv[6], "certify")) {
    DPGO::Matrix X((graph->d() + 1) * graph->num_poses(), graph->d()), x;
    if (dpgo_hash.gather(X) != 0) return 1;
    double theta = 0;
    int its = 0, status = -1;
    dpgo_cert_result_t r = {};
    dpgo_hash.verify_solution(X, 1e-3, theta, x, its, &status, &r);
    const char *name = status == DPGO_CERT_NEGATIVE ? "NEGATIVE" : status == DPGO_CERT_NONNEGATIVE ? "NONNEGATIVE"
                       : status == DPGO_CERT_UNDECIDED ? "UNDECIDED" : "FAILED";
    fprintf(stderr, "certificate: %s %.10e %.10e %d %.10e\n", name, theta, r.residual, its, r.stationarity);
    if (status < 0) return 1;
  }
  if (argc > 6 && !strcmp(argv[6], "verify")) {
    DPGO::Matrix X((graph->d() + 1) * graph->num_poses(), graph->d()), x;
    if (dpgo_hash.gather(X) != 0) return 1;
    double theta = 0;
    int its = 0, status = -1;
    dpgo_cert_result_t r = {};
    dpgo_cert_factor_t f = {};
    dpgo_hash.fast_verification(X, 1e-3, theta, x, its, &status, &r, &f);
    const char *name = status == DPGO_CERT_PROVEN ? "PROVEN" : status == DPGO_CERT_NEGATIVE ? "NEGATIVE"
                       : status == DPGO_CERT_NONNEGATIVE ? "NONNEGATIVE" : status == DPGO_CERT_UNDECIDED ? "UNDECIDED" : "FAILED";
    const char *oc = f.outcome == DPGO_CERT_FACTOR_PD ? "PD" : f.outcome == DPGO_CERT_FACTOR_NOT_PD ? "NOT_PD" : "SKIPPED";
    fprintf(stderr, "verification: %s %s %.10e %.10e %.10e %d %.10e\n", name, oc, f.pivot_min, theta, r.residual, its, r.stationarity);
    if (status < 0) return 1;
  }
  if (argc > 6 && !strcmp(argv[6], "reweighted")) {
    DPGO::Matrix X((graph->d() + 1) * graph->num_poses(), graph->d()), x;
    if (dpgo_hash.gather(X) != 0) return 1;
    const double loss_reg = DPGO::Options::driver(l, acc).loss_reg;
    DPGO::EdgeEvaluation edges(*graph, 0);
    if (edges.run(X, l, loss_reg) != 0) return 1;
    auto scaled = graph->scale_edges(edges.weight());
    double theta = 0, stat = 0;
    int its = 0, status = -1;
    dpgo_cert_factor_t f = {};
    dpgo_edge_summary_t es = {};
    DPGO::fast_verification_reweighted(*graph, X, l, loss_reg, 1e-3, theta, x, its, &status, &f, &es, &stat);
    const char *name = status == DPGO_CERT_PROVEN ? "PROVEN" : status == DPGO_CERT_NEGATIVE ? "NEGATIVE"
                       : status == DPGO_CERT_NONNEGATIVE ? "NONNEGATIVE" : status == DPGO_CERT_UNDECIDED ? "UNDECIDED" : "FAILED";
    const char *oc = f.outcome == DPGO_CERT_FACTOR_PD ? "PD" : f.outcome == DPGO_CERT_FACTOR_NOT_PD ? "NOT_PD" : "SKIPPED";
    fprintf(stderr, "reweighted verification: %s %s %.10e %.10e %d %.10e %d/%d %.10e %d\n", name, oc, f.pivot_min, theta, its, stat,
            es.num_downweighted, es.num_inter, es.weight_min, scaled->num_edges());
    if (status < 0 || es.num_downweighted != edges.summary().num_downweighted) return 1;
  }
  if (argc > 6 && !strcmp(argv[6], "covariance")) {
    DPGO::Matrix X((graph->d() + 1) * graph->num_poses(), graph->d());
    if (dpgo_hash.gather(X) != 0) return 1;
    const int d = graph->d(), dof = d + d * (d - 1) / 2;
    std::vector<double> marg;
    int status = -1;
    dpgo_cov_result_t r = {};
    const bool ok = dpgo_hash.marginal_covariances(X, marg, 0, &r, &status);
    for (int p = 0; ok && p < graph->num_poses(); p++) {
      fprintf(stderr, "covariance: %d", p);
      for (int a = 0; a < dof; a++)
        for (int b = a; b < dof; b++) fprintf(stderr, " %.17g", marg[((size_t)p * dof + a) * dof + b]);
      fprintf(stderr, "\n");
    }
    fprintf(stderr, "covariance: %s %d %d %.10e\n", status == DPGO_COV_OK ? "OK" : status == DPGO_COV_NOT_PD ? "NOT_PD"
            : status == DPGO_COV_SKIPPED ? "SKIPPED" : "FAILED", r.fronts, r.levels, r.stationarity);
    if (status < 0) return 1;
  }
  if (argc > 6 && !strcmp(argv[6], "polish")) {
    DPGO::Matrix X((graph->d() + 1) * graph->num_poses(), graph->d()), Z;
    if (dpgo_hash.gather(X) != 0) return 1;
    int status = -1;
    dpgo_polish_result_t r = {};
    dpgo_hash.newton_polish(X, Z, &r, &status);
    for (int i = 0; status >= 0 && status != DPGO_POLISH_SKIPPED && i < Z.rows(); i++) {
      fprintf(stderr, "polish: x %d", i);
      for (int c = 0; c < Z.cols(); c++) fprintf(stderr, " %.17g", Z.data()[(size_t)c * Z.rows() + i]);
      fprintf(stderr, "\n");
    }
    fprintf(stderr, "polish: %s %d %d %d %.17g %.17g %.17g %.17g\n",
            status == DPGO_POLISH_CONVERGED ? "CONVERGED" : status == DPGO_POLISH_MAX_STEPS ? "MAX_STEPS"
            : status == DPGO_POLISH_STALLED ? "STALLED" : status == DPGO_POLISH_SKIPPED ? "SKIPPED" : "FAILED",
            r.steps, r.factorisations, r.indefinite, r.F_initial, r.F_final, r.grad_initial, r.grad_final);
    if (status < 0) return 1;
  }
  if (argc > 6 && !strcmp(argv[6], "ml_polish")) {
    DPGO::Matrix X((graph->d() + 1) * graph->num_poses(), graph->d()), Xp, Z;
    if (dpgo_hash.gather(X) != 0) return 1;
    int status = -1;
    dpgo_ml_result_t r = {};
    dpgo_hash.newton_polish(X, Xp);   // (Xp is X itself where the polish is SKIPPED)
    dpgo_hash.ml_polish(Xp, Z, &r, &status);
    for (int i = 0; status >= 0 && status != DPGO_POLISH_SKIPPED && i < Z.rows(); i++) {
      fprintf(stderr, "ml polish: x %d", i);
      for (int c = 0; c < Z.cols(); c++) fprintf(stderr, " %.17g", Z.data()[(size_t)c * Z.rows() + i]);
      fprintf(stderr, "\n");
    }
    fprintf(stderr, "ml polish: %s %d %d %d %.17g %.17g %.17g %.17g\n",
            status == DPGO_POLISH_CONVERGED ? "CONVERGED" : status == DPGO_POLISH_MAX_STEPS ? "MAX_STEPS"
            : status == DPGO_POLISH_STALLED ? "STALLED" : status == DPGO_POLISH_SKIPPED ? "SKIPPED" : "FAILED",
            r.polish.steps, r.polish.factorisations, r.polish.indefinite, r.polish.F_initial, r.polish.F_final, r.polish.grad_initial,
            r.polish.grad_final);
    if (status < 0) return 1;
    const int d = graph->d(), dof = d + d * (d - 1) / 2;
    std::vector<double> marg;
    int cstatus = -1;
    dpgo_cov_result_t cr = {};
    const bool ok = dpgo_hash.ml_marginal_covariances(Z, marg, 0, &cr, &cstatus);
    for (int p = 0; ok && p < graph->num_poses(); p++) {
      fprintf(stderr, "ml covariance: %d", p);
      for (int a = 0; a < dof; a++)
        for (int b = a; b < dof; b++) fprintf(stderr, " %.17g", marg[((size_t)p * dof + a) * dof + b]);
      fprintf(stderr, "\n");
    }
    fprintf(stderr, "ml covariance: %s %d %d %.10e\n", cstatus == DPGO_COV_OK ? "OK" : cstatus == DPGO_COV_NOT_PD ? "NOT_PD"
            : cstatus == DPGO_COV_SKIPPED ? "SKIPPED" : "FAILED", cr.fronts, cr.levels, cr.stationarity);
    if (cstatus < 0) return 1;
  }
  if (argc > 6 && !strcmp(argv[6], "robust_polish")) {
    DPGO::Matrix X((graph->d() + 1) * graph->num_poses(), graph->d()), Z;
    if (dpgo_hash.gather(X) != 0) return 1;
    DPGO::Options trivial = DPGO::Options::driver(DPGO::Loss::None, acc);
    trivial.max_iterations = 0;
    DPGO::DPGOHashGroup post(graph, all, trivial, 0);
    int status = -1;
    dpgo_polish_result_t r = {};
    post.robust_newton_polish(X, l, DPGO::Options::driver(l, acc).loss_reg, Z, &r, &status);
    for (int i = 0; status >= 0 && status != DPGO_POLISH_SKIPPED && i < Z.rows(); i++) {
      fprintf(stderr, "robust polish: x %d", i);
      for (int c = 0; c < Z.cols(); c++) fprintf(stderr, " %.17g", Z.data()[(size_t)c * Z.rows() + i]);
      fprintf(stderr, "\n");
    }
    fprintf(stderr, "robust polish: %s %d %d %d %.17g %.17g %.17g %.17g\n",
            status == DPGO_POLISH_CONVERGED ? "CONVERGED" : status == DPGO_POLISH_MAX_STEPS ? "MAX_STEPS"
            : status == DPGO_POLISH_STALLED ? "STALLED" : status == DPGO_POLISH_SKIPPED ? "SKIPPED" : "FAILED",
            r.steps, r.factorisations, r.indefinite, r.F_initial, r.F_final, r.grad_initial, r.grad_final);
    if (status < 0) return 1;
  }
  if (argc > 6 && !strcmp(argv[6], "gnc")) {
    DPGO::Matrix X((graph->d() + 1) * graph->num_poses(), graph->d()), Z;
    if (dpgo_hash.gather(X) != 0) return 1;
    DPGO::Options trivial = DPGO::Options::driver(DPGO::Loss::None, acc);
    trivial.max_iterations = 0;
    DPGO::DPGOHashGroup post(graph, all, trivial, 0);
    int status = -1;
    dpgo_gnc_result_t r = {};
    dpgo_gnc_options_t o;
    dpgo_gnc_options_default(&o);
    o.barc2 = 4.0;
    std::vector<double> w;
    post.graduated_non_convexity(X, Z, w, &r, &status, &o);
    for (size_t e = 0; status >= 0 && status != DPGO_GNC_SKIPPED && e < w.size(); e++) fprintf(stderr, "gnc: w %zu %.17g\n", e, w[e]);
    for (int i = 0; status >= 0 && status != DPGO_GNC_SKIPPED && i < Z.rows(); i++) {
      fprintf(stderr, "gnc: x %d", i);
      for (int c = 0; c < Z.cols(); c++) fprintf(stderr, " %.17g", Z.data()[(size_t)c * Z.rows() + i]);
      fprintf(stderr, "\n");
    }
    fprintf(stderr, "gnc: %s %d %d %d %d %d %.17g %.17g %.17g\n",
            status == DPGO_GNC_CONVERGED ? "CONVERGED" : status == DPGO_GNC_ALL_INLIERS ? "ALL_INLIERS"
            : status == DPGO_GNC_MAX_LEVELS ? "MAX_LEVELS" : status == DPGO_GNC_INNER_FAILED ? "INNER_FAILED"
            : status == DPGO_GNC_SKIPPED ? "SKIPPED" : "FAILED",
            r.levels, r.steps, r.factorisations, r.num_zero, r.num_outliers, r.F_initial, r.F_weighted_final, r.F_surrogate_final);
    if (status < 0) return 1;
  }
  if (argc > 8 && !strcmp(argv[6], "ml_gnc")) {
    DPGO::Matrix X((graph->d() + 1) * graph->num_poses(), graph->d()), Z;
    if (dpgo_hash.gather(X) != 0) return 1;
    DPGO::Options trivial = DPGO::Options::driver(DPGO::Loss::None, acc);
    trivial.max_iterations = 0;
    DPGO::DPGOHashGroup post(graph, all, trivial, 0);
    int status = -1;
    dpgo_ml_gnc_result_t r = {};
    dpgo_gnc_options_t o;
    dpgo_gnc_options_default(&o);
    o.kind = !strcmp(argv[7], "gm") ? DPGO_GNC_GM : DPGO_GNC_TLS;
    o.barc2 = atof(argv[8]);
    std::vector<double> w;
    post.ml_graduated_non_convexity(X, Z, w, &r, &status, &o);
    for (size_t e = 0; status >= 0 && status != DPGO_GNC_SKIPPED && e < w.size(); e++) fprintf(stderr, "ml gnc: w %zu %.17g\n", e, w[e]);
    for (int i = 0; status >= 0 && status != DPGO_GNC_SKIPPED && i < Z.rows(); i++) {
      fprintf(stderr, "ml gnc: x %d", i);
      for (int c = 0; c < Z.cols(); c++) fprintf(stderr, " %.17g", Z.data()[(size_t)c * Z.rows() + i]);
      fprintf(stderr, "\n");
    }
    fprintf(stderr, "ml gnc: %s %d %d %d %d %d %.17g %.17g %.17g %lld %lld\n",
            status == DPGO_GNC_CONVERGED ? "CONVERGED" : status == DPGO_GNC_ALL_INLIERS ? "ALL_INLIERS"
            : status == DPGO_GNC_MAX_LEVELS ? "MAX_LEVELS" : status == DPGO_GNC_INNER_FAILED ? "INNER_FAILED"
            : status == DPGO_GNC_SKIPPED ? "SKIPPED" : "FAILED",
            r.gnc.levels, r.gnc.steps, r.gnc.factorisations, r.gnc.num_zero, r.gnc.num_outliers, r.gnc.F_initial, r.gnc.F_weighted_final,
            r.gnc.F_surrogate_final, r.near_pi, r.near_pi_all);
    if (status < 0) return 1;
  }
  if (argc > 6 && !strcmp(argv[6], "staircase")) {
    DPGO::Matrix X((graph->d() + 1) * graph->num_poses(), graph->d()), Z;
    if (dpgo_hash.gather(X) != 0) return 1;
    int status = -1;
    dpgo_staircase_result_t r = {};
    dpgo_hash.riemannian_staircase(X, Z, &r, &status);
    for (int i = 0; status >= 0 && status != DPGO_STAIR_SKIPPED && i < Z.rows(); i++) {
      fprintf(stderr, "staircase: x %d", i);
      for (int c = 0; c < Z.cols(); c++) fprintf(stderr, " %.17g", Z.data()[(size_t)c * Z.rows() + i]);
      fprintf(stderr, "\n");
    }
    fprintf(stderr, "staircase: %s %d %.17g %.17g %.17g %.17g\n",
            status == DPGO_STAIR_SOLVED ? "SOLVED" : status == DPGO_STAIR_MAX_RANK ? "MAX_RANK"
            : status == DPGO_STAIR_SADDLE ? "SADDLE" : status == DPGO_STAIR_SKIPPED ? "SKIPPED" : "FAILED",
            r.final_rank, r.F_initial, r.F_sdp, r.F_final, r.gap);
    if (status < 0) return 1;
  }
  if (argc > 7 && !strcmp(argv[6], "pairs")) {
    DPGO::Matrix X((graph->d() + 1) * graph->num_poses(), graph->d());
    if (dpgo_hash.gather(X) != 0) return 1;
    const int d = graph->d(), dof = d + d * (d - 1) / 2, nc = d * d + d + 2;
    auto cg = DPGO::Graph::read_g2o(argv[7], 1);
    const int m = cg->num_edges();
    std::vector<int> I(m), J(m), pairs((size_t)2 * m);
    std::vector<double> R((size_t)m * d * d), t((size_t)m * d), kappa(m), tau(m), cand((size_t)m * nc);
    if (cg->d() != d || dpgo_graph_edges(cg->handle(), I.data(), J.data(), R.data(), t.data(), kappa.data(), tau.data()) != 0) return 1;
    for (int k = 0; k < m; k++) {
      pairs[2 * k] = I[k]; pairs[2 * k + 1] = J[k];
      for (int i = 0; i < d * d; i++) cand[(size_t)k * nc + i] = R[(size_t)k * d * d + i];
      for (int i = 0; i < d; i++) cand[(size_t)k * nc + d * d + i] = t[(size_t)k * d + i];
      cand[(size_t)k * nc + d * d + d] = kappa[k];
      cand[(size_t)k * nc + d * d + d + 1] = tau[k];
    }
    std::vector<double> joint, rel, gate;
    int status = -1;
    dpgo_pairs_result_t r = {};
    const bool ok = dpgo_hash.pair_covariances(X, pairs, joint, rel, 0, &r, &status, &cand, &gate);
    auto line = [&](const char *what, int k, const std::vector<double> &v, int n) {
      fprintf(stderr, "pairs: %s %d", what, k);
      for (int i = 0; i < n; i++) fprintf(stderr, " %.17g", v[(size_t)k * n + i]);
      fprintf(stderr, "\n");
    };
    for (int k = 0; ok && k < m; k++) {
      line("joint", k, joint, 3 * dof * dof);
      line("rel", k, rel, dof * dof);
      line("gate", k, gate, 2 + dof);
    }
    fprintf(stderr, "pairs: %s %d %d %.10e\n", status == DPGO_PAIRS_OK ? "OK" : status == DPGO_PAIRS_NOT_PD ? "NOT_PD"
            : status == DPGO_PAIRS_SKIPPED ? "SKIPPED" : "FAILED", r.columns, r.batches, r.stationarity);
    if (status < 0) return 1;
    cand.pop_back();
    int short_status = 0;
    dpgo_hash.pair_covariances(X, pairs, joint, rel, 0, nullptr, &short_status, &cand, &gate);
    fprintf(stderr, "pairs: short candidates %d %d\n", short_status, (int)gate.size());
  }
  if (argc > 7 && !strcmp(argv[6], "marginal")) {
    DPGO::Matrix X((graph->d() + 1) * graph->num_poses(), graph->d()), Xp;
    if (dpgo_hash.gather(X) != 0 || !dpgo_hash.newton_polish(X, Xp)) return 1;
    std::vector<int> keep;
    FILE *in = fopen(argv[7], "r");
    if (!in) return 1;
    for (int p; fscanf(in, "%d", &p) == 1;) keep.push_back(p);
    fclose(in);
    const int base = argc > 8 ? atoi(argv[8]) : -1;
    std::vector<double> cov, info;
    double logdet = 0.0;
    int status = -1;
    dpgo_marg_result_t r = {};
    const bool ok = dpgo_hash.joint_marginal(Xp, keep, cov, &info, &logdet, 0, base, &r, &status);
    for (int w = 0; ok && w < 2; w++)
      for (int i = 0; i < r.n; i++) {
        fprintf(stderr, "marginal: %s %d", w ? "info" : "cov", i);
        for (int j = 0; j < r.n; j++) fprintf(stderr, " %.17g", (w ? info : cov)[(size_t)i * r.n + j]);
        fprintf(stderr, "\n");
      }
    fprintf(stderr, "marginal: %s %d %d %d %d %.17g\n", status == DPGO_MARG_OK ? "OK" : status == DPGO_MARG_NOT_PD ? "NOT_PD"
            : status == DPGO_MARG_SKIPPED ? "SKIPPED" : "FAILED", r.n, r.columns, r.batches, r.info_not_pd, logdet);
    if (status < 0) return 1;
    keep.push_back(keep[0]);
    int twice_status = 0;
    dpgo_hash.joint_marginal(Xp, keep, cov, &info, &logdet, 0, base, nullptr, &twice_status);
    fprintf(stderr, "marginal: repeated pose %d\n", twice_status);
  }
  if (argc > 8 && !strcmp(argv[6], "candidates")) {
    DPGO::Matrix X((graph->d() + 1) * graph->num_poses(), graph->d()), Xp;
    if (dpgo_hash.gather(X) != 0 || !dpgo_hash.newton_polish(X, Xp)) return 1;
    const int d = graph->d(), nc = d * d + d + 2;
    auto cg = DPGO::Graph::read_g2o(argv[7], 1);
    const int m = cg->num_edges();
    std::vector<int> I(m), J(m), pairs((size_t)2 * m);
    std::vector<double> R((size_t)m * d * d), t((size_t)m * d), kappa(m), tau(m), cand((size_t)m * nc);
    if (cg->d() != d || m < 1 || dpgo_graph_edges(cg->handle(), I.data(), J.data(), R.data(), t.data(), kappa.data(), tau.data()) != 0) return 1;
    for (int k = 0; k < m; k++) {
      pairs[2 * k] = I[k]; pairs[2 * k + 1] = J[k];
      std::copy(&R[(size_t)k * d * d], &R[(size_t)(k + 1) * d * d], &cand[(size_t)k * nc]);
      std::copy(&t[(size_t)k * d], &t[(size_t)(k + 1) * d], &cand[(size_t)k * nc + d * d]);
      cand[(size_t)k * nc + d * d + d] = kappa[k];
      cand[(size_t)k * nc + d * d + d + 1] = tau[k];
    }
    std::vector<double> S, res, info, steps;
    std::vector<int> selected;
    double sc[5];
    int status = -1;
    dpgo_cand_result_t r = {};
    const bool ok = dpgo_hash.candidate_set(Xp, pairs, cand, atoi(argv[8]), S, res, selected, steps, sc, &info, 0.0, 0, &r, &status);
    for (int w = 0; ok && w < 2; w++)
      for (int i = 0; i < r.n; i++) {
        fprintf(stderr, "candidates: %s %d", w ? "info" : "S", i);
        for (int j = 0; j < r.n; j++) fprintf(stderr, " %.17g", (w ? info : S)[(size_t)i * r.n + j]);
        fprintf(stderr, "\n");
      }
    for (size_t k = 0; ok && k < selected.size(); k++)
      fprintf(stderr, "candidates: step %d %d %.17g %.17g %d\n", (int)k, selected[k], steps[4 * k + 1], steps[4 * k + 2], (int)steps[4 * k + 3]);
    fprintf(stderr, "candidates: %s %d %d %d %.17g %.17g %.17g %.17g %.17g\n", status == DPGO_CAND_OK ? "OK" : status == DPGO_CAND_NOT_PD ? "NOT_PD"
            : status == DPGO_CAND_SKIPPED ? "SKIPPED" : "FAILED", r.n, r.poses, r.n_selected, sc[0], sc[1], sc[2], sc[3], sc[4]);
    if (status < 0) return 1;
    pairs[1] = pairs[0];
    int self_status = 0;
    dpgo_hash.candidate_set(Xp, pairs, cand, 1, S, res, selected, steps, sc, &info, 0.0, 0, nullptr, &self_status);
    fprintf(stderr, "candidates: self pair %d\n", self_status);
  }
  if (argc > 7 && !strcmp(argv[6], "modes")) {
    DPGO::Matrix X((graph->d() + 1) * graph->num_poses(), graph->d()), Xp;
    if (dpgo_hash.gather(X) != 0 || !dpgo_hash.newton_polish(X, Xp)) return 1;
    const int d = graph->d(), dof = d + d * (d - 1) / 2, N = graph->num_poses(), k = atoi(argv[7]);
    std::vector<double> values, vectors, residuals, energy;
    int status = -1;
    dpgo_modes_result_t r = {};
    const bool ok = dpgo_hash.hessian_modes(Xp, k, values, vectors, &residuals, &energy, nullptr, 0, &r, &status);
    for (int j = 0; ok && j < k; j++) {
      fprintf(stderr, "modes: v %d %.17g %.17g", j, values[j], residuals[j]);
      for (int i = 0; i < dof * N; i++) fprintf(stderr, " %.17g", vectors[(size_t)j * dof * N + i]);
      fprintf(stderr, "\n");
    }
    fprintf(stderr, "modes: %s %d %d %d %d %d %.17g %.17g\n", status == DPGO_MODES_CONVERGED ? "CONVERGED" : status == DPGO_MODES_MAX_ITERS ? "MAX_ITERS"
            : status == DPGO_MODES_STALLED ? "STALLED" : status == DPGO_MODES_SKIPPED ? "SKIPPED" : "FAILED", r.iterations, r.factorisations,
            r.shift_tries, r.block, r.negative, r.mu, r.hmax);
    if (status < 0) return 1;
    int wide_status = 0;
    dpgo_hash.hessian_modes(Xp, 61, values, vectors, nullptr, nullptr, nullptr, 0, nullptr, &wide_status);
    fprintf(stderr, "modes: k = 61 %d\n", wide_status);
  }
  if (argc > 7 && !strcmp(argv[6], "sensitivity")) {
    DPGO::Matrix X((graph->d() + 1) * graph->num_poses(), graph->d()), Xp;
    if (dpgo_hash.gather(X) != 0) return 1;
    const int d = graph->d(), dof = d + d * (d - 1) / 2, no = 2 + dof, m = graph->num_edges(), pose = atoi(argv[7]);
    if (pose < 0 || pose >= graph->num_poses() || !dpgo_hash.newton_polish(X, Xp)) return 1;
    const size_t n = (size_t)dof * graph->num_poses();
    std::vector<double> up(n * dof, 0.0), sens;
    for (int a = 0; a < dof; a++) up[(size_t)a * n + (size_t)dof * pose + a] = 1.0;
    int status = -1;
    dpgo_sens_result_t r = {};
    const bool ok = dpgo_hash.measurement_sensitivities(Xp, up, sens, 0, &r, &status);
    for (int e = 0; ok && e < m; e++) {
      fprintf(stderr, "sensitivity: e %d", e);
      for (int a = 0; a < dof; a++)
        for (int b = 0; b < no; b++) fprintf(stderr, " %.17g", sens[((size_t)a * m + e) * no + b]);
      fprintf(stderr, "\n");
    }
    fprintf(stderr, "sensitivity: %s %d %d %d\n", status == DPGO_SENS_OK ? "OK" : status == DPGO_SENS_NOT_PD ? "NOT_PD"
            : status == DPGO_SENS_SKIPPED ? "SKIPPED" : "FAILED", r.edges, r.columns, r.batches);
    if (status < 0) return 1;
    up.pop_back();
    int short_status = 0;
    dpgo_hash.measurement_sensitivities(Xp, up, sens, 0, nullptr, &short_status);
    fprintf(stderr, "sensitivity: short upstream %d %d\n", short_status, (int)sens.size());
  }
  if (argc > 6 && !strcmp(argv[6], "reliability")) {
    DPGO::Matrix X((graph->d() + 1) * graph->num_poses(), graph->d()), Xp;
    if (dpgo_hash.gather(X) != 0 || !dpgo_hash.newton_polish(X, Xp)) return 1;
    const int d = graph->d(), w = 6 + 2 * (d + d * (d - 1) / 2), m = graph->num_edges();
    std::vector<double> rec;
    int status = -1;
    dpgo_rely_result_t r = {};
    const bool ok = dpgo_hash.edge_reliability(Xp, rec, 0, &r, &status);
    for (int e = 0; ok && e < m; e++) {
      fprintf(stderr, "reliability: e %d", e);
      for (int b = 0; b < w; b++) fprintf(stderr, " %.17g", rec[(size_t)e * w + b]);
      fprintf(stderr, "\n");
    }
    fprintf(stderr, "reliability: %s %s %d %d %d %.17g\n", status == DPGO_RELY_OK ? "OK" : status == DPGO_RELY_NOT_PD ? "NOT_PD"
            : status == DPGO_RELY_SKIPPED ? "SKIPPED" : "FAILED", r.method_used == DPGO_RELY_SELINV ? "SELINV"
            : r.method_used == DPGO_RELY_SOLVE ? "SOLVE" : "AUTO", r.edges, r.flagged, r.unweighted, r.redundancy_sum);
    if (status < 0) return 1;
    const std::vector<int> bad = {0, m};
    int bad_status = 0;
    dpgo_hash.edge_reliability(Xp, rec, 0, nullptr, &bad_status, &bad);
    fprintf(stderr, "reliability: bad edge %d\n", bad_status);
  }
  if (argc > 6 && !strcmp(argv[6], "ml_reliability")) {
    DPGO::Matrix X((graph->d() + 1) * graph->num_poses(), graph->d()), Xp, Z;
    if (dpgo_hash.gather(X) != 0) return 1;
    dpgo_hash.newton_polish(X, Xp);   // (Xp is X itself where the polish is SKIPPED)
    int pstatus = -1;
    dpgo_hash.ml_polish(Xp, Z, nullptr, &pstatus);
    if (pstatus < 0) return 1;
    const int d = graph->d(), dof = d + d * (d - 1) / 2, w = 6 + 2 * dof, m = graph->num_edges();
    std::vector<double> rec;
    int status = -1;
    dpgo_rely_result_t r = {};
    const bool ok = dpgo_hash.ml_edge_reliability(Z, rec, 0, &r, &status);
    for (int e = 0; ok && e < m; e++) {
      fprintf(stderr, "ml reliability: e %d", e);
      for (int b = 0; b < w; b++) fprintf(stderr, " %.17g", rec[(size_t)e * w + b]);
      fprintf(stderr, "\n");
    }
    fprintf(stderr, "ml reliability: %s %s %d %d %.17g\n", status == DPGO_RELY_OK ? "OK" : status == DPGO_RELY_NOT_PD ? "NOT_PD"
            : status == DPGO_RELY_SKIPPED ? "SKIPPED" : "FAILED", r.method_used == DPGO_RELY_SELINV ? "SELINV"
            : r.method_used == DPGO_RELY_SOLVE ? "SOLVE" : "AUTO", r.edges, r.flagged, r.redundancy_sum);
    if (status < 0) return 1;
    // every edge of the graph as a candidate of its own
    std::vector<int> I(m), J(m), pairs((size_t)2 * m);
    std::vector<double> cR((size_t)m * d * d), ct((size_t)m * d), kappa(m), tau(m), info((size_t)m * dof * dof), gate, joint, rel;
    if (dpgo_graph_edges(graph->handle(), I.data(), J.data(), cR.data(), ct.data(), kappa.data(), tau.data()) != 0) return 1;
    if (dpgo_graph_edge_information(graph->handle(), info.data(), nullptr) != 0) return 1;
    for (int e = 0; e < m; e++) {
      pairs[(size_t)2 * e] = I[e];
      pairs[(size_t)2 * e + 1] = J[e];
    }
    int gstatus = -1;
    dpgo_pairs_result_t gr = {};
    const bool gok = dpgo_hash.ml_pair_gate(Z, pairs, cR, ct, info, gate, joint, rel, 0, &gr, &gstatus);
    for (int e = 0; gok && e < m; e++) {
      fprintf(stderr, "ml gate: e %d", e);
      for (int b = 0; b < 2 + dof; b++) fprintf(stderr, " %.17g", gate[(size_t)e * (2 + dof) + b]);
      fprintf(stderr, "\n");
    }
    fprintf(stderr, "ml gate: %s %d %d\n", gstatus == DPGO_PAIRS_OK ? "OK" : gstatus == DPGO_PAIRS_NOT_PD ? "NOT_PD"
            : gstatus == DPGO_PAIRS_SKIPPED ? "SKIPPED" : "FAILED", gr.columns, gr.batches);
    if (gstatus < 0) return 1;
  }
  if (argc > 7 && !strcmp(argv[6], "robust_sensitivity")) {
    DPGO::Matrix X((graph->d() + 1) * graph->num_poses(), graph->d()), Xp;
    if (dpgo_hash.gather(X) != 0) return 1;
    DPGO::Options trivial = DPGO::Options::driver(DPGO::Loss::None, acc);
    trivial.max_iterations = 0;
    DPGO::DPGOHashGroup post(graph, all, trivial, 0);
    const double loss_reg = DPGO::Options::driver(l, acc).loss_reg;
    const int d = graph->d(), dof = d + d * (d - 1) / 2, no = 3 + dof, m = graph->num_edges(), pose = atoi(argv[7]);
    int polished = -1;
    post.robust_newton_polish(X, l, loss_reg, Xp, nullptr, &polished);   // (Xp is X itself where the polish is SKIPPED)
    if (pose < 0 || pose >= graph->num_poses() || polished < 0) return 1;
    const size_t n = (size_t)dof * graph->num_poses();
    std::vector<double> up(n * dof, 0.0), sens, dreg;
    for (int a = 0; a < dof; a++) up[(size_t)a * n + (size_t)dof * pose + a] = 1.0;
    int status = -1;
    dpgo_sens_result_t r = {};
    const bool ok = post.robust_measurement_sensitivities(Xp, l, loss_reg, up, sens, dreg, 0, &r, &status);
    for (int e = 0; ok && e < m; e++) {
      fprintf(stderr, "robust sensitivity: e %d", e);
      for (int a = 0; a < dof; a++)
        for (int b = 0; b < no; b++) fprintf(stderr, " %.17g", sens[((size_t)a * m + e) * no + b]);
      fprintf(stderr, "\n");
    }
    if (ok) {
      fprintf(stderr, "robust sensitivity: delta");
      for (int a = 0; a < dof; a++) fprintf(stderr, " %.17g", dreg[a]);
      fprintf(stderr, "\n");
    }
    fprintf(stderr, "robust sensitivity: %s %d %d %d\n", status == DPGO_SENS_OK ? "OK" : status == DPGO_SENS_NOT_PD ? "NOT_PD"
            : status == DPGO_SENS_SKIPPED ? "SKIPPED" : "FAILED", r.edges, r.columns, r.batches);
    if (status < 0) return 1;
  }
  return 0;
}
