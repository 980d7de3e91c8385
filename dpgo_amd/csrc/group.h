// A group of DPGO nodes hosted on one MI355X.
//
// Host-side mirror of the reference's per-node optimizer
//   DPGOHash    C++/DPGO/src/DPGOHash.cpp (initialize :20-43, update :84-228,
//               amm_pgo :230-444, mm_pgo :446-581, iterate :583-628),
//               C++/DPGO/include/DPGO/DPGOHash.h:28-86 (communicate)
//   DPGOProblem C++/DPGO/src/DPGOProblem.cpp (operators), DPGOProblem.h:275-294
// with every vector operation batched over the nodes of the group and executed
// by the kernels of kernels.hip.  The scalar state machine (Nesterov sequence,
// adaptive-restart counters) stays on the host exactly as in the reference; a
// per-node device mask lets nodes that take different branches share launches.
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <functional>
#include <initializer_list>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <utility>
#include <string>
#include <vector>

#include "assemble.h"
#include "cert.h"
#include "cand.h"
#include "cov.h"
#include "graph.h"
#include "kernels.h"
#include "marg.h"
#include "ml.h"
#include "pairs.h"
#include "gnc.h"
#include "ml_gnc.h"
#include "modes.h"
#include "polish.h"
#include "rely.h"
#include "robust.h"
#include "rsens.h"
#include "schedule.h"
#include "sens.h"
#include "settings.h"
#include "spd_solve.h"
#include "stair.h"

namespace dpgo {

// DPGO::Options (C++/DPGO/include/DPGO/DPGO_types.h:78-201), plain data.
struct Options {
  int scheme = 1;  // 0 MM, 1 AMM
  double regularizer = 1e-10;
  double accepted_delta = 5e-4;
  double eta[2] = {5e-4, 2.5e-2};
  double psi = 1e-10;
  double phi = 1e-6;
  int max_soft_restart_hits[2] = {10, 25};
  int oscillation_cnt_period = 15;
  int max_oscillations = 12;
  int loss = 0;  // 0 None, 1 Huber, 2 GemanMcClure, 3 Welsch
  double loss_reg = 1.0;
  int rescale = 1;            // 0 Static, 1 Dynamic (DPGO_types.h:128)
  int max_rescale_count = 5;  // DPGO_types.h:131
  double grad_norm_tol = 5e-3;
  double rel_func_decrease_tol = 1e-6;
  double stepsize_tol = 1e-4;
  int max_iterations = 10;
  int max_iterations_accepted = 1;
  double reg_Cholesky_precon_max_condition_number = 1e6;
  double preconditioned_grad_norm_tol = 1e-4;
  int max_tCG_iterations = 10000;
  double STPCG_kappa = 0.05;
  double STPCG_theta = 0.9;
  int verbose = 0;         // DPGO_types.h:87: a summary line per node and TNT refinement on stdout
  int preconditioner = 3;  // Preconditioner (DPGO_types.h:35-40): 0 None, 1 Jacobi, 2 IncompleteCholesky, 3 RegularizedCholesky
};

// The scalar fields of DPGOResult (DPGO_types.h:204-322) the state machine uses.
struct NodeResults {
  int updated = 1;
  int iters = 0;
  bool pre_done = false, pre_repeat = false;   // host_update_pre ran for the update under way (and what `repeat` was)
  int hist_iter = -1;   // iteration whose X[iter-1], g[iter-1], fobj[iter-1], s[iter] are in place (update() may run twice per iteration)
  double gradFnorm = 0, fobjE = 0, Fk[2] = {0, 0}, Gk = 0, Gkh = 0;
  double Gk_alt = 0;   // run_tnt: the refined point's surrogate value under the caller's second linear term
  double fobj = 0, fobj_prev = 0, f = 0, gamma = 0, s0 = 1, s1 = 1;
  int soft_restart_hits[2] = {0, 0};
  int num_oscillations = 0;
  int refined = 0;
  int tnt_status = -1;
  int tnt_inner = 0;
  int restarts = 0;
  std::vector<int> oscillations;
};

// DChordal::Options (C++/DChordal/include/DChordal/DChordal_types.h:44-70) + the driver's stage schedule
// (C++/examples/dist_pgo.cpp:205,274,344,383) + the length of the stage-0 stand-in (dchordal.cpp)
struct DChordalOptions {
  int iters[4] = {100, 400, 150, 250};   // reduced R, R, reduced t, t
  int local_iters = 30;
  double reg_G = 1e-12;
};

// TNTParams as DPGOHash leaves them (TNT.h:81-97, 129): the acceptance test and trust-region update of run_tnt() (tnt.cpp) and
// the same test in the gate of a speculative update (speculate_update)
struct TntConst {
  static constexpr double eta1 = .05, eta2 = .9, alpha1 = .25, alpha2 = 2.5, Delta_tol = 1e-6, Delta0 = 1.0;
  static double sqrt_eps() { return std::sqrt(std::numeric_limits<double>::epsilon()); }
};

// DPGO_SETUP_TIMING=1: wall time of the set-up phases on stderr
struct SetupClock {
  const bool on = settings().setup_timing;
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  void lap(const char *what) {
    if (!on) return;
    const auto n = std::chrono::steady_clock::now();
    fprintf(stderr, "[setup] %-44s %8.3f s\n", what, std::chrono::duration<double>(n - t).count());
    t = n;
  }
};

class Group {
 public:
  Group(const Graph &g, const std::vector<int> &node_ids, const Options &opt, int device);
  ~Group();
  bool ok() const { return ok_; }
  // the group cannot go on (a collective on its stream timed out, a refactorisation failed): update() / iterate() return -1
  // from now on and the destructor does not wait for the stream
  void mark_failed() { failed_ = true; }
  int d() const { return d_; }
  int num_local() const { return (int)nodes_.size(); }
  const DataInfo &info(int local) const { return info_[local]; }
  const NodeResults &results(int local) { finish_update(); return res_[local]; }
  const Options &options() const { return opt_; }
  int node_id(int local) const { return nodes_[local]; }

  // X: (d+1)(n0+n1) x d column-major with leading dimension ld (DPGOHash::initialize)
  int initialize(int local, const double *X, int ld);
  // X: global (d+1)N x d column-major; fills own and neighbour rows of every local node
  // (dist_pgo.cpp:435-446) and initialises them.
  int initialize_global(const double *X, int ld);
  // DPGOStar::evaluate_f / evaluate_grad at an arbitrary global X (DPGOStar.cpp:713-829); state untouched
  int evaluate_global(const double *X, int ld, double *F, double *grad_sqnorm, double *grad, int ldg);
  int set_options(const Options &o);                     // DPGOHash::set_options (DPGOHash.h:93-96)
  int update(const std::vector<int> &locals);
  int iterate(const std::vector<int> &locals);
  int communicate_local();
  // the driver's loop body (C++/examples/dist_pgo.cpp:496-521) for the nodes in `locals`: iterate -> exchange (the caller's:
  // an RCCL exchange on the communicator's stream, or none) -> communicate_local -> update.  Without an exchange the tail
  // of iterate() (Xk <- Xak) and the local halo copy are not launched on their own but become the head of update()'s first
  // segment (the schedule's deferred launches): one submission less per iteration where the host's launch rate is what bounds
  // the group.
  int step(const std::vector<int> &locals, const std::function<int()> &exchange);
  // DPGOHash::receive (DPGOHash.cpp:45-82): msg for neighbour node beta is ((d+1) |recv[beta]|) x d,
  // [t rows ; R rows], poses in the order of recv[beta]; send() builds the message node `local` owes beta
  // from its current Xk (the poses of sent[beta], DPGO_utils.cpp:428-435)
  int receive(int local, int beta, const double *msg, int ld);
  int send(int local, int beta, double *msg, int ld) const;
  int num_recv(int local, int beta) const;
  int num_send(int local, int beta) const;

  // ---- distributed chordal initialisation (dchordal.cpp; C++/DChordal, C++/examples/dist_pgo.cpp:144-416).
  // Xlocal (optional): per-node local solutions in the global layout (stage 0); X: the initial guess, global
  // (d+1)N x d; objectives (optional): 0.5 sum |B X + b|^2 of the running stage every 20 iterations, stages in order.
  int dist_chordal_initialization(const DChordalOptions &o, const double *Xlocal, int ldl, double *X, int ld,
                                  std::vector<double> *objectives);
  // the sparse stages: setup -> initialize -> step ... -> get (DChordal_R / DChordal_t for all nodes in lockstep)
  int chordal_setup(int kind, double xi, const std::vector<std::vector<double>> &R);
  int chordal_initialize(const std::vector<std::vector<double>> &X);
  int chordal_step();
  double chordal_objective();
  int chordal_get(std::vector<std::vector<double>> &Xak);
  void chordal_release();

  // ---- AMM-PGO* (DPGOStar, C++/DPGO/src/DPGOStar.cpp:107-711); every node of the graph must be local
  int star_initialize_global(const double *X, int ld);   // DPGOStar::initialize (:107-124)
  int star_update();                                     // DPGOStar::update     (:306-313, update_n :315-390)
  int star_iterate();                                    // DPGOStar::iterate    (:126-213)
  double star_F() const { return starF_; }
  double star_fobj() const { return star_fobj_; }
  double star_fobjh() const { return star_fobjh_; }
  int star_branches() const { return star_branches_; }   // bit 0 pm, bit 1 mm, bit 2 phi fallback
  // ---- solution certificate (cert.h, cert.cpp): LOBPCG on S = M - Lambda(X) (C++/SESync/src/SESyncProblem.cpp:375-468,
  // C++/SESync/src/SESync_utils.cpp:721-830).  X: global (d+1)N x d; trivial loss, every node of the graph local; the
  // optimiser's state is untouched.  V0 (optional): the initial block, (d+1)N x d; x (optional): the returned unit vector
  int certify(const double *X, int ld, const CertOptions &o, const double *V0, int ldv0, CertResult &res, double *x, int ldx);
  int cert_lambda(const double *X, int ld, double *Lambda);   // N blocks d x d, row-major, by global pose
  int cert_apply(const double *X, int ld, const double *V, int ldv, double *SV, int ldsv);   // SV = S(X) V
  // fast_verification STEP 1 (C++/SESync/src/SESync_utils.cpp:731-754): the device Cholesky of S(X) + eta I; verify: STEP 1,
  // then the search of certify only when it did not succeed (:721-830); cert_matrix: what is factored, read back
  int cert_factor(const double *X, int ld, double eta, long long max_factor_bytes, CertFactor &out);
  int verify(const double *X, int ld, const CertOptions &o, long long max_factor_bytes, const double *V0, int ldv0, CertResult &res,
             double *x, int ldx, CertFactor &fac);
  int cert_matrix(const double *X, int ld, double eta, int *ptr, int *col, double *val, long long cap, long long *nnz);
  // ---- marginal pose covariances (cov.h, cov.cpp): the anchored tangent-space Hessian written on the device, factored,
  // and inverted inside the factor's pattern (spd.h: spd_selinv_device).  marginals: N blocks dof x dof row-major by global
  // pose; cross: one block per requested pair (p, q) of global poses, S_pq -- every pair must be an edge of the graph (or
  // p == q); cov_hessian: the matrix that is factored, read back as CSR on global poses (as cert_matrix)
  int covariance(const double *X, int ld, int anchor, long long max_bytes, const int *pairs, int npairs, double *marginals,
                 double *cross, CovResult &out);
  int cov_hessian(const double *X, int ld, int anchor, int *ptr, int *col, double *val, long long cap, long long *nnz);
  // Newton polish (polish.h): damped Riemannian Newton steps from X on the anchored tangent-space Hessian, factored in the
  // covariance's numeric context and solved with spd_vsolve_device; Xout (ldout >= (d+1) N): the new point, written unless
  // SKIPPED; log (optional, log_cap rows of POLISH_LOG_COLS doubles): one row per iteration
  int polish(const double *X, int ld, int anchor, const PolishOptions &o, long long max_bytes, double *Xout, int ldout, double *log,
             int log_cap, PolishResult &out);
  // ---- the robust objective (robust.h, robust.cpp): the polish and the covariances on the TRUE Hessian of
  // F = 1/2 sum_intra s_e + 1/2 sum_inter rho(s_e) (curvature 1), or on the re-weighted one (curvature 0).  g: a graph of
  // the group's poses whose every edge is a block of the certificate's pattern (-1 otherwise); the group itself is a
  // trivial-loss group that hosts every node, as for every call above.  robust_hessian: the anchored H as cov_hessian hands it
  // out, optionally with grad (dof N by global pose), F and per edge w, c, s_rot, s_trans, rho; robust_matrix: M_w as cert_matrix hands out S
  int robust_polish(const Graph &g, const double *X, int ld, int loss, double loss_reg, int curvature, int anchor,
                    const PolishOptions &o, long long max_bytes, double *Xout, int ldout, double *log, int log_cap, PolishResult &out,
                    EdgeSummary *sum);
  int robust_covariance(const Graph &g, const double *X, int ld, int loss, double loss_reg, int curvature, int anchor,
                        long long max_bytes, const int *pairs, int npairs, double *marginals, double *cross, CovResult &out);
  int robust_hessian(const Graph &g, const double *X, int ld, int loss, double loss_reg, int curvature, int anchor, int *ptr, int *col,
                     double *val, long long cap, long long *nnz, double *grad, double *F, double *w, double *c, double *s_rot,
                     double *s_trans, double *rho);
  int robust_matrix(const Graph &g, const double *X, int ld, int loss, double loss_reg, int *ptr, int *col, double *val, long long cap,
                    long long *nnz);
  // ---- maximum-likelihood refinement on the full information matrices (ml.h, ml.cpp): polish's loop and covariance's tail on
  // F_ml = 1/2 sum r' Omega r and its Gauss-Newton Hessian.  g: as for the robust objective, with its Omega (or Omega_iso),
  // every Omega_e symmetric positive definite (-1 otherwise, the edge named).  ml_hessian: the anchored H as cov_hessian hands
  // it out, optionally with grad (dof N by global pose) and F; ml_eval: F_ml, near_pi and per edge r (dof), chi2, and (debug) what else
  // the edge pass left: wr (dof), grad (2 dof), jw (ml_jw_doubles)
  int ml_polish(const Graph &g, const double *X, int ld, int anchor, const PolishOptions &o, long long max_bytes, double *Xout,
                int ldout, double *log, int log_cap, MlResult &out);
  int ml_covariance(const Graph &g, const double *X, int ld, int anchor, long long max_bytes, const int *pairs, int npairs,
                    double *marginals, double *cross, CovResult &out);
  int ml_hessian(const Graph &g, const double *X, int ld, int anchor, int *ptr, int *col, double *val, long long cap, long long *nnz,
                 double *grad, double *F);
  // debug: k_ml_hessian on a sentinel-padded array of its own; guards: 2 pad doubles, val: the values in ml_hessian's order
  int ml_hessian_guarded(const Graph &g, const double *X, int ld, int anchor, int pad, double sentinel, double *guards, double *val,
                         long long cap);
  int ml_eval(const Graph &g, const double *X, int ld, double *F, long long *near_pi, double *r, double *chi2, double *wr, double *grad,
              double *jw);
  // ---- edge reliability and candidate gating on the full information matrices (ml_rely.h, ml_rely.cpp): edge_reliability's
  // arguments, list semantics, methods and outputs on H = sum J' Omega J with the graph's Omega, stationarity = |g_ml|; and
  // pair_covariance's gate (SOLVE only) for candidates (R~, t~, Omega): cand_R npairs x d^2 row-major, cand_t npairs x d,
  // cand_info npairs x dof^2, each symmetric positive definite (-1 otherwise, the candidate named).  The restrictions of ml_covariance.
  int ml_edge_reliability(const Graph &g, const double *X, int ld, int anchor, long long max_bytes, int method, const int *edges,
                          int nedges, double *rec, double *rel, double *joint, RelyResult &out);
  int ml_pair_gate(const Graph &g, const double *X, int ld, int anchor, long long max_bytes, const int *pairs, int npairs,
                   const double *cand_R, const double *cand_t, const double *cand_info, double *joint, double *rel, double *gate,
                   PairsResult &out);
  // ---- graduated non-convexity on the maximum-likelihood objective (ml_gnc.h, ml_gnc.cpp): GNC-TLS / GNC-GM on chi2_e =
  // r_e' Omega_e r_e, one polish_loop per level on (F_w, g_w, H_w) with the weights of k_ml_gnc_edge.  The restrictions and the
  // refusals of ml_polish and of gnc; barc2 is a threshold on chi2.  weights: num_edges; log: log_cap rows of GNC_LOG_COLS.
  int ml_gnc(const Graph &g, const double *X, int ld, const GncOptions &o, const int *robust_set, long long max_bytes, double *Xout,
             int ldout, double *weights, double *log, int log_cap, MlGncResult &out);
  // debug: one FULL edge pass at X.  w_in null: WEIGH, the array starting as the caller's w; otherwise FIXED on w_in.  chi2, w:
  // num_edges each (w: the array behind the pass); sums: the ML_GNC_SUMS of MlGncSummaryDev as doubles; full: also what else the
  // pass left, as ml_eval hands it out (any of r, wr, grad, jw may be null)
  int ml_gnc_eval(const Graph &g, const double *X, int ld, int kind, double mu, double barc2, const int *robust_set, const double *w_in,
                  bool full, double *chi2, double *w, double *sums, double *r, double *wr, double *grad, double *jw);
  // debug: g_w and the anchored H_w of the weights w_in (FIXED) as ml_hessian hands out g and H
  int ml_gnc_hessian(const Graph &g, const double *X, int ld, int anchor, const int *robust_set, const double *w_in, int *ptr, int *col,
                     double *val, long long cap, long long *nnz, double *grad);
  // ---- graduated non-convexity (gnc.h, gnc.cpp): outlier rejection on the robust objective's plan, one polish_loop per level
  // with the weights of k_gnc_edge.  The restrictions of the robust objective; robust_set (optional, one int per edge): the
  // edges the loss may touch, instead of the inter rule.  Xout: the point (written unless SKIPPED), weights: num_edges, log
  // (optional): log_cap rows of GNC_LOG_COLS doubles, one per level k >= 1
  int gnc(const Graph &g, const double *X, int ld, const GncOptions &o, const int *robust_set, long long max_bytes, double *Xout,
          int ldout, double *weights, double *log, int log_cap, GncResult &out);
  // debug: one edge pass at X.  w_in null: WEIGH, the array starting as the caller's w; otherwise FIXED on w_in.  s_rot,
  // s_trans, w: num_edges each (w: the array behind the pass); sums: the eight of GncSummaryDev as doubles
  int gnc_eval(const Graph &g, const double *X, int ld, int kind, double mu, double barc2, const int *robust_set, const double *w_in,
               double *s_rot, double *s_trans, double *w, double *sums);
  // ---- joint covariances of arbitrary pose pairs and the loop-closure gate (pairs.h, pairs.cpp): the covariance's factor,
  // the columns of H^-1 of the poses asked for by spd_msolve_device.  pairs: npairs x 2 global poses, any two; candidates
  // (optional): npairs x (d^2 + d + 2) doubles, R~ row-major, t~, kappa, tau; joint: npairs x 3 x dof^2 (S_pp, S_pq, S_qq);
  // rel: npairs x dof^2; gate (with candidates): npairs x (2 + dof) doubles, d^2, not_pd, the residual
  int pair_covariance(const double *X, int ld, int anchor, long long max_bytes, const int *pairs, int npairs, const double *candidates,
                      double *joint, double *rel, double *gate, PairsResult &out);
  // ---- joint marginals of a pose set (marg.h, marg.cpp): the covariance's factor, the columns of H^-1 of the K kept poses,
  // Sigma_KK in LIST order; base < 0: the absolute form (n = dof K), otherwise the covariance of T_base^-1 T_k (n = dof (K - 1)).
  // cov, info (with want_info): n x n row-major; logdet: log det cov (with want_info)
  int joint_marginal(const double *X, int ld, const int *keep, int K, int anchor, int base, bool want_info, long long max_bytes,
                     double *cov, double *info, double *logdet, MargResult &out);
  // ---- joint compatibility and budgeted selection of loop-closure candidates (cand.h, cand.cpp): Sigma_KK of the candidates'
  // end poses by joint_marginal's batches, the joint innovation covariance S, its inverse and r^T S^-1 r (want_joint), and the
  // greedy selection of at most `budget` candidates by conditional information gain on the device
  int candidate_set(const double *X, int ld, const int *pairs, int m, const double *candidates, int anchor, int budget, double d2_max,
                    bool want_joint, long long max_bytes, const CandOut &o, CandResult &out);
  // ---- Hessian modes (modes.h, modes.cpp): the k smallest eigenpairs of the anchored H by shift-invert block subspace iteration
  // on the covariance's factor.  values, residuals: k; vectors: k x (dof N), row j the unit vector v_j by global pose; energy:
  // k x N, |v_j|^2 per pose; X_escape (with want_escape, leading dimension ld): a lower point along v_0 where lambda_0 < 0, else X
  int hessian_modes(const double *X, int ld, int anchor, int k, const ModesOptions &o, long long max_bytes, double *values,
                    double *residuals, double *vectors, double *energy, double *X_escape, ModesResult &out);
  // measurement: ncols unit columns solved one at a time with spd_vsolve_device on the same factor; ms: of the solves
  int pairs_vsolve_baseline(const double *X, int ld, int anchor, int ncols, double *ms);
  // ---- measurement sensitivities (sens.h, sens.cpp): the covariance's factor, the adjoints H^-1 c of k upstream gradients by
  // spd_msolve_device, and per edge of g the derivative of each L_l in (kappa, tau, t~, R~).  g: as for the robust objective;
  // upstream: (dof N) x k column-major by global pose (ldu >= dof N); adjoint (optional): (dof N) x k; sens: k x num_edges x (2 + dof)
  int sensitivity(const Graph &g, const double *X, int ld, int anchor, long long max_bytes, const double *upstream, int ldu, int k,
                  double *adjoint, double *sens, SensResult &out);
  // ---- per-edge reliability (rely.h, rely.cpp): the covariance's factor, the three blocks of every listed edge by the selected
  // inversion or by the pair covariances' batches, one record per listed edge.  g: as for the sensitivities; edges (optional):
  // nedges indices into g's edges, any order, repeats allowed -- null: all of them; rec: one row of rely_width(d) doubles per
  // listed edge; rel (optional): dof^2 per listed edge; joint (optional): 3 dof^2
  int edge_reliability(const Graph &g, const double *X, int ld, int anchor, long long max_bytes, int method, const int *edges,
                       int nedges, double *rec, double *rel, double *joint, RelyResult &out);
  // ---- ... of the ROBUST objective (rsens.h, rsens.cpp): the same on the true robust Hessian (robust_covariance's, curvature 1)
  // with the loss threshold one more parameter.  sens: k x num_edges x (3 + dof), the last entry the edge's term of dL/ddelta;
  // dloss_reg: k, their sums over the edges
  int robust_sensitivity(const Graph &g, const double *X, int ld, int loss, double loss_reg, int anchor, long long max_bytes,
                         const double *upstream, int ldu, int k, double *adjoint, double *sens, double *dloss_reg, SensResult &out);
  // ---- the Riemannian staircase (stair.h, stair.cpp): TNT at rank r, verify on Lambda(Y), the escape along the certificate's
  // direction, the rounding, the polish.  X: global (d+1)N x d; Xhat (ldx >= (d+1) N): the result, written unless SKIPPED; Y
  // (optional, (d+1)N x 2d): the final lifted point; log (optional, log_cap rows of STAIR_LOG_COLS doubles): one row per level
  int staircase(const double *X, int ld, const StairOptions &o, long long max_bytes, double *Xhat, int ldx, double *Y, int ldy,
                double *log, int log_cap, StairResult &out);
  // operator hooks on a lifted point Y ((d+1)N x 2d, zero columns >= r): F, |grad|, Lambda (N blocks d x d by global pose) and
  // grad (optional); Hess[V]; retract(Y, V); the rounding (B: 2d x d row-major, sigma: 2d, Xhat before any polish)
  int stair_eval(const double *Y, int ldy, double *F, double *gnorm, double *Lambda, double *grad, int ldg);
  int stair_hess(const double *Y, int ldy, const double *V, int ldv, double *out, int ldo);
  int stair_retract(const double *Y, int ldy, const double *V, int ldv, double *Z, int ldz);
  int stair_round(const double *Y, int ldy, double *B, double *sigma, double *Xhat, int ldx);
  // boundary exchange across groups: records of the poses other groups need
  int num_sent() const { return (int)sent_rows_.size(); }
  // device buffer, num_sent()*RS doubles; st: the stream to enqueue on (default: the group's)
  int pack_sent(double *dev_buf, hipStream_t st = nullptr);
  // counts[r] keys of rank r (concatenated in nodes/poses); slot of key k of rank r = r*stride + k
  int set_recv_layout(int nranks, int stride, const int *counts, const int *nodes, const int *poses);
  int unpack_recv(const double *dev_gathered, hipStream_t st = nullptr);   // gathered buffer of all groups
  // a lazy unpack of buf through the lists dst (neighbour rows) / src (slots), device arrays (group.cpp); -1: not taken
  int set_pending_recv(const double *buf, int count, const int *dst_dev, const int *src_dev);
  void flush_pending_recv();
  // receive lists (set_recv_layout's or a communicator's) were uploaded or released: the digest set_pending_recv keeps is stale
  // even where the new lists got the old ones' address
  void recv_lists_changed() { recv_gen_++; }
  // the exchange's pack rides on the tail of iterate(): rows (device) of the records to pack, how many, where to (null: off);
  // take_packed(): whether the last iterate() did it (and forgets it)
  void set_exchange_pack(const int *rows_dev, int n, double *dst) { pack_rows_ = rows_dev; pack_n_ = n; pack_dst_ = dst; packed_ = false; }
  bool take_packed() { const bool p = packed_; packed_ = false; return p; }
  // a wait for the group's stream ran into its deadline (a collective enqueued on it never ends): called before the error is raised
  void set_stuck_handler(void (*fn)(void *), void *user) { sched_.set_stuck_handler(fn, user); }
  // an exchange running on another stream (comm.cpp): `done` is recorded behind its unpack.  update() queues the
  // part of the surrogate build that needs no neighbour row, then makes the group's stream wait for it.
  void set_pending_exchange(hipEvent_t done) { xchg_done_ = done; }
  int device() const { return device_; }
  // AMM-PGO* across groups: the master's global objective needs the trial point's boundary poses of the other
  // groups (all-gather of `send` into `gathered`, stream-ordered on stream()) and sums of scalars over the groups
  typedef int (*AllGatherFn)(void *user);
  typedef int (*AllReduceFn)(void *user, double *vals, int n);
  int set_collectives(double *send_dev, double *gathered_dev, AllGatherFn ag, AllReduceFn ar, void *user);
  // optional: an in-place sum of n DEVICE doubles over the groups, enqueued on this group's stream (RCCL: comm.cpp).  With
  // it AMM-PGO*'s master sums never visit the host between the kernels that produce them and the one read-back.
  typedef int (*AllReduceDevFn)(void *user, double *dev_vals, int n);
  void set_device_allreduce(AllReduceDevFn f) { coll_allreduce_dev_ = f; }
  // results
  int get_Xk(int local, double *X, int ld) const;       // (d+1)(n0+n1) x d column-major
  int get_X_own(int local, double *X, int ld) const;    // Xak: (d+1) n0 x d
  int scatter_global(double *X, int ld) const;          // writes own poses into the global layout
  void sync() const;
  hipStream_t stream() const { return st_; }

  // test hooks (tests/ compare single operators with the oracle)
  int debug_apply(int local, const char *op, const double *in, int ld_in, double *out, int ld_out);
  // The scalar kernels of the truncated CG on GIVEN partial sums: a script of launches, each through its production launcher
  // (launch_cg_begin, launch_tnt_begin, launch_cg_scal, launch_cg_scal_begin) on the group's own segment table, records,
  // masks, pinned summaries and flag; the state after every launch is read back.  Nothing here computes: the entry feeds
  // inputs and reads state.
  // ... and the trial point's reduction with the gate of a speculative update behind the steps (tests/test_gpu_gate.py):
  // reduce_gate is launch_reduce_gate as speculate_update() makes it -- the group's own partial sums, pinned scalars, flag,
  // device sums, refinement start (what the script's scal_begin left), CG records, gate word and pinned verdict -- with the
  // per-node scalars and the options of the gate handed in; reduce is launch_reduce(own rows) on the same sums, for comparison
  enum CgDebugKind { CG_DBG_BEGIN_HOST = 0, CG_DBG_BEGIN_DEVICE, CG_DBG_SCAL0, CG_DBG_SCAL1, CG_DBG_SCAL_BEGIN, CG_DBG_REDUCE_GATE,
                     CG_DBG_REDUCE, CG_DBG_KINDS };
  struct GateDebug {   // (reduce_gate; reduce reads nslots only)
    int nslots = 0, max_it = 0, max_acc = 0, max_hits0 = 0, max_hits1 = 0;
    double rel_tol = 0, step_tol = 0, psi = 0, phi = 0;
    const double *f = nullptr, *Fk0 = nullptr, *Fk1 = nullptr, *fobj = nullptr;   // per local node
    const int *hits0 = nullptr, *hits1 = nullptr;
  };
  struct CgDebugLaunch {
    const GateDebug *gate = nullptr;
    int kind = 0;
    NodeBits bits = 0;                                        // the candidates (the begin kinds)
    int use_precon = 0, max_it = 0;
    double grad_tol = 0, pgrad_tol = 0, kappa = 0, theta = 0; // (begin_device, scal_begin)
    const double *rv = nullptr, *Delta = nullptr, *target = nullptr;   // per local node; rv and target: begin_host only
    const double *partials = nullptr;                         // slots x nseg_all, copied into the partial sums before the launch
    int slots = 0;
  };
  static constexpr int CG_DBG_RECORD = 17;   // a CgNode as doubles, in the order of its fields
  // per launch i: records[i][node][CG_DBG_RECORD], masks[i][3], cg_summary[i][node][CG_SUMMARY], tnt_summary and dev_tnt
  // [i][node][TNT_SUMMARY] (pinned / device), seq[i][2] = the host flag's value once the launch is over and the last sequence
  // number given out, arrived[i] = the flag's arrival counter
  // where the script has a reduce_gate or a reduce: gate_sums[i][2][node][MAX_SLOTS] (the pinned scalars, the device copy)
  // and gate_words[i][2] (the gate's word, the bits of the pinned verdict)
  int debug_cg_scalars(const CgDebugLaunch *script, int n, double *records, unsigned long long *masks, double *cg_summary,
                       double *tnt_summary, double *dev_tnt, unsigned long long *seq, unsigned *arrived, double *gate_sums,
                       unsigned long long *gate_words);
  // AMM-PGO*'s master sums on given partial sums (MAX_SLOTS x nseg_all): launch_star_sums with star_sums()'s slot table and
  // launch_publish on the group's flag, as star_sums() makes them.  out[0..3]: the device values, out[4..7]: the pinned ones;
  // seq[2]: the flag's value, the last sequence number given out
  int debug_star_sums(const double *partials, unsigned valid, double *out, unsigned long long *seq);
  // The launches speculate_update() enqueues behind its gate (update_continuation) under a GIVEN gate word, 0 or all ones, on a
  // group whose every node is past its first iteration (robust loss, Static rescale): between iterate() and update() with the
  // buffers in the roles of the accepted step (roles_accepted, what speculate_update() hands them), behind update() in the
  // roles they have now (roles_now).  Every buffer the launches may write is saved before and put back afterwards: the group can
  // go on.  report[3 k + 0..2] for buffer k of GATED_BUFFERS (Xk, X[iter], X[iter-1], g, g[iter-1], Dfobj, Dfobj[iter-1], G X,
  // G X[iter-1], the partial sums, DfobjE, the edge weights): present; bit-identical to the saved copy after the gated launches;
  // (all ones only, else -1) the gated launches' result bit-identical to that of the same launches without a gate from the
  // same saved state
  static constexpr int GATED_BUFFERS = 12;
  int debug_gated_update(NodeBits go_word, int *report);
  // One CG of a refinement round on given points, linear terms and radii (tnt.cpp), through TntRun's own pieces
  static constexpr int STPCG_DBG_SCALARS = 12;
  int debug_stpcg(const std::vector<int> &nodes, const double *in, int ld_in, const double *Delta, bool device_start, double fill,
                  double *out, int ld_out, double *scalars);
  // The inter-edge pass, the objective and the Dynamic rescale on GIVEN inputs (debug_inter.cpp; tests/test_gpu_inter.py,
  // tests/test_gpu_rescale_ops.py): each enqueues the launch the iteration makes -- update_inter_pass, prepare_extrapolated (+ the
  // proximal step amm_head() adds where the pass did not take it), launch_cost, launch_rescale_decide + rescale_device -- on the
  // group's own records and operators.  Matrices are reference layout, column-major, contiguous: "all" = (d+1)(n0+n1) x d (own
  // and neighbour rows of node `local`), "own" = (d+1) n0 x d.  `whole`: under the whole group's mask, the other nodes' rows zero.
  // They overwrite the group's iterates (DfE, and debug_inter_iterate the whole history): not for a group that iterates on.
  struct InterUpdateDebug {
    int local = 0, whole = 0, quad = 0, with_Df = 0;
    const double *Z = nullptr, *Zprev = nullptr, *DfE_old = nullptr;   // all
    const double *GX = nullptr, *X = nullptr;                          // own (with_Df)
    const double *Znbr = nullptr;                                      // all (halo: its neighbour rows are the ones read)
    const double *recv = nullptr; int nrecv = 0; const int *nsrc = nullptr;   // lazy: (d+1) nrecv x d, and n1 slots (-1: not delivered)
    double *DfE = nullptr, *g = nullptr, *w = nullptr, *sums = nullptr, *Df = nullptr;   // all, own, m1, 5 (slots 0..4), own
    double *Z_after = nullptr, *Znbr_after = nullptr;                  // all
  };
  int debug_inter_update(const InterUpdateDebug &q);
  struct InterIterateDebug {
    int local = 0, whole = 0, fused = 1, prox = 0, gamma_dev = 0;
    const double *Zc = nullptr, *Zp = nullptr;                         // all
    const double *GXc = nullptr, *GXp = nullptr, *Xref = nullptr;      // own
    const double *gamma = nullptr;                                     // one per node of the group
    double *Y = nullptr, *g = nullptr, *Df = nullptr, *Xout = nullptr, *Xref_after = nullptr, *sums = nullptr;   // all, own x4, 2 (<Y, g>, |Xout - Xref|^2)
  };
  int debug_inter_iterate(const InterIterateDebug &q);
  int debug_cost(int local, int whole, int eform, const double *Z, double *sums);   // Z: all; sums: k_cost's two slots
  // w, scale: one per inter-node edge of the GROUP (node a's from debug_edge_offsets()[a]); count: one per node; nodes: the set.
  // Out: flags / host_flags / count_out per node, scale_out per edge.  Returns the number of rescaled nodes, -1 on an error.
  int debug_rescale(const double *w, const double *scale, const int *count, int max_rescale_count, const int *nodes, int n,
                    int *flags, double *host_flags, double *scale_out, int *count_out);
  const std::vector<int> &debug_edge_offsets() const { return e_off_; }
  // The kernels of the certificate's search on GIVEN inputs (debug_cert.cpp; tests/test_gpu_cert_search.py): each copies
  // reference-layout matrices ((d+1)N x d, column-major, leading dimension ld) into CertState's buffers with cert_upload, makes
  // the launch cert_search makes -- launch_cert_gram / launch_cert_update, then launch_cert_reduce over all cert_nsums(d)
  // sums -- and reads the results back with cert_download.  Nothing here computes.  Preconditions of certify.
  // gram: cert_prepare(X) for Lambda; S W's buffer takes MW, or (MW null) cert_apply_M(W) as in the loop.  sums: the
  // cert_nsums(d) host sums as k_cert_reduce left them (both upper triangles in cert_tri order first); SW: the finished S W
  int debug_cert_gram(const double *X, const double *V, const double *W, const double *P, const double *SV, const double *SP,
                      const double *MW, int ld, double *sums, double *SW);
  // update: C 3d x d row-major and theta[d] go into a CertCoef; precondition: cert_build_precon() and its T_p, else null.
  // The neighbour rows of V, W, P are set to nbr_fill before the launch and handed back raw in nbr (3 P1 RS doubles: V's,
  // W's, P's records).  out: V', W', P', SV', SW (as the launch left it), SP', each (d+1)N x d with ld; sums: cert_nsums(d)
  struct CertUpdateDebug {
    const double *C = nullptr, *theta = nullptr, *V = nullptr, *W = nullptr, *P = nullptr, *SV = nullptr, *SW = nullptr, *SP = nullptr;
    int ld = 0, precondition = 0;
    double nbr_fill = 0;
    double *out[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, *sums = nullptr, *nbr = nullptr;
  };
  int debug_cert_update(const CertUpdateDebug &q);
  int debug_cert_nbr_rows() const { return P1_; }
  int debug_cert_precon(double *T);   // the T_p cert_build_precon uploaded: N blocks (d+1) x (d+1) row-major by global pose
  // the trace of the production search: on / off (off: cert_search is what it is without); the records of the last search
  void debug_cert_trace(bool on) { cert_trace_on_ = on; cert_trace_.clear(); }
  int cert_trace_len() const { return cert_nsums(d_) + 2 + d_ + 3 * d_ * d_ + 1; }
  const std::vector<double> &debug_cert_trace_records() const { return cert_trace_; }
  // the segment table the partial sums are laid out by: nseg_all, and per node its own / neighbour segments [ptr[a], ptr[a+1])
  int debug_seg_layout(int *nseg_all, int *own_ptr, int *nbr_ptr) const;
  const NodeOperators &host_ops(int local) const { return ops_[local]; }
  const SpdFactor &factor_tt() const { return Ltt_.F; }
  const SpdFactor &factor_rr() const { return Lrr_.F; }
  double lambda_max(int local) const { return lambda_max_[local]; }
  // (sent list across groups) unified own row of every boundary pose this group exports, with key
  const std::vector<std::pair<int, int>> &sent_keys() const { return sent_keys_; }
  const std::vector<int> &sent_rows() const { return sent_rows_; }
  // (node, pose) of every neighbour row whose owner lives in another group, and that row (unified numbering)
  void needed_keys(std::vector<std::pair<int, int>> &keys, std::vector<int> &rows) const;
  int num_records() const { return P0_ + P1_; }
  double *Xk_records() { return Xk_.p; }
  // dst[didx[k]] = src[sidx[k]] over pose records (didx may be null: dst[k]) on stream st
  void copy_records(hipStream_t st, int count, const int *didx, const int *sidx, const double *src, double *dst) const;

 private:
  bool ok_ = false;
  // A Dynamic rescale on the device commits its scales before the verdict on the new factor of G_tt is in (the host never
  // waits for it: rescale_device).  A non-positive pivot -- which the reference reports from inside its CHOLMOD call --
  // therefore leaves the group with operators it cannot solve with: it is marked failed and every later update() /
  // iterate() returns -1 (a new group is the way on; nothing is silently computed with a broken factor).
  mutable bool failed_ = false;
  int d_ = 0, RS_ = 0, B_ = 0, device_ = 0;
  Options opt_;
  std::vector<int> nodes_;
  std::map<int, int> local_of_node_;
  std::vector<DataInfo> info_;
  std::vector<NodeOperators> ops_;
  std::vector<NodeResults> res_;
  std::vector<double> lambda_max_;
  std::vector<std::map<int, int>> g_index_;   // per local node: local pose -> global pose
  int num_poses_global_ = 0, num_nodes_total_ = 1;
  // unified rows
  int P0_ = 0, P1_ = 0;
  std::vector<int> own_off_, nbr_off_;
  // how the launches reach the GPU and how the host learns they are done (schedule.h); st_: its stream (not owned)
  Schedule sched_;
  hipStream_t st_ = nullptr;

  // device data
  DevBuf<Seg> segs_;
  DevBuf<int> own_seg_ptr_, nbr_seg_ptr_;
  SegTable T_;
  // masks and per-node coefficients live in rings (device + pinned host), so changing them never
  // needs a stream synchronisation
  NodeMask cur_mask_ = ALL_NODES;  // the nodes the launches work on (set_mask), passed to the kernels by value
  double *h_scal_ = nullptr;       // pinned (the schedule's block, in front of its flag), written by k_reduce
  // a refactorisation of G_tt whose verdict (positive definite or not) has not been read yet: it is read at the first
  // wait for a read-back that was enqueued behind it (sequence number >= tt_verdict_seq_), or at sync()
  mutable bool tt_verdict_pending_ = false;
  unsigned long long tt_verdict_seq_ = 0;
  void check_tt_verdict(bool wait) const;
  double *h_cg_ = nullptr, *h_tnt_ = nullptr;   // pinned summaries of k_cg_scal / k_tnt_begin (the block behind the flag)
  bool zc_ready_ = false;       // iterate() wrote Xk's own rows into the buffer the next update() rotates into X[iter]
  bool tnt_speculate_ = true;   // run_tnt: take the trial point behind the first CG step without waiting for its outcome
  // ---- The branch-free SEGMENTS of an iteration as graph replays (schedule.h).  Between two read-backs an iteration is a fixed
  // sequence of launches -- update() behind the exchange, the start of iterate() up to the translation solve, a refinement from
  // its model gradient to the trial point's sums, a whole CG step (tnt.cpp) -- whose arguments are pointers, node sets and
  // constants: everything that changes from one iteration to the next lives in device memory (the Nesterov gammas: coefs_dev_,
  // written by the one eager launch of update(); the flag's sequence number; the CG's masks and step lengths).  segment() runs
  // such a sequence through the schedule, keyed by the buffers it touches (which rotate), the node set and the variant.  Rare
  // branches (a rejected step, a restart, a fallback, a Dynamic rescale) stay eager.  Bitwise the same results.
  // bits: the nodes the sequence works on.  Only sequences over ALL the group's nodes are replayed: a partial set is a group
  // whose nodes are taking different branches, where the sets change from one iteration to the next and every new set
  // would be a new capture (measured: city10000 / 8 nodes with every subset captured ran 4 x slower than eagerly)
  // wanted: -1 = by the schedule's iter_graph_wanted(), 0 / 1 = the caller's own policy (the CG steps: cg_graph_wanted)
  void segment(int id, NodeBits bits, std::initializer_list<unsigned long long> extra, const std::function<void()> &body,
               int wanted = -1);
  NodeBits all_bits() const { const int L = num_local(); return L >= 64 ? ~0ull : ((1ull << L) - 1); }
  DevBuf<double> coefs_dev_;  // per local node: gamma of the iteration under way (k_set_coefs)
 public:
  // (counters for the tests and the API-trace summary: replays, captures, segments run eagerly)
  void graph_stats(long *replays, long *captures, long *eager) const { sched_.stats(replays, captures, eager); }
 private:
  // the mask of the nodes in `bits` (and-ed on the device with *p, if any) with the map that lets own-segment launches
  // cover these nodes only (kernels.h: NodeMask::nlive) when they are few
  NodeMask live_mask(NodeBits bits, const NodeBits *p) const;
  std::vector<int> own_seg_ptr_host_;
  // the fusions of round 6 (extrapolation and Dfobj inside the inter-edge pass, iterate()'s tail on the product with G, the
  // first CG step's vector update with the retraction): DPGO_FUSED=0 gives round 5's launch sequence (A/B hook; same bits)
  bool fused_ = true;
  // ---- update() and what it shares with iterate() and run_tnt() (update.cpp).  Its launches take the buffers by ROLE -- the
  // own records' source, Xk, X[iter], X[iter-1], g, Dfobj, the kept product G X (T1_ where it is not kept), the base of its partial
  // sums -- so that update() (the roles as they stand) and speculate_update() (as they will stand) share one statement of them
  struct UpdateRoles {
    const double *xak = nullptr, *zp = nullptr;
    double *xk = nullptr, *zc = nullptr, *gc = nullptr, *dfc = nullptr, *gx = nullptr, *pupd = nullptr;
    const char *differs(const UpdateRoles &o) const;   // the first role that differs, null: none
    bool operator==(const UpdateRoles &o) const { return !differs(o); }
  };
  UpdateRoles roles_now() const;                           // from the members as they stand
  UpdateRoles roles_accepted(const double *xprop) const;   // ... once the trial point xprop is accepted and the history has rotated
  // What a sequence that closes an update() is enqueued with: the roles and the scalar facts that shape it
  struct UpdateDesc {
    UpdateRoles roles;
    int seg_id = 0, nslots = 0;
    NodeBits bits = 0;                  // the nodes of the sequence
    bool fuse_copy = false, split = false, lazy_recv = false, deferred = false, tail = false;
    unsigned long long seq_last = 0;    // the last sequence number given out when the sequence was complete
    const char *differs(const UpdateDesc &o) const;
  };
  // The tail of iterate() -- Xk <- Xak, and the buffer the next update() rotates into X[iter] -- waits for that update()'s
  // product with G, which reads the same records anyway and stores them on the way (k_bsr's copy1 / copy2): armed by step()
  // when no exchange stands between the two (the exchange's pack reads Xk); anything else launches it on its own.
  struct PendingTail { bool on = false; NodeMask m = ALL_NODES; const double *xak = nullptr; double *xk = nullptr, *z = nullptr; };
  PendingTail pending_tail_;
  bool tail_fusable_ = false;
  void flush_pending_tail();
  // The next update() enqueued AHEAD of the host's decision (round 6).  Between the trial point's read-back and the first
  // launch of update() the GPU used to idle for the host's acceptance test and bookkeeping (~13-17 us of an iteration of
  // 0.35-1.25 ms).  In the regime where that decision always comes out the same way -- every node refined, its CG over after
  // one step, the step accepted, no redo, no restart, no fallback: the whole early regime -- run_tnt() enqueues, right behind
  // the last kernel of the trial point and before it waits for it: the trial point's reduction with a GATE in the same launch
  // (k_reduce_gate) that takes that very decision on the device from the same sums, and the launches the common course leads to -- the local halo copy, update()'s product with G
  // (which carries iterate()'s tail) and its inter-edge pass and reduction, with the buffers in the roles they will have
  // after the accepted step and the rotation of the history -- under the device word the gate sets.  The host then takes its
  // decision as ever; if it is the common one, iterate() / communicate_local() / update() find their launches done and only
  // do their bookkeeping; if not, those launches have fallen through (they touched nothing) and the normal path runs.  The
  // two verdicts come from the same bits through the same operations; the host checks that they agree when it next waits
  // (finish_update).  Armed by step() without an exchange; eager launches only; DPGO_SPEC_UPDATE=0 switches it off.
  struct SpecUpdate {
    bool on = false;
    unsigned long long seq_trial = 0;  // the flag of the trial point's reduction (+ gate)
    bool lazy = false;                 // the continuation left update()'s reduction to the next refinement (UpdLazy)
    UpdateDesc what;                   // what the continuation was enqueued with (update() compares it with what it finds)
  };
  SpecUpdate spec_upd_;
  long n_spec_enqueued_ = 0, n_spec_stood_ = 0;   // (DPGO_HOST_TIMING=1 prints them)
  bool spec_update_armed_ = false, spec_update_enabled_ = true;
  bool tnt_common_ = false;          // run_tnt: the refinement took the common course (one step, accepted by every node, over)
  DevBuf<NodeBits> go_;              // the gate's word
  DevBuf<double> dev_sums_, dev_tnt_;   // the trial point's sums / the refinement's start, per node, in device memory
  double *h_gate_ = nullptr;         // pinned (same allocation as h_scal_): the gate's verdict
  bool spec_verdict_pending_ = false, spec_verdict_expected_ = false;   // the host acted on its own verdict; the gate's is compared at the next wait
  unsigned long long spec_verdict_seq_ = 0;
  bool spec_update_possible(const double *xprop) const;
  void speculate_update(const double *xprop, int nslots_trial);   // run_tnt: the trial point's reduction + gate, then the continuation
  // what the gate gets by value: the options it tests against and, per node, the scalars of the last update()
  // (speculate_update: opt_ and res_; debug_cg_scalars: the script's)
  void update_continuation(const UpdateRoles &r, const NodeBits *gate);   // the launches speculate_update() enqueues behind the gate
  struct GateNode { double f, Fk0, Fk1, fobj; int hits0, hits1; };
  static AmmGate amm_gate(int L, const Options &o, const std::function<GateNode(int)> &node);
  void check_gate(bool host_common);
  // update()'s closing reduction is only read by the host, late (finish_update): where the read-back is deferred the
  // reduction is not launched at all but rides on the next refinement's k_cg_scal_begin (one workgroup per node anyway),
  // from partial-sum slots of its own; if no refinement comes, finish_update() launches it
  struct UpdLazy { bool pending = false; int nslots = 0; };
  UpdLazy upd_lazy_;
  bool lazy_update_reduce() const;
  double *upd_slots() const { return partials_.p + (size_t)UPD_SLOT0 * T_.nseg_all; }   // update()'s own partial-sum slots
  // the stated sequence (m: the nodes, possibly under the gate's word; r: the roles)
  void update_product(const NodeMask &m, const UpdateRoles &r, bool from_xak, bool carry_tail);   // G X and <X, 1/2 G X> (slot 5)
  void update_inter_pass(const NodeMask &m, const UpdateRoles &r, bool quad, bool with_Df, const double *lazy_recv,
                         double *wout = nullptr);   // wout: the weights go there (a test hook; else to e_w_ with Dynamic rescale)
  void update_reduce(int nslots, const double *pupd);   // the closing reduction into h_upd_
  // The host-side facts of one update() call, computed once (plan_update); the phases below run over it
  struct UpdatePlan {
    std::vector<int> locals, adv, first, later;   // the nodes to update; whose history advances; at their first / a later iteration
    NodeBits bits = 0;                            // of locals
    NodeMask mask = ALL_NODES;                    // ... and their mask
    bool trivial = false, rotate = false, both = false, can_defer = false, fuse_copy = false, split = false;
    const double *lazy_recv = nullptr;            // the receive buffer the inter-edge pass unpacks on the way (robust losses)
  };
  UpdatePlan plan_update(const std::vector<int> &locals_in) const;
  void advance_history(const UpdatePlan &p);      // the rotation or copy, and X[iter]'s own rows
  void update_head(const UpdatePlan &p, const UpdateRoles &r);   // the product with G where it has not gone ahead of an exchange
  void build_trivial(const UpdatePlan &p, const UpdateRoles &r);
  void trivial_common(const UpdatePlan &p, const UpdateRoles &r);
  void trivial_launches(const UpdatePlan &p, const UpdateRoles &r, bool later);
  void build_robust(const UpdatePlan &p, const UpdateRoles &r);
  void dynamic_detour(const UpdateRoles &r, const std::vector<int> &set, bool quad, std::vector<double> &rho, std::vector<double> &gap);
  void robust_launches(const UpdatePlan &p, const UpdateRoles &r, const std::vector<int> &set, const std::vector<int> &fresh, bool quad, bool head_inside);
  void close_update(const UpdatePlan &p, const UpdateRoles &r, int seg_id, unsigned long long variant, int nslots,
                    const std::vector<int> &set, const std::function<void()> &launches, std::function<void()> logic);
  void host_update_logic(int local, double fobj, double f, double gradFnorm);
  // The read-back that ends update() is deferred where nothing has to be decided yet: update() enqueues the reduction,
  // advances the Nesterov sequence (host_update_pre: s, gamma -- they do not depend on the numbers read back) and
  // returns; the next iterate() queues its extrapolation, proximal step and translation solve and only then waits
  // (finish_update), so the GPU does not idle while the host takes the scalars.  Every other reader of the node state
  // or of the pinned scalars calls finish_update() first.
  void host_update_pre(int local);
  void finish_update();
  std::function<void()> pending_update_;
  unsigned long long pending_seq_ = 0;
  DevBuf<double> partials_;
  DevBuf<CgNode> cg_;       // device-resident state of the truncated CG (tnt.cpp, k_cg_scal)
  DevBuf<double> jacobi_;   // Preconditioner::Jacobi: 1 / diag(G_RR), one entry per rotation row
  DevBuf<NodeBits> dmask_;  // [0] nodes taking the next Hessian product, [1] nodes going on to the preconditioner, [2] nodes whose CG is over
  struct BsrBufs { DevBuf<int> ptr, col; DevBuf<double> val, tcol; BsrDev dev; };   // tcol: first column of every block (G only)
  BsrBufs G_, S_, P_, P0m_, Q_;
  DevBuf<double> Dd_, Qd_, Tinv_, N_, V_;
  DevBuf<int> e_tail_, e_head_, e_inc_ptr_, e_inc_;
  DevBuf<double> e_R_, e_t_, e_kappa_, e_tau_;
  DevBuf<InterInc> e_rec_;        // the same data once more, one record per incidence (k_inter)
  InterEdgesDev E_;
  DevBuf<int> i_tail_, i_head_, i_inc_ptr_, i_inc_;
  DevBuf<double> i_R_, i_t_, i_kappa_, i_tau_;
  InterEdgesDev Ei_;              // intra-node edges in residual form (objective evaluation only)
  SpdSolverDev Ltt_, Lrr_;
  // halo
  DevBuf<int> gather_dst_, gather_src_;   // local halo copy lists
  std::vector<int> sent_rows_;     // unified own rows exported to other groups
  std::vector<std::pair<int, int>> sent_keys_;   // (node, pose) of each exported row
  DevBuf<int> sent_rows_dev_;
  DevBuf<int> recv_dst_, recv_src_;       // remote halo: nbr row <- gathered slot
  const double *pending_recv_ = nullptr;  // a lazy unpack nobody has consumed yet (set_pending_recv)
  const int *recv_key_ = nullptr, *recv_dst_dev_ = nullptr, *recv_src_dev_ = nullptr;
  int recv_count_ = 0;
  unsigned long long recv_gen_ = 1, recv_key_gen_ = 0;   // the digest is valid for generation recv_key_gen_ of the lists
  DevBuf<int> recv_nsrc_;                 // per neighbour row: its slot in the receive buffer, -1: none
  std::vector<InterInc> e_rec_host_;      // host copy of the incidence records (their osrc field follows the receive lay-out)
  const int *pack_rows_ = nullptr;
  int pack_n_ = 0;
  double *pack_dst_ = nullptr;
  bool packed_ = false;
  // vectors (records)
  DevBuf<double> Xk_, Zc_, Zp_, Y_, DfE_, Tall_;                 // P0+P1 rows
  DevBuf<double> Xak_, Xakh_, gc_, gp_, Dfc_, Dfp_, gx_, Dfx_, T1_;   // P0 rows
  // robust loss, Static rescale: G X[k] and G X[k-1] (own rows), rotated with the history of X: the product with G at the
  // extrapolated point is their linear combination (prepare_extrapolated), one pass over the operator less per iteration
  DevBuf<double> GXc_, GXp_;
  bool keep_gx() const { return opt_.loss != 0 && !dynamic(); }
  DevBuf<double> tmp_[14];                                       // P0 rows, TNT work vectors
  DevBuf<double> dbg_X_, dbg_g_;                                 // debug_stpcg's point and linear term (allocated by its first call)
  // own rows of node a between a device record array and a reference-layout matrix (column-major, leading dimension ld;
  // translations from row row_t0, rotation rows from row_r0): the debug entries' upload / download
  void put_rows(int a, double *dev, const double *X, int ld, int row_t0, int row_r0, bool has_t);
  void get_rows(int a, const double *dev, double *X, int ld, int row_t0, int row_r0, bool has_t);
  // ... and its neighbour rows (dev: an array over own AND neighbour rows)
  void put_nbr_rows(int a, double *dev, const double *X, int ld, int row_t0, int row_r0);
  void get_nbr_rows(int a, const double *dev, double *X, int ld, int row_t0, int row_r0);
  DevBuf<double> dbg_all_[4], dbg_w_;                            // the debug inter-edge entries' operands over all rows, and the weights
  hipEvent_t xchg_done_ = nullptr;   // pending boundary exchange (not owned)
  void join_exchange();              // the group's stream waits for it
  struct ChordalState;
  ChordalState *ch_ = nullptr;
  struct CertState;   // the certificate's buffers (cert.cpp), allocated by the first call
  CertState *cert_ = nullptr;
  void cert_release();
  int cert_begin(const double *X, int ld);
  int cert_ready();   // cert_begin without the check of X: the group's loss and nodes, the optimiser's pending work, the buffers
  int cert_prepare(const double *X, int ld, double *stationarity);
  void cert_upload(const double *M, int ld, int ncols, double *dev_all, bool with_nbr = true);
  void cert_download(const double *dev_own, double *M, int ld, int ncols);
  void cert_apply_M(double *in_all, double *out_own);
  void cert_apply_S(double *in_all, double *out_own);
  void cert_build_precon();
  void cert_build_pattern();
  int cert_factor_setup(long long max_factor_bytes, CertFactor &out);   // 0: ready to factor, 1: SKIPPED, -1: error
  int cert_factor_numeric(double eta, CertFactor &out);                 // S + eta I from the Lambda in place, factored
  int cert_search(const CertOptions &o, const double *V0, int ldv0, CertResult &res, double *x, int ldx);   // LOBPCG, likewise
  // debug_cert_trace: one record of cert_trace_len() doubles per pass of cert_search's inner loop that reached its update
  // (debug_cert.cpp); off, cert_search does not touch it
  bool cert_trace_on_ = false;
  std::vector<double> cert_trace_;
  void cert_trace_pass(const double *sums, int nblk, int used, const CertCoef &K);
  int verify_lambda(const CertOptions &o, long long max_factor_bytes, double stationarity, CertResult &res, double *x, int ldx,
                    CertFactor &fac);
  struct StairState;  // the staircase's lifted vectors (stair.cpp), allocated by the first call that is not refused
  StairState *stair_ = nullptr;
  void stair_release();
  int stair_begin(const double *X, int ld, long long max_bytes, long long *bytes);   // 0: ready, 1: SKIPPED, -1: error
  struct StairPoint;  // the buffers of one lifted point: Y, M Y, grad, Lambda
  void stair_upload(const double *X, int ld, int ncols, const struct Lifted &dst);
  void stair_download(const struct LiftedC &src, double *X, int ld);
  void stair_apply_M(const struct Lifted &in_all, const struct Lifted &out_own, int rank);
  void stair_eval_point(StairPoint &p, int rank, bool store_grad, double *F, double *gnorm);
  double stair_hess_product(StairPoint &p, int rank, const struct Lifted &V_all, const struct Lifted &MV, const struct Lifted &out,
                            double *ww, double *vv);
  int stair_tnt(const StairOptions &o, int rank, double *F, double *gnorm, int *iters, int *products);
  int stair_round_point(int rank, double *Bout, double *sigma, double *Xhat, int ldx);
  struct CovState;    // the covariance's pattern, factor and blocks (cov.cpp), allocated by the first call
  CovState *cov_ = nullptr;
  void cov_release();
  int cov_begin(const double *X, int ld, int anchor);
  int cov_analyse(HessAnalysis &out);   // the pattern and the symbolic analysis (first call), the sizes
  // What every consumer of the factor shares (hess.cpp).  hess_reserve, the one refusal, behind cov_analyse: 0 ready (the
  // numeric context set up on its first use), 1 SKIPPED, -1 error; device_bytes <- the sum of the parts.  hess_factor, the one
  // verdict: write_H launched, the factorisation, the pivots, factor_ms: 0 factored, 1 NOT_PD (synchronised), -1 error;
  // hess_refactor: its part from the factorisation to the pivots, which polish_loop's own loop shares
  bool device_has_room(long long remain);
  int hess_reserve(long long max_bytes, const char *who, std::initializer_list<HessPart> parts, HessAnalysis &out);
  int hess_refactor(const char *who, HessAnalysis &out);
  int hess_factor(const char *who, const std::function<void()> &write_H, HessAnalysis &out);
  // the maps of the certificate's pattern (cert.cpp, behind cert_build_pattern): global pose -> unified own row; the block
  // that holds (p, q), -1: none
  int own_row(int global_pose) const;
  int cert_block_of(int p, int q) const;
  // the callers' refusals, each the analysis and its list of parts; extra: bytes the caller allocates behind the same refusal
  // (robust.cpp, gnc.cpp).  cov_setup: with the blocks of the selected inversion (cov.cpp); polish_setup: with the vector solve
  // and polish's vectors, which it allocates (polish.cpp)
  int cov_setup(long long max_bytes, CovResult &out, HessPart extra = {0, 0});
  int polish_setup(long long max_bytes, HessAnalysis &out, HessPart extra = {0, 0});
  // the pair arguments of covariance, robust_covariance and pair_covariance: poses of the graph; edges of it (cov.cpp)
  bool pairs_args_ok(const char *who, const int *pairs, int npairs) const;
  bool pairs_are_edges(const char *who, const int *pairs, int npairs) const;
  void launch_cov_hessian_at(int arow);   // k_cov_hessian on the certificate's M, Lambda, X into the factor's values
  // covariance's tail: write_H and the factorisation (hess_factor), the selected inversion, the read-out
  int cov_finish(const std::function<void()> &write_H, int arow, const int *pairs, int npairs, double *marginals, double *cross,
                 CovResult &out);
  // a value array in the order of the certificate's / the covariance's pattern as CSR on global poses (cert_matrix, cov_hessian)
  void cert_csr_out(const std::vector<double> &v, int *ptr, int *col, double *val);
  void cov_csr_out(const std::vector<double> &v, int *ptr, int *col, double *val);
  // The loop of the Newton polish (polish.cpp) on CertState's X, shared by polish and robust_polish.  What differs is launched
  // by the caller's hooks: point -- M X (or M_w X) into MX, Lambda, g, |g|^2 into slot 0 and F into slot 1 of the partials;
  // hessian -- H at X into the factorisation's values; trial -- F at the trial point V into slot 2
  struct PolishHooks {
    std::function<void()> point, hessian, trial;
  };
  int polish_loop(const double *X, int ld, int arow, const PolishOptions &o, const PolishHooks &hooks, double *Xout, int ldout,
                  double *log, int log_cap, PolishResult &out);
  // The outer loop of graduated non-convexity (gnc.h; gnc.cpp), shared by gnc and ml_gnc, behind the caller's begin, refusal and
  // allocation: the option check (who names the caller), level 0, the levels and the read-out into out, Xout, weights and log;
  // last (optional): the summary the result's sums were read from.  What an objective is to it, filled by the caller:
  struct GncObjective {
    // the edge pass at a device point with the weights written (weigh) or read; per_edge: with what only a point needs (gnc:
    // the rows; ml_gnc: FULL); fslot as robust_eval
    std::function<void(const double *Xdev, double mu, bool weigh, bool per_edge, int fslot)> pass;
    std::function<void(GncSummary &q, bool per_edge)> summary;   // of the last pass with that per_edge, read back (synchronises)
    std::function<void()> gradient;   // behind the point pass at CertState's X: g, |g|^2 into slot 0 of the partials
    std::function<void()> hessian;    // H_w at CertState's X into the factorisation's values
    std::function<void(double *s)> edge_s;   // m doubles: s_e as the last per-edge-writing pass left it (synchronises)
    double *wdev = nullptr;           // the weight array behind the pass, m doubles
    std::vector<int> in_R;            // per edge: in the robust set
    int num_robust = 0;               // |R|
    // Whether the pass at a failure must write per-edge output.  ml_gnc: yes -- chi2 per edge comes from a FULL pass only.
    // gnc: no -- every pass of it writes s_rot and s_trans, and the rows are of no use there.
    bool failure_per_edge = false;
    // Whether a stall at level 0 is evaluated (a pass at X with unit weights, whose sums and counts the result reports) or
    // returned as it is, those fields zero.  ml_gnc evaluates, gnc does not: both as they were written, kept.
    bool level0_stall_evaluated = false;
  };
  int gnc_loop(const char *who, const double *X, int ld, const GncOptions &o, const GncObjective &ob, double *Xout, int ldout,
               double *weights, double *log, int log_cap, GncResult &out, GncSummary *last = nullptr);
  // The loop of the Hessian modes (modes.cpp) on CertState's X, behind cov_begin.  What depends on the objective is launched by
  // the caller's hooks, each handed the anchor's own row: hessian -- H at X into the factorisation's values; trial -- F at the
  // trial point V into slot 2 of the certificate's partials
  struct ModesHooks {
    std::function<void(int)> hessian, trial;
  };
  int modes_loop(const double *X, int ld, int anchor, int k, const ModesOptions &o, long long max_bytes, const ModesHooks &hooks,
                 double *values, double *residuals, double *vectors, double *energy, double *X_escape, ModesResult &out);
  struct RobustState;   // the lists and buffers of the robust objective (robust.cpp), allocated by the first call that is not refused
  RobustState *rob_ = nullptr;
  void robust_release();
  int robust_begin(const Graph &g, const double *X, int ld, int loss, double loss_reg, int curvature, int anchor, const char *who,
                   const int *robust_set = nullptr);
  long long robust_remain() const;
  void robust_alloc();
  void robust_eval(const double *Xdev, int loss, double loss_reg, bool with_rows, int fslot);
  void robust_point(const double *X, int ld, int loss, double loss_reg, double *stationarity);   // null: no reduction, no wait
  void robust_hessian_launch(int arow, int curvature);
  void robust_summary(EdgeSummary *sum);
  // gnc.cpp: the buffers of the edge pass; the pass at a record array of the group (fslot as robust_eval), its summary read back
  void gnc_alloc();
  void gnc_pass(const double *Xdev, int kind, double mu, double c2, bool weigh, bool with_rows, int fslot);
  void gnc_summary(GncSummary &q);
  struct MlState;   // the lists and buffers of the maximum-likelihood objective (ml.cpp), allocated by the first call that is not refused
  MlState *ml_ = nullptr;
  void ml_release();
  int ml_begin(const Graph &g, const double *X, int ld, int anchor, const char *who);
  long long ml_remain() const;
  void ml_alloc();
  void ml_edge_pass(const double *Xdev, bool full, int fslot);   // fslot >= 0: F into that slot of the certificate's partial sums
  void ml_point(int arow, double *g, int slot_g2, int fslot);     // the full edge pass at CertState's X and the gather into g
  void ml_hessian_launch(int arow);
  double ml_stationarity(const double *X, int ld, int arow);   // X uploaded, the full edge pass and the gather: |g_ml| (ml_rely.cpp)
  // ml_gnc.cpp: the buffers of the weighted edge pass; the robust set of a call, uploaded (returns |R|); the pass at a record
  // array of the group (full: the per-edge arrays and summary [0], else summary [1]; fslot as ml_edge_pass); a summary read back
  void ml_gnc_alloc();
  int ml_gnc_set(const int *robust_set, std::vector<int> &in_R);
  void ml_gnc_pass(const double *Xdev, int kind, double mu, double c2, bool weigh, bool full, int fslot);
  void ml_gnc_summary(GncSummary &q, bool full);
  MargCache *marg_ = nullptr;   // the dense factors of joint_marginal, one per order (marg.cpp), allocated by the first call
  void marg_release();
  // the batches of a column plan behind a factorisation: Sigma_KK of the kept poses into g1 / g2 (device), d_prow <- their records
  int marg_sigma(const MargPlan &pl, const int *keep, int K, double *g1, double *g2, DevBuf<int> &d_prow, const char *who);
  // the refusal of the block solves with kb columns (pairs.cpp); own: the call's buffers
  int pairs_setup(long long max_bytes, HessPart own, int kb, HessAnalysis &out);
  // the batches of a plan behind a factorisation: joint (device, zeroed by the caller) <- the blocks of the pairs (pairs.cpp)
  int pairs_solve_joint(const PairsPlan &pl, int npairs, const int *d_prow, double *d_joint, const char *who);
  // the three blocks of nu listed edges behind a factorisation, by the selected inversion's gather map or by the batches
  // (rely.cpp; edge_reliability and ml_edge_reliability share it)
  int rely_joint(int use, const PairsPlan &pl, int nu, const std::vector<int> &prow, int arow, const int *d_prow, double *d_joint,
                 const char *who);
  // a graph checked against the group and its pattern; rec: its edge records in graph order, heads on unified own rows; eb:
  // the four blocks of every edge (robust.cpp; sens.cpp and rely.cpp too)
  int graph_records_own(const Graph &g, const char *who, std::vector<double> &rec, std::vector<int> *eb = nullptr);
  // what sensitivity and robust_sensitivity share (sens.cpp): the upstream checked and the sizes (returns the batch array's row
  // length, -1: error), and the batch loop, whose per-batch edge step is the caller's
  struct SensBatch {
    int b, c0, nc, kb;    // the batch, its first column, its columns, the row length of Xb
    const double *Xb;     // the solved columns (device)
  };
  int sens_begin(const char *who, const double *upstream, int ldu, int k, SensResult &out);
  int sens_batches(const char *who, int anchor, const double *upstream, int ldu, int k, double *adjoint,
                   const std::function<void(const SensBatch &)> &edge, SensResult &out);
  bool star_ = false;
  double *coll_send_ = nullptr, *coll_gathered_ = nullptr;
  AllGatherFn coll_allgather_ = nullptr;
  AllReduceFn coll_allreduce_ = nullptr;
  AllReduceDevFn coll_allreduce_dev_ = nullptr;
  DevBuf<double> star_vals_;   // AMM-PGO*: the master's four sums on the device (k_star_sums)
  void *coll_user_ = nullptr;
  double starF_ = 0, star_fobj_ = 0, star_fobjh_ = 0;
  int star_branches_ = 0;
  void node_rows_of_global(int a, const double *X, int ld, std::vector<double> &Z) const;
  // ---- iterate() (iterate.cpp)
  void half_step_product();   // amm(): T1_ = G [0 ; Xakh.R] + gx and the sum of Gkh, one pass
  // Gk <- the surrogate value G(X | g[k]) of the nodes of `set`, one pass and one read-back (nothing for an empty set);
  // into (optional, indexed by local node): the values go there instead of Gk
  void surrogate_at(const std::vector<int> &set, const double *X, double *into = nullptr);
  // Gk of the nodes of `set` at Xak, whose translations were just recovered with g: the refined ones are refined against g
  // (run_tnt), then the others are evaluated (surrogate_at)
  void refine_or_evaluate(const std::vector<int> &set, const double *g);
  // The per-call facts of one amm(), and its phases in their order
  struct AmmIter {
    const std::vector<int> &locals;
    NodeMask mask;                              // of locals
    std::vector<double> Gkh;                    // G(Xakh | g[k]) per local node
    std::vector<int> redo, restart, fb_x, fb_c; // the half step taken again; restarted; fallen back (g extrapolated / g[k])
    std::vector<char> g_is_current;             // a restart re-based the node's Xak on g[k]
    bool done_tnt = false, abandoned = false;   // the unasked refinement stood / was abandoned
  };
  void amm_head(const double *gam_dev, const NodeMask &mask);   // extrapolation, proximal half step, translation solve
  bool decide_refined(const std::vector<int> &locals);          // `refined` of every node; true: all of them are
  void refine_unasked(AmmIter &it);
  void refine_asked(AmmIter &it);
  void redo_half_step(AmmIter &it);
  void restart(AmmIter &it);
  void fall_back(AmmIter &it);
  bool prepare_extrapolated(const double *gam_dev = nullptr, int prox_slot = -1);   // Y, g_x, Df_x for the masked nodes (+ the proximal step)
  double global_objective(const double *X_own);           // F at the point whose own rows are X_own
  // the master's numbers in ONE read-back: F(X1) [, F(X2)] [, |X1 - ref|^2, |X2 - ref|^2] (null pointers: not wanted)
  int star_sums(const double *X1_own, const double *X2_own, const double *ref_own, double *F1, double *F2, double *d1, double *d2);
  static const int *star_slots();   // the six partial-sum slots star_sums() hands k_star_sums
  void enqueue_objective(const double *X_own, int slot0);   // k_cost partials of the point into slots slot0, slot0 + 1

  void upload_bsr(const std::vector<const BsrMatrix *> &per_node, bool rows_all, BsrBufs &out);
  void upload_operators();
  int refactor_tt();
  // Rescale::Dynamic (DPGOProblem.cpp:289-358, 426-514, 751-840): scale of every inter-node edge per node, the
  // counter of DPGOResult::rescale_count, the edge weights of the last evaluate_E
  std::vector<std::vector<double>> scale_;
  std::vector<int> rescale_count_;
  std::vector<int> e_off_;          // first inter edge of every node in E_
  DevBuf<double> e_w_;
  bool dynamic() const { return opt_.loss != 0 && opt_.rescale == 1; }
  // ... on the device (DPGO_RESCALE_HOST=1 keeps the host path: weights read back, operators re-assembled and uploaded):
  // the scales, counters and decisions live in device memory, the block-diagonal terms are rebuilt by k_rescale_apply
  // and G_tt is re-factored from values that never leave the GPU (SpdFactor::keep_numeric)
  bool device_rescale_ = false;
  DevBuf<double> e_scale_, Gbase_, Hbase_;
  DevBuf<int> rs_count_, rs_flags_, gpos_, att_pos_, e_off_dev_;
  double *h_rs_ = nullptr;   // pinned (same allocation as h_scal_): the rescale decision of every node
  std::vector<int> rescale_device(const std::vector<int> &set);   // after the decision arrived: apply + refactor; returns the rescaled nodes
  void setup_device_rescale();
  // decide per node whether its surrogate is rescaled (weights in e_w_), rebuild what changed; returns the nodes
  // that were rescaled
  std::vector<int> maybe_rescale(const std::vector<int> &set);
  void set_mask(const std::vector<int> &locals);
  void fetch(int nslots, bool all_rows);                  // -> h_scal_[local * MAX_SLOTS + s]
  void wait_flag(unsigned long long seq);   // the schedule's wait, then the verdicts that were enqueued in front of that flag
  int deferred_slots_ = 0;   // slots written earlier that ride along with the next fetch (saves a host round trip)
  // ... taken along by a reduction of nslots slots: how many it reduces.  Consumed once: by the first reduction after they were parked
  int take_deferred_slots(int nslots) { const int n = std::max(nslots, deferred_slots_); deferred_slots_ = 0; return n; }
  double scal(int local, int s) const { return h_scal_[local * MAX_SLOTS + s]; }
  double *h_upd_ = nullptr;   // pinned (same allocation): the sums update() ends with
  double uscal(int local, int s) const { return h_upd_[local * MAX_SLOTS + s]; }
  bool spec_refined_ = false; // amm(): every node of the group was refined in the last iteration (the next one starts its refinement unasked)
  void copy_rows(double *dst, const double *src, bool all_rows, int part = 0);
  // (a captured CG step launches over every node but takes the tile classes of the eager step's node sets: tnt.cpp, graph_step)
  const NodeBits *class_tt_ = nullptr, *class_rr_ = nullptr;
  void solve_tt(double *in, double *out, double scale);   // out.t <- scale * G_tt^-1 in.t
  void solve_rr(double *in, double *out, double scale);   // out.R <- scale * (G_RR + lambda I)^-1 in.R
  // the context of this group's launches (kernels.h) over the nodes of m / of cur_mask_
  LaunchCtx lc(const NodeMask &m) const { return {d_, st_, T_, m}; }
  LaunchCtx lc() const { return lc(cur_mask_); }
  TcolOp g_tcol() const { return {G_.dev, G_.tcol.p}; }   // G's translation column: y = base + G_{:,t} xt.t (launch_bsr_tcol*)
  void recover_translations(double *X, const double *g);  // X.t = -Gtt^-1 (g_t + G_tR X.R) for masked nodes
  void eval_G(const double *X, const double *g, int slot);
  unsigned long long fetch_async(int nslots, bool all_rows);
  int amm(const std::vector<int> &locals);
  int mm(const std::vector<int> &locals);
  // refine X in place (TNT on G(. | g)); sets Gk = G(X | g) and, with g_alt, Gk_alt = G(X | g_alt)
  // base_ready: X.t was just recovered from X.R with this g (recover_translations) and T1_ still holds that product
  // confirm (optional): called once the start of the refinement is enqueued -- the caller's chance to take a read-back
  // that decides whether these nodes are refined at all; false: the refinement is abandoned (returns false; what was
  // enqueued only touched work vectors, and T1_)
  bool run_tnt(const std::vector<int> &locals, double *X, const double *g, const double *g_alt = nullptr,
               bool base_ready = false, const std::function<bool()> *confirm = nullptr);
  struct TntRun;   // the state and the phases of one run_tnt() call (tnt.cpp)
};

}  // namespace dpgo
