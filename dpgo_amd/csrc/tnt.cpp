// Riemannian truncated-Newton trust-region refinement on device vectors,
// batched over the nodes of a group.
//
// Same algorithm as the reference's generic solvers
//   TNT    C++/Optimization/include/Optimization/Riemannian/TNT.h:242-693
//   STPCG  C++/Optimization/include/Optimization/LinearAlgebra/IterativeSolvers.h:166-426
// instantiated the way DPGOHash does (C++/DPGO/src/DPGOHash.cpp:270-349):
//   f(Y)        = G(Y | g, f)                       DPGOProblem.cpp:180-205
//   grad        = Proj_R(g_R + (G Y)_R)             DPGOProblem.h:380-406
//   Hess[Rdot]  = Proj_R(G_Rt tdot + G_RR Rdot - SBD(Rdot, R, nabla)), tdot = -G_tt^-1 G_tR Rdot
//                                                   DPGOProblem.cpp:552-577
//   precon      = Proj_R((G_RR + lambda I)^-1 v)    DPGOProblem.cpp:579-598
//   retraction  = [ -G_tt^-1(g_t + G_tR R+) ; R+ = proj(R + V) ]   DPGOProblem.cpp:127-143
//   metric      = sum V1 .* V2                      DPGOHash.cpp:307-310
//
// Every node runs the reference's control flow with its OWN scalars (step
// lengths, trust-region radius, stopping tests); the nodes advance in lockstep so
// that one launch serves all of them.  Per-node step lengths and the set of nodes
// a launch works on travel as kernel arguments (NodeCoefs, NodeMask: no uploads),
// and the handful of reductions per CG step come back through one polled read-back.
//
// One call of run_tnt() is one TntRun: the state of the refinement, the launch helpers, the host's scalar logic (no launch in
// it) and the phases -- the first round, started on the device or on the host; later rounds, started on the host; the rest
// of a round, which both kinds share; the publishing of the results.  run_tnt() drives them.
//
// Segment bodies (the lambdas handed to segment()) only LAUNCH: a replay does not run the body, so every piece of host state
// that the host reads afterwards -- the masks mA, mB, cur_mask_, the flags' sequence numbers -- is set by the caller when
// segment() has returned.  (The one thing a body does beside launching is to hand update()'s lazy reduction to
// k_cg_scal_begin, scal_begin(): that happens only where the body runs eagerly -- never under capture --, so a replay has
// nothing to miss.)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "group.h"

namespace dpgo {

namespace {
enum { ST_GRADIENT = 0, ST_PRECON_GRADIENT, ST_REL_DECREASE, ST_STEPSIZE, ST_TRUST_REGION, ST_ITER_LIMIT };

struct NodeTnt {
  bool active = true;       // outer trust-region loop still running
  int status = ST_ITER_LIMIT;
  double fx = 0, gnorm = 0, pgnorm = 0, Delta = TntConst::Delta0;
  int iteration = 0, accepted = 0, inner_total = 0;
  // STPCG state (IterativeSolvers.h:207-283)
  bool cg = false;
  double sk_M_pk = 0, sk_M_2 = 0, pk_M_2 = 0, rv = 0, Delta_2 = 0, target = 0, h_M_norm = 0;
  int cg_it = 0;
};

// what a segment's key must hold beside the rotating buffers (segment()): the vectors of this call and its variant
unsigned long long K(const void *q) { return (unsigned long long)(uintptr_t)q; }
}  // namespace

struct Group::TntRun {
  static constexpr int NSUM = 6;   // the sums a trial point needs (TNT.h:505-536)
  Group &G;
  const Options &o;
  const int L;
  // ---- the call's arguments.  X and xprop change: an accepted step of the whole group swaps Xak_ with tmp_[7], and a
  // segment's key takes K(X) as of the time of use
  const std::vector<int> &nodes;
  double *X;
  const double *const g, *const ga;
  const bool base_ready;
  const std::function<bool()> *const confirm;
  const bool jacobi, use_precon;
  // hh accumulates H s_k alongside s_k (every step s_k += c p_k is mirrored by hh += c H p_k), so the
  // predicted decrease needs no extra Hessian-vector product: same value as Hess(x, h) of TNT.h:514-515
  // up to rounding of the CG recurrence.
  double *const nabla, *const grad, *const sk, *const rk, *const vk, *const pk, *const Hp, *xprop, *const w1, *const pg,
         *const hh, *const w3, *const nprop;
  const unsigned long long kg, kga, kvar;
  const bool use_graph;
  // The first trust-region iteration starts without a host round trip: the norms, the gradient tests and the start
  // values of the CG are taken on the device (k_tnt_begin); the host reads the same sums at its first wait.
  const bool device_start;
  // In the early regime every node ends its first CG step on the trust-region boundary, so -- as long as that was the case
  // the last time -- the trial point of the nodes whose CG is over (dmask[2]) is enqueued right behind that step and ONE
  // wait brings the norms, the CG summary and the trial point's sums.  Otherwise the step is awaited at once.
  const bool spec;
  // ---- per node: the trust-region state; rv0 = <grad, P grad> (the first CG scalar); lin / lin_alt = <X, g> / <X, g_alt>,
  // which let the caller re-base f on g_alt without another G X
  std::vector<NodeTnt> S;
  std::vector<double> rv0, lin, lin_alt;
  // ---- what sizes the launches.  by value: the nodes the host last saw iterating (the solves shrink their grids with it);
  // by pointer: the device's own, more recent masks
  NodeBits bitsA = 0;
  NodeMask mA = ALL_NODES, mB = ALL_NODES;
  // ---- the round under way: its candidates, the sums of their trial points, who has had one, who accepted, who needs a
  // new model
  std::vector<int> A, acc, requad;
  std::vector<double> tsum;
  std::vector<char> tried;
  int tr_rounds = 0;
  // ---- the flags of the first step's scalars and of the first round's last launch
  unsigned long long seqA = 0, seq_first = 0;

  TntRun(Group &grp, const std::vector<int> &nodes_, double *X_, const double *g_, const double *ga_, bool base_ready_,
         const std::function<bool()> *confirm_);

  // launch helpers
  bool quad_model(const double *Y, bool from_base);
  void precon_with_sums(const double *Y, const double *v, double *out);
  void norms_enqueue(bool with_f, bool have_sums);
  void norms(const std::vector<int> &set, bool with_f, bool have_sums);
  void enqueue_trial(NodeMask m, bool retracted, int nslots, bool with_reduce = true);
  void scal_begin(const TntStart &start);
  void step_a(bool first, bool retract = false, const TntStart *begin = nullptr);
  void step_b();
  void graph_step();
  // host logic (no launch)
  void norms_take(int a, bool with_f, double g2, double xn, double xg, double xga, double pg2, double gpg);
  void norms_read(const std::vector<int> &set, bool with_f);
  double cgs(int a, int k) const { return G.h_cg_[a * CG_SUMMARY + k]; }
  // The nodes still iterating after scalar step `w` of this run (phase 0 / 1 of step j: 2 j - 1 / 2 j).  The summary of a
  // later step may already have overwritten the one waited for; it carries the ordinal each node stopped at (kernels.h,
  // CG_LIVE_ORD), so the answer -- and with it the node sets and tile classes of the next launches -- is the same however
  // late the host comes.
  bool live_after(int a, int w) const { return cgs(a, 0) > (double)w; }
  bool any_live(int w);
  bool select_candidates(bool host_gradient_tests);
  void read_device_verdicts();
  void take_first_step_trials();
  void judge(int a, const double *t);
  void publish();
  // phases
  void enqueue_device_start(int nslots, bool plan_spec);
  bool first_round_device();
  bool first_round_host();
  void begin_round();
  void later_round();
  void host_cg_start();
  void finish_round(bool more_steps, bool unasked);
  void finish_cg(bool more_steps);
  void remaining_cg_steps();
  void trial_of_rest();
  void accept_steps(bool unasked);
};

Group::TntRun::TntRun(Group &grp, const std::vector<int> &nodes_, double *X_, const double *g_, const double *ga_,
                      bool base_ready_, const std::function<bool()> *confirm_)
    : G(grp), o(grp.opt_), L(grp.num_local()), nodes(nodes_), X(X_), g(g_), ga(ga_), base_ready(base_ready_), confirm(confirm_),
      jacobi((o.preconditioner == 1) && grp.jacobi_.n > 0),                     // Preconditioner::Jacobi
      use_precon(jacobi || ((o.preconditioner == 3) && grp.Lrr_.F.n > 0)),      // ... or RegularizedCholesky
      nabla(grp.tmp_[0].p), grad(grp.tmp_[1].p), sk(grp.tmp_[2].p), rk(grp.tmp_[3].p), vk(grp.tmp_[4].p), pk(grp.tmp_[5].p),
      Hp(grp.tmp_[6].p), xprop(grp.tmp_[7].p), w1(grp.tmp_[8].p), pg(grp.tmp_[10].p), hh(grp.tmp_[11].p), w3(grp.tmp_[12].p),
      nprop(grp.tmp_[13].p), kg(K(g_)), kga(K(ga_)),
      kvar((use_precon ? 1ull : 0ull) | (jacobi ? 2ull : 0ull) | (base_ready_ ? 4ull : 0ull)),
      use_graph(grp.sched_.cg_graph_wanted()), device_start(o.max_iterations > 0 && o.max_iterations_accepted > 0),
      spec(device_start && grp.tnt_speculate_), S(L), rv0(L, 0.0), lin(L, 0.0), lin_alt(L, 0.0), tsum((size_t)L * NSUM, 0.0),
      tried(L, 0) {
  for (auto &s : S) s.active = false;
  for (int a : nodes) S[a] = NodeTnt();
}

// ---------------------------------------------------------------------------------------------------------------------
// launch helpers
// ---------------------------------------------------------------------------------------------------------------------

// nabla = G Y + g and grad = Proj_Y(nabla) (rotation rows).  from_base: Y.t was just recovered from Y.R with
// this g (recover_translations), so T1_ = G [0 ; Y.R] + g is there and only the translation column is missing.
// Returns true when the pass also left the four sums of the refinement's start (|grad|^2, <Y, nabla>, <Y, g>,
// <Y, g_alt>) in the partial slots 0..3 (its epilogue), so that no separate pass over the vectors is needed.
bool Group::TntRun::quad_model(const double *Y, bool from_base) {
  if (from_base) {
    // nabla, grad and the sums in one pass
    launch_bsr_tcol_begin(G.lc(), G.g_tcol(),
                          {.xt = Y, .base = G.T1_.p, .y = nabla, .X = Y, .grad = grad, .partials = G.partials_.p, .g = g, .ga = ga});
    return true;
  }
  launch_bsr(G.lc(), G.G_.dev, {.x = Y, .addv = g, .y = nabla});
  launch_tangent_rot(G.lc(), {.X = Y, .in = nabla, .out = grad});
  return false;
}

// out = P(v) = Proj_Y(M^-1 v) with |out|^2 and <v, out> in the partial slots MAX_DOTS, MAX_DOTS + 1, and -out in pk
// (the first CG direction); only called with a preconditioner
void Group::TntRun::precon_with_sums(const double *Y, const double *v, double *out) {
  if (jacobi) launch_rot_rowscale(G.lc(), G.jacobi_.p, v, w1);
  else G.solve_rr(const_cast<double *>(v), w1, 1.0);   // w1.R = (G_RR + lambda I)^-1 v.R; the forward sweep only reads v
  launch_tangent_rot(G.lc(), {.X = Y, .in = w1, .out = out, .dotv = v, .partials = G.partials_.p, .slot = MAX_DOTS, .two = true,
                              .neg = pk});
}

// The dot products (partial slots 0..3 and MAX_DOTS, MAX_DOTS + 1) behind gnorm, pgnorm, rv0 and -- with_f -- f(X | g),
// from the model gradient nabla = G X + g that is there anyway:
//   f = <X, g> + 1/2 <X, G X> = 1/2 (<X, nabla> + <X, g>)      (DPGOProblem.cpp:180-205)
// and the first CG direction pk = -P(grad); who reduces the sums is the caller's choice: k_reduce + wait (norms) or
// k_tnt_begin (no wait).  have_sums: slots 0..3 were already left there by quad_model's epilogue
void Group::TntRun::norms_enqueue(bool with_f, bool have_sums) {
  if (!have_sums) {
    const double *pa[MAX_DOTS] = {grad, X, X, X}, *pb[MAX_DOTS] = {grad, nabla, g, ga};
    const int parts[MAX_DOTS] = {2, 0, 0, 0, 0, 0};
    launch_dots(G.lc(), with_f ? 4 : 1, pa, pb, parts, G.partials_.p, 0);
  }
  if (use_precon) precon_with_sums(X, grad, pg);
  else launch_cg_init(G.lc(), grad, grad, nullptr, nullptr, nullptr, nullptr, pk);
}

// ... of the nodes in `set` (mask == set), reduced and awaited
void Group::TntRun::norms(const std::vector<int> &set, bool with_f, bool have_sums) {
  norms_enqueue(with_f, have_sums);
  G.fetch(MAX_DOTS + 2, false);
  for (int a : set)
    norms_take(a, with_f, G.scal(a, 0), G.scal(a, 1), G.scal(a, 2), G.scal(a, 3), G.scal(a, MAX_DOTS), G.scal(a, MAX_DOTS + 1));
}

// trial point of the nodes in `m`: x+ = retract(x, s), f(x+) and, for an accepted step, the next model gradient
// retracted: the rotations of x+ are there already (the CG step's vector update took them along, step_a)
void Group::TntRun::enqueue_trial(NodeMask m, bool retracted, int nslots, bool with_reduce) {
  G.cur_mask_ = m;
  if (!retracted) launch_retract_rot(G.lc(), X, sk, xprop);
  G.recover_translations(xprop, g);
  // nprop = G xprop + g: gives f(xprop) and, if accepted, the next model; its epilogue leaves the six sums
  // <s,s>, <grad,s>, <s,Hs>, <x+,g>, <x+,g_alt>, <x+,nprop> in the partial slots 0..5
  launch_bsr_tcol(G.lc(), G.g_tcol(),
                  {.xt = xprop, .base = G.T1_.p, .y = nprop, .partials = G.partials_.p, .g = g, .ga = ga, .s = sk, .grad = grad, .hs = hh});
  // (with_reduce = false: the caller launches the reduction itself, with the gate of a speculative update: group.h)
  if (with_reduce) launch_reduce(G.st_, G.T_, L, false, nslots, G.partials_.p, G.h_scal_, G.sched_.flag());
}

// The start of the refinement -- the norms, the gradient tests, the CG's start values (k_tnt_begin) -- riding with the first
// step's scalar kernel (k_cg_scal_begin), and with it update()'s reduction, if it is still waiting for somebody to take it
// along (group.h, UpdLazy)
void Group::TntRun::scal_begin(const TntStart &start) {
  const int carry = (G.upd_lazy_.pending && !G.sched_.capturing()) ? G.upd_lazy_.nslots : 0;
  launch_cg_scal_begin(G.st_, G.T_, start, G.h_cg_, G.sched_.flag(), G.dev_tnt_.p, carry, G.h_upd_);
  if (carry) { G.upd_lazy_.pending = false; G.pending_seq_ = G.sched_.last_seq(); }
}

// ---- STPCG (IterativeSolvers.h:207-426).  The scalar recurrences (alpha, beta, the boundary / negative
// curvature / kernel tests, the stopping test) run on the device (k_cg_scal); the vector kernels take their
// step lengths and the set of still-iterating nodes from device memory, so a whole CG step is enqueued
// without a host round trip.  The host only polls the summary (live, |h|_M, iterations) of a step it enqueued
// earlier: step i+1 is already queued when the outcome of step i arrives; once every node has stopped, the
// kernels of the surplus step find an empty device mask and return at once.
//
// First half of a step: H p and its four scalars, then the step-length logic (:296-362)
// first: the first step of a run -- s_0 = 0, H s_0 = 0, r_0 = grad are not materialised, the step takes them as given, and
// it runs for every node of the run, live or not: a node that stops before its first step has c1 = 0 and gets its
// s = H s = 0 written here
// retract: the nodes whose CG ends with this step (dmask[2]) get the rotations of their trial point from the vector
// update (k_cg_step) instead of a launch of their own.  begin: the start of the refinement has not been taken yet and rides
// with this step's scalar kernel (scal_begin): the product then runs for every candidate, and leaves its sums where the
// refinement's are not
void Group::TntRun::step_a(bool first, bool retract, const TntStart *begin) {
  G.cur_mask_ = begin ? G.live_mask(bitsA, nullptr) : mA;
  launch_bsr(G.lc(), G.G_.dev, {.x = pk, .mode = BsrMode::NoTrans, .y = w1});   // G [0 ; p.R]
  G.solve_tt(w1, w3, -1.0);
  double *sums = G.partials_.p + (begin ? (size_t)cg_first_slot() * G.T_.nseg_all : 0);
  // Hp and <p,Hp>, <Hp,Hp>, <p,p>, <p,r>
  launch_bsr_tcol_hess(G.lc(), G.g_tcol(),
                       {.xt = w3, .base = w1, .X = X, .nabla = nabla, .p = pk, .Hp = Hp, .r = first ? grad : rk, .partials = sums});
  // the step-length logic
  if (begin) scal_begin(*begin);
  else launch_cg_scal(G.st_, G.T_, L, 0, G.partials_.p, G.cg_.p, G.dmask_.p, G.h_cg_, G.sched_.flag());
  // s += c1 p, H s += c1 H p for every node of the step (a node that stops here takes its boundary step), r += alpha H p
  // for those that go on
  CgStepArgs step = {.cg = G.cg_.p, .p = pk, .Hp = Hp, .s = sk, .hs = hh, .r = rk, .r0 = first ? grad : nullptr};
  if (retract) { step.X = X; step.xprop = xprop; step.rmask = G.dmask_.p + 2; }
  launch_cg_step(G.lc(first ? NodeMask{bitsA, nullptr} : mA), step);
}

// second half: preconditioner; beta and the recurrences, next stopping test (:364-390, :285-291)
void Group::TntRun::step_b() {
  G.cur_mask_ = mB;
  if (use_precon) {
    if (jacobi) launch_rot_rowscale(G.lc(), G.jacobi_.p, rk, w1);
    else G.solve_rr(rk, w1, 1.0);
    launch_tangent_rot(G.lc(), {.X = X, .in = w1, .out = vk, .dotv = rk, .partials = G.partials_.p});   // v = Proj(M^-1 r) and <r, v>
  } else {
    G.copy_rows(vk, rk, false, 0);
    const double *pa[MAX_DOTS] = {rk}, *pb[MAX_DOTS] = {vk};
    const int P2[MAX_DOTS] = {2, 2, 2, 2, 2, 2};
    launch_dots(G.lc(), 1, pa, pb, P2, G.partials_.p, 0);
  }
  launch_cg_scal(G.st_, G.T_, L, 1, G.partials_.p, G.cg_.p, G.dmask_.p, G.h_cg_, G.sched_.flag());
  launch_cg_dir(G.lc(), G.cg_.p, vk, pk);
}

// One whole step (A then B, not the first) as ONE submission: captured once per set of argument values, replayed ever
// after.  The by-value node sets of a replay are the group's nodes -- the device's own masks keep the nodes that are
// not (or no longer) part of the CG out, as they do for a node that stopped since the host last looked.
void Group::TntRun::graph_step() {
  const NodeBits all = G.all_bits();
  const NodeMask sA = mA, sB = mB;
  // (the roots' tile classes are the eager step's: they are part of the arithmetic, and so of the key)
  const unsigned long long cls = (G.Ltt_.fine_root_for(sA.v) ? 1ull : 0ull) | (use_precon && !jacobi && G.Lrr_.fine_root_for(sB.v) ? 2ull : 0ull);
  G.segment(21, all, {K(X), kvar, cls}, [&] {
    mA = NodeMask{all, G.dmask_.p};
    mB = NodeMask{all, G.dmask_.p + 1};
    struct Classes {
      Group *g;
      ~Classes() { g->class_tt_ = g->class_rr_ = nullptr; }
    } classes{&G};
    G.class_tt_ = &sA.v;
    G.class_rr_ = &sB.v;
    step_a(false);
    step_b();
  }, 1);
  mA = sA; mB = sB;   // (the launches of the body were sized for the whole group: the host's own sets again)
}

// ---------------------------------------------------------------------------------------------------------------------
// host logic: no launch in any of these
// ---------------------------------------------------------------------------------------------------------------------

void Group::TntRun::norms_take(int a, bool with_f, double g2, double xn, double xg, double xga, double pg2, double gpg) {
  S[a].gnorm = S[a].pgnorm = std::sqrt(g2);
  rv0[a] = g2;
  if (use_precon) {
    S[a].pgnorm = std::sqrt(pg2);
    rv0[a] = gpg;
  }
  if (with_f) {
    S[a].fx = 0.5 * (xn + xg) + G.res_[a].f;
    lin[a] = xg;
    lin_alt[a] = xga;
  }
}

// ... from the pinned summary of k_tnt_begin
void Group::TntRun::norms_read(const std::vector<int> &set, bool with_f) {
  for (int a : set) {
    const double *t = G.h_tnt_ + a * TNT_SUMMARY;
    norms_take(a, with_f, t[0], t[1], t[2], t[3], t[4], t[5]);
  }
}

// (sets the masks of the next launches to the live nodes; few live nodes: the own-segment launches cover them alone)
bool Group::TntRun::any_live(int w) {
  NodeBits live = 0;
  for (int a : A)
    if (live_after(a, w)) live |= 1ull << a;
  mA = G.live_mask(live, G.dmask_.p);
  mB = G.live_mask(live, G.dmask_.p + 1);
  return live != 0;
}

// A <- the nodes that start another trust-region iteration (TNT.h:446-484).  host_gradient_tests = false: the gradient
// tests are the device's (k_tnt_begin), and A holds the candidates until the host has seen its summary (read_device_verdicts)
bool Group::TntRun::select_candidates(bool host_gradient_tests) {
  A.clear();
  for (int a : nodes) {
    NodeTnt &s = S[a];
    if (!s.active) continue;
    if (!(s.iteration < o.max_iterations && s.accepted < o.max_iterations_accepted)) { s.active = false; continue; }
    if (host_gradient_tests) {
      if (s.gnorm < o.grad_norm_tol) { s.status = ST_GRADIENT; s.active = false; continue; }
      if (s.pgnorm < o.preconditioned_grad_norm_tol) { s.status = ST_PRECON_GRADIENT; s.active = false; continue; }
    }
    A.push_back(a);
  }
  return !A.empty();
}

// the sums k_tnt_begin reduced, and its verdict on the gradient tests: A <- the candidates that passed them
void Group::TntRun::read_device_verdicts() {
  norms_read(A, true);
  std::vector<int> act;
  for (int a : A) {
    if (G.h_tnt_[a * TNT_SUMMARY + 6] != 0.0) { act.push_back(a); continue; }
    S[a].status = S[a].gnorm < o.grad_norm_tol ? ST_GRADIENT : ST_PRECON_GRADIENT;
    S[a].active = false;
  }
  A.swap(act);
}

// a node whose CG ended with (or before) the first step: the sums just read are its trial point's (enqueued unasked)
void Group::TntRun::take_first_step_trials() {
  for (int a : A)
    if (!live_after(a, 1)) {
      tried[a] = 1;
      for (int q = 0; q < NSUM; q++) tsum[(size_t)a * NSUM + q] = G.scal(a, q);
      S[a].h_M_norm = cgs(a, 1);
      S[a].cg_it = (int)cgs(a, 2);
    }
}

// acceptance test and trust-region update of node a from the sums of its trial point (TNT.h:537-607)
void Group::TntRun::judge(int a, const double *t) {
  NodeTnt &s = S[a];
  const double fx_prop = 0.5 * (t[5] + t[3]) + G.res_[a].f;
  const double h_norm = std::sqrt(t[0]);
  const double dm = -t[1] - 0.5 * t[2];
  const double df = s.fx - fx_prop;
  const double rel_dec = df / (TntConst::sqrt_eps() + std::fabs(s.fx));
  const double rho = df / dm;
  const bool ok = (!std::isnan(rho)) && rho > TntConst::eta1;
  s.accepted += ok;
  bool stop = false;
  if (ok) {
    acc.push_back(a);
    s.fx = fx_prop;
    lin[a] = t[3];
    lin_alt[a] = t[4];
    if (rel_dec < o.rel_func_decrease_tol) { s.status = ST_REL_DECREASE; stop = true; }
    else if (h_norm < o.stepsize_tol) { s.status = ST_STEPSIZE; stop = true; }
    else if (s.iteration + 1 < o.max_iterations && s.accepted < o.max_iterations_accepted)
      requad.push_back(a);   // the new model is only needed if another iteration follows (TNT.h:446-449)
  }
  if (!stop) {   // trust-region update (TNT.h:593-607)
    if ((!std::isnan(rho)) && rho >= TntConst::eta2) s.Delta = std::max(TntConst::alpha2 * s.h_M_norm, s.Delta);
    else if (std::isnan(rho) || rho < TntConst::eta1) {
      s.Delta = TntConst::alpha1 * s.h_M_norm;
      if (s.Delta < TntConst::Delta_tol) { s.status = ST_TRUST_REGION; stop = true; }
    }
  }
  if (stop) s.active = false;
  else s.iteration++;
}

// Gk, Gk_alt, tnt_status, tnt_inner of the nodes (and, verbose, a line each)
void Group::TntRun::publish() {
  if (o.verbose) {
    static const char *names[] = {"gradient", "preconditioned gradient", "relative decrease", "step size", "trust region", "iteration limit"};
    for (int a : nodes)
      printf("[dpgo_amd] node %d TNT: f = %.12e, |grad| = %.3e, %d iteration(s), %d accepted, %d CG step(s), Delta = %.3e, stop: %s\n",
             G.nodes_[a], S[a].fx + 0.0, S[a].gnorm, S[a].iteration, S[a].accepted, S[a].inner_total, S[a].Delta, names[S[a].status]);
    fflush(stdout);
  }
  for (int a : nodes) {
    G.res_[a].Gk = S[a].fx;
    G.res_[a].Gk_alt = S[a].fx - lin[a] + lin_alt[a];   // f(X | g_alt): only the linear term depends on g
    G.res_[a].tnt_status = S[a].status;
    G.res_[a].tnt_inner = S[a].inner_total;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// phases
// ---------------------------------------------------------------------------------------------------------------------

// Everything from the model gradient to the first wait is branch-free: ONE segment (a replay where the host's launch
// rate would bound it).  Every node of `nodes` is a candidate (the iteration limits allow a first iteration), the radii
// are TntConst::Delta0.  With `spec` the trial point of the nodes whose CG ends at step 1 follows unasked.
void Group::TntRun::enqueue_device_start(int nslots, bool plan_spec) {
  const NodeBits bits_nodes = bitsA;
  // (the radii travel by value: part of the key.  run_tnt() starts every node at Delta0; debug_stpcg() takes them as given)
  unsigned long long kdelta = 1469598103934665603ull;
  for (int a : nodes) {
    unsigned long long w;
    static_assert(sizeof(w) == sizeof(double), "");
    std::memcpy(&w, &S[a].Delta, sizeof(w));
    kdelta = (kdelta ^ w) * 1099511628211ull;
  }
  G.segment(20, bits_nodes, {K(X), kg, kga, kvar, spec ? 1ull : 0ull, (unsigned long long)nslots, plan_spec ? 1ull : 0ull, kdelta}, [&] {
    G.cur_mask_ = G.live_mask(bits_nodes, nullptr);
    const bool have_sums = quad_model(X, base_ready);
    norms_enqueue(true, have_sums);
    std::vector<double> Delta(L, 0.0);
    for (int a : nodes) Delta[a] = S[a].Delta;
    const TntStart start = {.nnodes = L, .bits = bitsA, .use_precon = use_precon, .max_it = o.max_tCG_iterations,
                            .grad_tol = o.grad_norm_tol, .pgrad_tol = o.preconditioned_grad_norm_tol, .kappa = o.STPCG_kappa,
                            .theta = o.STPCG_theta, .Delta = Delta.data(), .partials = G.partials_.p, .cg = G.cg_.p, .dmask = G.dmask_.p,
                            .host_tnt = G.h_tnt_};
    const bool merged = G.fused_;   // the start rides on the first step's scalar kernel
    if (!merged) launch_tnt_begin(G.st_, G.T_, start);
    mA = G.live_mask(bitsA, G.dmask_.p);
    mB = G.live_mask(bitsA, G.dmask_.p + 1);
    step_a(true, spec && G.fused_, merged ? &start : nullptr);
    if (spec) enqueue_trial(NodeMask{bitsA, G.dmask_.p + 2}, G.fused_, nslots, !plan_spec);
  });
  mA = G.live_mask(bitsA, G.dmask_.p);   // (a replay does not run the body: the host's copies)
  mB = G.live_mask(bitsA, G.dmask_.p + 1);
  G.cur_mask_ = G.live_mask(bits_nodes, nullptr);
}

// The first round, started on the device; false: the caller's `confirm` said no
bool Group::TntRun::first_round_device() {
  bitsA = G.cur_mask_.v;   // (of `nodes`)
  const int nslots = spec ? G.take_deferred_slots(NSUM) : 0;
  // where every node of the group is in here and the trial point follows unasked, the update() that the common outcome
  // leads to goes out as well, under a gate that takes the decision on the device (group.h: SpecUpdate); the trial point's
  // reduction then waits for the gate's inputs (below)
  const bool plan_spec = confirm && spec && G.fused_ && (int)nodes.size() == L && base_ready && X == G.Xak_.p && G.spec_update_possible(xprop);
  enqueue_device_start(nslots, plan_spec);
  seq_first = G.sched_.last_seq();   // (the flag of the last launch of the segment: the trial point's reduction, or the first step's scalars)
  // the caller's read-back (the scalars that decide whether these nodes are refined at all) is taken NOW, with the start
  // of the refinement already on the GPU: the stream never waits for that decision
  if (confirm && !(*confirm)()) return false;
  if (plan_spec) {
    seqA = seq_first;                        // (the first step's scalars: the segment's last flag)
    G.speculate_update(xprop, nslots);       // the trial point's reduction with the gate, then the continuation
    seq_first = G.spec_upd_.seq_trial;
  } else seqA = seq_first - (spec ? 1 : 0);
  if (!select_candidates(false)) return true;
  begin_round();
  G.wait_flag(spec ? seq_first : seqA);   // (spec: the trial point's reduction -- everything before it is there too)
  read_device_verdicts();
  if (spec) take_first_step_trials();
  const bool more_steps = any_live(1);
  G.tnt_speculate_ = !more_steps;   // speculate next time if nobody needed a second step this time
  finish_round(more_steps, spec);
  return true;
}

// The first "round" where the iteration limits allow none (device_start is false: no node passes select_candidates): the
// norms and f of the starting point are all there is to take.  false: the caller's `confirm` said no
bool Group::TntRun::first_round_host() {
  G.sched_.flush_deferred();   // (launches that were waiting for this refinement's first segment: there is none on this path)
  if (confirm && !(*confirm)()) return false;
  const bool have_sums = quad_model(X, base_ready);
  norms(nodes, true, have_sums);
  return true;
}

void Group::TntRun::begin_round() {
  tr_rounds++;
  if (tr_rounds > 1) G.tnt_common_ = false;   // (a further round: not the common course)
  std::fill(tsum.begin(), tsum.end(), 0.0);
  std::fill(tried.begin(), tried.end(), 0);
}

// A later round of the candidates A, started on the host from the norms it has read (norms)
void Group::TntRun::later_round() {
  begin_round();
  host_cg_start();
  finish_round(any_live(1), false);
}

// The CG of the candidates A started on the host: its start values from the norms read back, and its first step, awaited
void Group::TntRun::host_cg_start() {
  G.set_mask(A);
  bitsA = G.cur_mask_.v;
  // p_0 = -v_0, v_0 = P(grad): a node whose step was rejected starts from the same gradient (pk was overwritten), one whose
  // step was accepted from the one norms() has just taken
  launch_cg_init(G.lc(), grad, use_precon ? pg : grad, nullptr, nullptr, nullptr, nullptr, pk);
  CgStart cs;
  for (int a = 0; a < L; a++) cs.rv[a] = cs.Delta[a] = cs.target[a] = 0.0;
  for (int a : A) {
    cs.rv[a] = rv0[a];   // <r_0, v_0> = <grad, P grad>, read back together with the norms
    cs.Delta[a] = S[a].Delta;
    const double r0 = std::sqrt(rv0[a]);
    cs.target[a] = r0 * std::min(o.STPCG_kappa, std::pow(r0, o.STPCG_theta));
  }
  launch_cg_begin(G.st_, L, bitsA, cs, o.max_tCG_iterations, G.cg_.p, G.dmask_.p);
  mA = G.live_mask(bitsA, G.dmask_.p);
  mB = G.live_mask(bitsA, G.dmask_.p + 1);
  step_a(true);
  seqA = G.sched_.last_seq();
  G.wait_flag(seqA);
}

// What both kinds of round share once the first CG step is in: the remaining steps (finish_cg); then the trial points of the
// nodes that have not had theirs, the acceptance tests, the accepted steps and the new models.  unasked: the first step's
// trial points were enqueued behind it without waiting (spec)
void Group::TntRun::finish_round(bool more_steps, bool unasked) {
  finish_cg(more_steps);
  trial_of_rest();
  acc.clear();
  requad.clear();
  for (int a : A) judge(a, &tsum[(size_t)a * NSUM]);
  accept_steps(unasked);
  if (!requad.empty()) {
    G.set_mask(requad);
    G.copy_rows(nabla, nprop, false, 0);   // the model gradient at the accepted point
    launch_tangent_rot(G.lc(), {.X = X, .in = nabla, .out = grad});
    norms(requad, false, false);
  }
}

// ... where the CG ends: the steps after the first, and what the host keeps of every candidate's CG
void Group::TntRun::finish_cg(bool more_steps) {
  if (more_steps) remaining_cg_steps();
  for (int a : A) {
    if (!tried[a]) {
      S[a].h_M_norm = cgs(a, 1);
      S[a].cg_it = (int)cgs(a, 2);
    }
    S[a].cg = false;
    S[a].inner_total += S[a].cg_it;
  }
}

// steps 2, 3, ...: step i+1 is enqueued before the host waits for the outcome of step i
void Group::TntRun::remaining_cg_steps() {
  step_b();
  unsigned long long seqB = G.sched_.last_seq();
  for (int w = 2;; w += 2) {
    if (use_graph) graph_step();
    else { step_a(false); step_b(); }
    const unsigned long long next = G.sched_.last_seq();
    G.wait_flag(seqB);   // the outcome of the step before the one just enqueued (its phase 1: scalar step w)
    if (!any_live(w)) break;
    seqB = next;
  }
}

// trial point (TNT.h:505-536) of the nodes that have not had theirs
void Group::TntRun::trial_of_rest() {
  std::vector<int> rest;
  for (int a : A)
    if (!tried[a]) rest.push_back(a);
  if (rest.empty()) return;
  G.set_mask(rest);
  const NodeMask mrest = G.cur_mask_;
  const int nslots = G.take_deferred_slots(NSUM);
  G.segment(22, mrest.v, {K(X), kg, kga, (unsigned long long)nslots}, [&] { enqueue_trial(mrest, false, nslots); });
  G.wait_flag(G.sched_.last_seq());
  for (int a : rest)
    for (int q = 0; q < NSUM; q++) tsum[(size_t)a * NSUM + q] = G.scal(a, q);
}

// x <- x+ for the nodes whose step was accepted
void Group::TntRun::accept_steps(bool unasked) {
  if ((int)acc.size() == L && X == G.Xak_.p && xprop == G.tmp_[7].p) {
    // every node of the group took its step: the trial buffer simply becomes the iterate (no copy)
    G.Xak_.swap(G.tmp_[7]);
    X = G.Xak_.p;
    xprop = G.tmp_[7].p;
    // the common course (group.h: SpecUpdate): the first round, every node's trial point taken behind its first CG step,
    // every step accepted, no further round
    bool all_tried = unasked;
    for (int a = 0; a < L; a++) all_tried = all_tried && tried[a];
    G.tnt_common_ = all_tried && tr_rounds == 1 && requad.empty();
  } else if (!acc.empty()) {
    G.set_mask(acc);
    G.copy_rows(X, xprop, false, 0);
  }
}

bool Group::run_tnt(const std::vector<int> &nodes, double *X, const double *g, const double *g_alt, bool base_ready,
                    const std::function<bool()> *confirm) {
  if (!confirm) finish_update();
  TntRun run(*this, nodes, X, g, g_alt ? g_alt : g, base_ready, confirm);
  set_mask(nodes);
  tnt_common_ = false;
  if (!(run.device_start ? run.first_round_device() : run.first_round_host())) return false;
  while (run.select_candidates(true)) run.later_round();
  // scalars the caller parked in the partial sums (amm: the half step's three) ride with the first read-back of this
  // function; if there was none (every node left at the gradient tests), fetch them now
  if (deferred_slots_) fetch(deferred_slots_, false);
  run.publish();
  return true;
}

// One CG of a refinement round, and nothing after it, on given points, linear terms and radii: for tests/test_gpu_stpcg.py.
// The same pieces in the same order as a round of run_tnt(): the model gradient and the norms, then the host start
// (host_cg_start: a later round's) or the device start (enqueue_device_start: the first round's, without the unasked trial
// point), then finish_cg.  in: per node of the GROUP, in order, [Y ; g] ((d+1) n0 rows each, debug_apply's layout); out: per
// node [s ; H s ; grad]; the rows of the nodes outside `nodes` are set to `fill` beforehand in every work vector and
// must come back as they were.  scalars: STPCG_DBG_SCALARS per node -- the six start sums, h_M_norm, cg_it, stop_ord, active,
// live, Delta (zeros for a node outside `nodes`).
int Group::debug_stpcg(const std::vector<int> &nodes, const double *in, int ld_in, const double *Delta, bool device_start,
                       double fill, double *out, int ld_out, double *scalars) {
  finish_update();
  const int L = num_local();
  if (nodes.empty() || !in || !Delta || !out || !scalars) return -1;
  NodeBits bits = 0;
  for (int a : nodes) {
    if (a < 0 || a >= L || ((bits >> a) & 1ull)) return -1;
    bits |= 1ull << a;
  }
  sched_.flush_deferred();
  sync();
  const size_t nrec = (size_t)P0_ * RS_;
  if (dbg_X_.n != nrec) { dbg_X_.alloc(nrec); dbg_g_.alloc(nrec); }
  {   // the work vectors: zero on the rows of `nodes`, `fill` elsewhere
    std::vector<double> init(nrec, fill);
    for (int a : nodes) std::fill(init.begin() + (size_t)own_off_[a] * RS_, init.begin() + (size_t)own_off_[a + 1] * RS_, 0.0);
    for (auto &t : tmp_) HIP_CHECK(hipMemcpy(t.p, init.data(), sizeof(double) * std::min(nrec, t.n), hipMemcpyHostToDevice));
  }
  std::vector<int> row0(L + 1, 0);
  for (int a = 0; a < L; a++) row0[a + 1] = row0[a] + (d_ + 1) * info_[a].n[0];
  for (int a = 0; a < L; a++) {
    const int n0 = info_[a].n[0], R0 = (d_ + 1) * n0;
    put_rows(a, dbg_X_.p, in, ld_in, 2 * row0[a], 2 * row0[a] + n0, true);
    put_rows(a, dbg_g_.p, in, ld_in, 2 * row0[a] + R0, 2 * row0[a] + R0 + n0, true);
  }
  std::fill(scalars, scalars + (size_t)L * STPCG_DBG_SCALARS, 0.0);
  const bool speculate = tnt_speculate_;
  tnt_speculate_ = false;   // (the trial point is not part of this)
  struct Restore { bool &b; bool v; ~Restore() { b = v; } } restore{tnt_speculate_, speculate};
  TntRun run(*this, nodes, dbg_X_.p, dbg_g_.p, dbg_g_.p, false, nullptr);
  set_mask(nodes);
  for (int a : nodes) run.S[a].Delta = Delta[a];
  auto sums_from = [&](int a, const double *six) { std::copy(six, six + 6, scalars + (size_t)a * STPCG_DBG_SCALARS); };
  if (device_start) {
    run.bitsA = cur_mask_.v;
    run.enqueue_device_start(0, false);
    run.seqA = sched_.last_seq();
    run.select_candidates(false);
    run.begin_round();
    wait_flag(run.seqA);
    run.read_device_verdicts();
    for (int a : nodes) sums_from(a, h_tnt_ + a * TNT_SUMMARY);
    run.finish_cg(run.any_live(1));
  } else {
    const bool have_sums = run.quad_model(run.X, false);
    run.norms(nodes, true, have_sums);
    for (int a : nodes) {
      const double six[6] = {scal(a, 0), scal(a, 1), scal(a, 2), scal(a, 3), run.use_precon ? scal(a, MAX_DOTS) : 0.0,
                             run.use_precon ? scal(a, MAX_DOTS + 1) : 0.0};
      sums_from(a, six);
    }
    if (run.select_candidates(true)) {
      run.begin_round();
      run.host_cg_start();
      run.finish_cg(run.any_live(1));
    }
  }
  sync();
  std::vector<CgNode> rec(L);
  HIP_CHECK(hipMemcpy(rec.data(), cg_.p, sizeof(CgNode) * L, hipMemcpyDeviceToHost));
  std::vector<char> active(L, 0);
  for (int a : run.A) active[a] = 1;
  for (int a : nodes) {
    double *w = scalars + (size_t)a * STPCG_DBG_SCALARS;
    if (active[a]) {
      w[6] = run.S[a].h_M_norm; w[7] = run.S[a].cg_it; w[8] = rec[a].stop_ord; w[10] = rec[a].live; w[11] = rec[a].Delta;
    }
    w[9] = active[a];
  }
  for (int a = 0; a < L; a++) {
    const int n0 = info_[a].n[0], R0 = (d_ + 1) * n0;
    get_rows(a, run.sk, out, ld_out, 3 * row0[a], 3 * row0[a] + n0, true);
    get_rows(a, run.hh, out, ld_out, 3 * row0[a] + R0, 3 * row0[a] + R0 + n0, true);
    get_rows(a, run.grad, out, ld_out, 3 * row0[a] + 2 * R0, 3 * row0[a] + 2 * R0 + n0, true);
  }
  return 0;
}

}  // namespace dpgo
