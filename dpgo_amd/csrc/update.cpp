// Group::update (DPGOHash::update, DPGOHash.cpp:84-228) and what belongs to it: its deferred end, the update enqueued ahead of
// the host's decision, the tail of iterate() that rides on it.  The launches of the robust, statically scaled build are stated
// ONCE here (update_product, update_inter_pass, update_reduce); update() and speculate_update() differ in the node mask and in
// the roles of the buffers they hand them (group.h: UpdateRoles).
#include <algorithm>
#include <cmath>
#include <limits>

#include "group.h"

namespace dpgo {

#define DPGO_DIFFERS(f) if (f != o.f) return #f
const char *Group::UpdateRoles::differs(const UpdateRoles &o) const {
  DPGO_DIFFERS(xak); DPGO_DIFFERS(xk); DPGO_DIFFERS(zc); DPGO_DIFFERS(zp);
  DPGO_DIFFERS(gc); DPGO_DIFFERS(dfc); DPGO_DIFFERS(gx); DPGO_DIFFERS(pupd);
  return nullptr;
}
const char *Group::UpdateDesc::differs(const UpdateDesc &o) const {
  DPGO_DIFFERS(seg_id); DPGO_DIFFERS(fuse_copy); DPGO_DIFFERS(nslots); DPGO_DIFFERS(bits); DPGO_DIFFERS(split);
  DPGO_DIFFERS(lazy_recv); DPGO_DIFFERS(seq_last); DPGO_DIFFERS(deferred); DPGO_DIFFERS(tail);
  return roles.differs(o.roles);
}
#undef DPGO_DIFFERS

// update()'s partial sums have slots of their own (UPD_SLOT0 ..): they may wait there for the next refinement's
// k_cg_scal_begin to reduce them (close_update: `lazy`) while that refinement's passes use the first slots.  Not with Dynamic
// rescale (its fetch() in the middle reads the first slots) nor when parked sums ride along (they are in the first slots)
Group::UpdateRoles Group::roles_now() const {
  return {.xak = Xak_.p, .zp = Zp_.p, .xk = Xk_.p, .zc = Zc_.p, .gc = gc_.p, .dfc = Dfc_.p, .gx = (opt_.loss != 0 && keep_gx()) ? GXc_.p : T1_.p,
          .pupd = (dynamic() || deferred_slots_ != 0) ? partials_.p : upd_slots()};
}

// the accepted point is the trial buffer; the history rotates (X[iter] <- what is X[iter-1] now, and so on); update()'s own
// slots (deferred_slots_ is 0 there, Dynamic is off: spec_update_possible)
Group::UpdateRoles Group::roles_accepted(const double *xprop) const {
  return {.xak = xprop, .zp = Zc_.p, .xk = Xk_.p, .zc = Zp_.p, .gc = gp_.p, .dfc = Dfp_.p, .gx = GXp_.p, .pupd = upd_slots()};
}

// ---- the stated sequence
// G X -> gx and <X, 1/2 G X> -> slot 5 (half of evaluate_G, DPGOProblem.cpp:180-205; kept as G X[k] where the next extrapolation
// reuses it).  from_xak: on Xak's records (the same numbers as X[iter]'s own rows); carry_tail: ... which go to Xk and X[iter] on the way
void Group::update_product(const NodeMask &m, const UpdateRoles &r, bool from_xak, bool carry_tail) {
  const double *x = from_xak ? r.xak : r.zc;
  BsrArgs a = {.x = x, .y = r.gx, .dot = {.v = x, .coef = 0.5, .partials = r.pupd, .slot = 5}};
  if (carry_tail) a.copy = BsrCopy{.to1 = r.xk, .to2 = r.zc};
  launch_bsr(lc(m), G_.dev, a);
}

// the inter-edge pass: slots 0, 1 and 2 = <X, g>; quad: a later iteration (the majorisation gap against X[iter-1]);
// with_Df: Dfobj and |grad F|^2 (slot 4) on the way; lazy_recv: the receive buffer of a lazy unpack
void Group::update_inter_pass(const NodeMask &m, const UpdateRoles &r, bool quad, bool with_Df, const double *lazy_recv, double *wout) {
  InterEdgesDev E = E_;
  if (lazy_recv) { E.recv = lazy_recv; E.nsrc = recv_nsrc_.p; }
  InterUpdate up = {.quad = quad, .Z = r.zc, .Zprev = r.zp, .Qdiag = Qd_.p, .Ddiag = Dd_.p, .DfE = DfE_.p, .g = r.gc,
                    .partials = r.pupd, .wout = wout ? wout : (dynamic() ? e_w_.p : nullptr), .Znbr = r.xk};
  if (with_Df) { up.GX = r.gx; up.X = r.xak; up.Df = r.dfc; up.gn_slot = 4; }
  launch_inter_update(lc(m), E, opt_.loss, opt_.loss_reg, up);
}

void Group::update_reduce(int nslots, const double *pupd) {
  launch_reduce(st_, T_, num_local(), true, nslots, pupd, h_upd_, sched_.flag());
}

// ---- the update enqueued ahead of the host's decision (group.h: SpecUpdate)
// spec_update_possible: asked by run_tnt() before it enqueues the head of a refinement -- the trial
// point's reduction then waits for speculate_update(), which is called once update(k-1)'s scalars are taken (the gate gets
// them by value) and enqueues that reduction WITH the gate in one launch, then the continuation.
bool Group::spec_update_possible(const double *xprop) const {
  const int L = num_local();
  if (!spec_update_armed_ || !spec_update_enabled_ || !fused_ || !keep_gx() || star_ || sched_.capturing() || sched_.iter_graph_wanted() ||
      xchg_done_ || pending_recv_ || sched_.has_deferred() || pending_tail_.on || xprop != tmp_[7].p || L == 0)
    return false;
  for (int a = 0; a < L; a++)
    if (res_[a].iters < 1 || !res_[a].updated) return false;   // (every node: a later update, never a node's first)
  return true;
}

AmmGate Group::amm_gate(int L, const Options &o, const std::function<GateNode(int)> &node) {
  AmmGate G;
  G.nnodes = L; G.ds = 2 * MAX_DOTS; G.max_it = o.max_iterations; G.max_acc = o.max_iterations_accepted;
  G.max_hits0 = o.max_soft_restart_hits[0]; G.max_hits1 = o.max_soft_restart_hits[1];
  G.sqrt_eps = TntConst::sqrt_eps(); G.eta1 = TntConst::eta1;
  G.rel_tol = o.rel_func_decrease_tol; G.step_tol = o.stepsize_tol; G.psi = o.psi; G.phi = o.phi;
  for (int a = 0; a < MAX_LOCAL_NODES; a++) {
    const GateNode n = a < L ? node(a) : GateNode{0.0, 0.0, 0.0, 0.0, 0, 0};
    G.f[a] = n.f; G.Fk0[a] = n.Fk0; G.Fk1[a] = n.Fk1; G.fobj[a] = n.fobj;
    G.hits0[a] = n.hits0; G.hits1[a] = n.hits1;
  }
  return G;
}

// the launches of the common course behind the gate: the local halo copy, then update()'s later-iteration product (with
// iterate()'s tail) and inter-edge pass, all under the device word `gate` (null: unconditionally -- a test hook's comparison)
void Group::update_continuation(const UpdateRoles &r, const NodeBits *gate) {
  const NodeMask m{all_bits(), gate};
  if (gather_dst_.n > 0) launch_copy_indexed(d_, st_, (int)gather_dst_.n, gather_dst_.p, gather_src_.p, r.xak, r.xk, gate);
  update_product(m, r, true, true);
  update_inter_pass(m, r, true, true, nullptr);
}

void Group::speculate_update(const double *xprop, int nslots_trial) {
  spec_upd_ = SpecUpdate();
  const int L = num_local();
  const AmmGate G = amm_gate(L, opt_, [this](int a) {
    const NodeResults &r = res_[a];
    return GateNode{r.f, r.Fk[0], r.Fk[1], r.fobj, r.soft_restart_hits[0], r.soft_restart_hits[1]};
  });
  // the trial point's sums to the host (k_reduce's work, its flag) and the gate's verdict, one launch
  launch_reduce_gate(st_, T_, L, nslots_trial, partials_.p, h_scal_, sched_.flag(), dev_sums_.p, G, dev_tnt_.p, cg_.p, go_.p, h_gate_);
  spec_upd_.seq_trial = sched_.last_seq();
  // the common course from here: iterate()'s tail and the local halo copy, then update()'s later-iteration sequence for the
  // static robust surrogate, all under the gate's word
  const UpdateRoles r = roles_accepted(xprop);
  update_continuation(r, go_.p);
  // (the closing reduction: left to the next refinement where update() itself would leave it, group.h: UpdLazy)
  spec_upd_.lazy = lazy_update_reduce();
  if (!spec_upd_.lazy) update_reduce(6, r.pupd);
  n_spec_enqueued_++;
  spec_upd_.on = true;
  // (what update() must find: its later-iteration segment over every node, the tail on the product, the read-back deferred)
  spec_upd_.what = {.roles = r, .seg_id = 4, .nslots = 6, .bits = all_bits(), .fuse_copy = true, .deferred = true, .tail = true,
                    .seq_last = sched_.last_seq()};
}

// The host has taken its decision: the enqueued continuation stands (the common course) or is forgotten (its launches fell
// through); either way the gate's verdict, which arrives behind the trial point's flag, is compared at the next wait that
// covers it.
void Group::check_gate(bool host_common) {
  if (!spec_upd_.on) return;
  spec_verdict_pending_ = true;
  spec_verdict_expected_ = host_common;
  spec_verdict_seq_ = spec_upd_.seq_trial;   // (the verdict is written in front of that flag)
  if (!host_common) spec_upd_ = SpecUpdate();
  else n_spec_stood_++;
}

// update()'s closing reduction left for the next refinement's k_cg_scal_begin (group.h: UpdLazy): eager launches of the fused
// sequence only (a replayed segment is a fixed list of launches)
bool Group::lazy_update_reduce() const {
  return settings().lazy_update_reduce && fused_ && keep_gx() && !star_ && !sched_.capturing() && !sched_.iter_graph_wanted();
}

void Group::flush_pending_tail() {
  if (!pending_tail_.on) return;
  const PendingTail p = pending_tail_;
  pending_tail_.on = false;
  launch_axpby(lc(p.m), false, 1.0, p.xak, 0.0, nullptr, p.xk, 0, p.z);
}

// The deferred end of update(): wait for its reduction, then the scalar logic that needs the numbers.
void Group::finish_update() {
  if (!pending_update_) return;
  if (upd_lazy_.pending) {   // (nobody has taken update()'s reduction along: launch it now)
    upd_lazy_.pending = false;
    update_reduce(upd_lazy_.nslots, upd_slots());
    pending_seq_ = sched_.last_seq();
  }
  std::function<void()> f;
  f.swap(pending_update_);
  wait_flag(pending_seq_);
  f();
}

// The part of the scalar logic that does not need the numbers update() reads back: the Nesterov sequence s[iter],
// s[iter+1] and gamma (DPGOHash.cpp:150-160, 206-216).  The next iterate() may start with it.
void Group::host_update_pre(int a) {
  NodeResults &r = res_[a];
  const int it = r.iters;
  r.pre_repeat = (r.hist_iter == it);
  r.pre_done = true;
  if (opt_.scheme == 1) {
    if (it == 0) r.s0 = 1.0;
    else if (!r.pre_repeat) r.s0 = r.s1;
    r.s1 = 0.5 + 0.5 * std::sqrt(4.0 * r.s0 * r.s0 + 1.0);
    r.gamma = (r.s0 - 1) / r.s1;
  } else {
    r.gamma = 0;
  }
}

void Group::host_update_logic(int a, double fobj, double f, double gradFnorm) {
  NodeResults &r = res_[a];
  const Options &o = opt_;
  const int it = r.iters;
  // update() may run again at the same iteration (update -> receive() -> update): X[iter-1], fobj[iter-1] and
  // s[iter] are those of the first call, everything else is re-done as the reference does (DPGOHash.cpp:99-225)
  if (!r.pre_done && !star_) host_update_pre(a);   // (the Nesterov sequence, unless update() advanced it when it deferred this)
  const bool repeat = r.pre_done ? r.pre_repeat : (r.hist_iter == it);
  r.pre_done = false;
  r.hist_iter = it;
  if (!repeat) r.fobj_prev = r.fobj;
  r.fobj = fobj;
  r.f = f;
  r.gradFnorm = gradFnorm;
  if (star_) {   // update_n (DPGOStar.cpp:339-385): no restart counters, Gk = Fk = fobj every iteration
    r.Gk = fobj;
    if (o.scheme == 1) {
      if (!repeat) r.s0 = it == 0 ? 1.0 : r.s1;
      r.s1 = 0.5 + 0.5 * std::sqrt(4.0 * r.s0 * r.s0 + 1.0);
      r.gamma = (r.s0 - 1) / r.s1;
    }
    r.Fk[0] = r.Fk[1] = fobj;
    r.updated = 1;
    return;
  }
  if (it == 0) {
    r.Fk[0] = r.Fk[1] = fobj;
    r.Gk = fobj;
  }
  if (o.scheme == 1) {
    if (it == 0) {
      if (!repeat) r.oscillations.assign(1, 1);
      else r.oscillations.push_back(1);   // the reference pushes again (DPGOHash.cpp:168-171)
    }
    if (fobj <= r.Fk[1]) r.soft_restart_hits[0] = r.soft_restart_hits[0] > 2 ? r.soft_restart_hits[0] - 2 : 0;
    else r.soft_restart_hits[0]++;
    if (it > 0) {
      if (fobj <= r.fobj_prev) { r.soft_restart_hits[1] = 0; r.oscillations.push_back(1); }
      else { r.soft_restart_hits[1]++; r.oscillations.push_back(0); }
      r.num_oscillations += (r.oscillations[it] != r.oscillations[it - 1]);
    }
    if (it > o.oscillation_cnt_period) {
      const int k = it - o.oscillation_cnt_period;
      r.num_oscillations -= (r.oscillations[k] != r.oscillations[k - 1]);
    }
    r.Fk[0] = r.Fk[0] * (1 - o.eta[0]) + fobj * o.eta[0];
    r.Fk[1] = std::max(fobj, r.Fk[1] * (1 - o.eta[1]) + fobj * o.eta[1]);
  } else {
    r.Fk[0] = r.Fk[1] = fobj;
  }
  r.updated = 1;
}

// ---- update() in phases
// The host-side facts of a call (group.h: UpdatePlan); nothing is launched and no member changes here
Group::UpdatePlan Group::plan_update(const std::vector<int> &locals_in) const {
  UpdatePlan p;
  for (int a : locals_in)
    if (!res_[a].updated) p.locals.push_back(a);
  p.trivial = (opt_.loss == 0);
  for (int a : p.locals) {
    p.bits |= 1ull << a;
    if (res_[a].hist_iter != res_[a].iters) p.adv.push_back(a);
    ((res_[a].iters == 0 || star_) ? p.first : p.later).push_back(a);
  }
  p.mask = live_mask(p.bits, nullptr);
  p.rotate = (int)p.adv.size() == num_local();
  p.both = !p.first.empty() && !p.later.empty();
  // the closing read-back is deferred to the next reader (finish_update) where there is exactly one of them and nothing
  // depends on it at once: not for AMM-PGO* (the master decides on the sums right away) nor with Dynamic rescale
  p.can_defer = settings().defer_update && !star_ && !dynamic() && (p.first.empty() != p.later.empty());
  // the tail of iterate() rides on the product with G (group.h: PendingTail) where that product reads the very records the
  // tail copies: every node advances, the copy's second target is the buffer that becomes X[iter] in advance_history
  p.fuse_copy = pending_tail_.on && !p.trivial && p.rotate && zc_ready_ && !xchg_done_ && !star_ && pending_tail_.m.v == p.bits &&
                pending_tail_.z == Zp_.p && pending_tail_.xk == Xk_.p && pending_tail_.xak == Xak_.p;
  // The new linearisation point needs the neighbours' poses, which may still be on their way (an exchange on the
  // communicator's stream, comm.cpp).  What needs no neighbour row goes first -- X[iter] own rows and the product
  // with G, a third of the surrogate build -- then the stream waits for the exchange and takes the neighbour rows.
  // Without a pending exchange the product is simply the head of a segment (update_head).
  p.split = xchg_done_ != nullptr;
  // a lazy unpack is taken by the one inter-edge pass that covers every node of the group (it delivers all neighbour rows
  // at once); anything else gets the plain copy first
  if (!p.trivial && !p.both && !dynamic() && p.bits == all_bits()) p.lazy_recv = pending_recv_;
  return p;
}

// history: X[iter-1] <- X[iter], X[iter] <- Xk ; same for g and Dfobj (masked nodes only).  A node whose
// history already stands at this iteration (update() ran, then receive() cleared `updated`) only refreshes
// X[iter]: the reference overwrites X[iter] / g[iter] in place and leaves X[iter-1] alone (DPGOHash.cpp:99-106).
void Group::advance_history(const UpdatePlan &p) {
  bool zc_done = false;
  if (p.rotate) {
    // every node advances: rotate the buffers instead of copying them
    Zp_.swap(Zc_);
    gp_.swap(gc_);
    Dfp_.swap(Dfc_);
    if (keep_gx()) GXp_.swap(GXc_);
    zc_done = zc_ready_;   // iterate() already left Xk's own rows in what is X[iter] now
  } else if (!p.adv.empty()) {
    set_mask(p.adv);
    copy_rows(Zp_.p, Zc_.p, true);
    copy_rows(gp_.p, gc_.p, false);
    copy_rows(Dfp_.p, Dfc_.p, false);
    if (keep_gx()) copy_rows(GXp_.p, GXc_.p, false);
    cur_mask_ = p.mask;
  }
  zc_ready_ = false;
  if (!zc_done) copy_rows(Zc_.p, Xk_.p, false);
}

// (what a segment starts with when the product has not gone ahead; the trivial loss takes T1 = G Xak and <Xak, 1/2 G Xak>)
void Group::update_head(const UpdatePlan &p, const UpdateRoles &r) {
  if (p.split) return;
  cur_mask_ = p.mask;
  if (p.fuse_copy) pending_tail_.on = false;   // (it rides on this product)
  update_product(cur_mask_, r, p.trivial || p.fuse_copy, p.fuse_copy);
}

// X[iter]'s neighbour rows <- Xk's: a launch of its own for the trivial loss; the robust losses' inter-edge pass does it
// on the way (it reads the neighbour rows from Xk and stores them)
// g = S Z  (evaluate_none_g_and_f0 / _f, DPGOProblem.cpp:269-287, 516-542), with <Xak, g> alongside
void Group::trivial_common(const UpdatePlan &p, const UpdateRoles &r) {
  update_head(p, r);
  cur_mask_ = p.mask;
  launch_copy_nbr_rows(lc(), r.xk, r.zc);
  launch_bsr(lc(), S_.dev, {.x = r.zc, .y = r.gc, .dot = {.v = r.xak, .coef = 1.0, .partials = r.pupd, .slot = 1}});
}

void Group::trivial_launches(const UpdatePlan &p, const UpdateRoles &r, bool later) {
  if (!p.both) trivial_common(p, r);
  set_mask(later ? p.later : p.first);
  if (!later) {
    launch_bsr(lc(), P0m_.dev, {.all_rows = true, .x = r.zc, .dot = {.v = r.zc, .coef = 0.5, .partials = r.pupd, .slot = 0}});
  } else {
    launch_axpby(lc(), true, 1.0, r.zc, -1.0, r.zp, Tall_.p, 0);
    launch_bsr(lc(), Q_.dev, {.all_rows = true, .x = Tall_.p, .dot = {.v = Tall_.p, .coef = 0.5, .partials = r.pupd, .slot = 0}});
    launch_bsr(lc(), P_.dev, {.all_rows = true, .x = r.zc, .dot = {.v = r.zc, .coef = 0.5, .partials = r.pupd, .slot = 3}});
  }
  // fobj = G(Xak | g, f0) = f0 + <Xak, g> + <Xak, 1/2 G Xak>: slots 1 and 5; Dfobj = g + G Xak
  launch_tangent_full(lc(), r.xak, r.gx, nullptr, r.pupd, 2, r.gc, r.dfc);
}

void Group::build_trivial(const UpdatePlan &p, const UpdateRoles &r) {
  flush_pending_recv();
  if (p.both) sched_.flush_deferred();
  if (p.both) trivial_common(p, r);   // (nodes at different iterations: two read-backs, nothing deferred, the shared part goes first)
  const unsigned long long variant = (p.split ? 1ull : 0ull) | (p.both ? 2ull : 0ull);
  if (!p.first.empty())
    close_update(p, r, 1, variant, 6, p.first, [this, &p, &r] { trivial_launches(p, r, false); }, [this, first = p.first] {
      for (int a : first) {
        const double f0 = uscal(a, 0);
        host_update_logic(a, f0 + (uscal(a, 1) + uscal(a, 5)), f0, std::sqrt(uscal(a, 2)));
      }
    });
  if (!p.later.empty())
    close_update(p, r, 2, variant, 4, p.later, [this, &p, &r] { trivial_launches(p, r, true); }, [this, later = p.later] {
      for (int a : later) {
        const double fobj = res_[a].Gk + uscal(a, 0);
        host_update_logic(a, fobj, fobj + uscal(a, 3), std::sqrt(uscal(a, 2)));
      }
    });
}

// Rescale::Dynamic: the inter-edge pass goes ahead of the segment.  The sum of rho and the majorisation gap (under the OLD Q)
// are final; whether the surrogate is rescaled depends on the edge weights just computed (DPGOProblem.cpp:300-321, :464-485).
// Rescaled nodes get their D, G, T, N, V, Q and the factor of G_tt rebuilt, and g, G X are taken again with the new operators.
void Group::dynamic_detour(const UpdateRoles &r, const std::vector<int> &set, bool quad, std::vector<double> &rho, std::vector<double> &gap) {
  set_mask(set);
  update_inter_pass(cur_mask_, r, quad, false, nullptr);
  if (device_rescale_)   // the rescale test on the weights just computed; its verdict rides with the sums below
    launch_rescale_decide(st_, num_local(), cur_mask_.v, e_off_dev_.p, e_w_.p, e_scale_.p, rs_count_.p, opt_.max_rescale_count,
                          rs_flags_.p, h_rs_);
  fetch(3, true);
  for (int a : set) { rho[a] = scal(a, 0); gap[a] = scal(a, 1); }
  const std::vector<int> changed = device_rescale_ ? rescale_device(set) : maybe_rescale(set);
  if (!changed.empty()) {
    set_mask(changed);
    update_product(cur_mask_, r, false, false);
    // g = DfobjE_own - D X with the new D (slot 2 = <X, g> again)
    launch_inter_iterate(lc(), E_, opt_.loss, opt_.loss_reg, {.Z = r.zc, .Ddiag = Dd_.p, .g = r.gc, .partials = r.pupd});
    set_mask(set);
  }
}

// the launches of a robust segment (the inter-edge pass has gone ahead with Dynamic rescale).  GXp_ is no role of update()'s
// launches: a node's first update has no X[k-1] yet -- gamma is 0 there, but the buffer must hold numbers
void Group::robust_launches(const UpdatePlan &p, const UpdateRoles &r, const std::vector<int> &set, const std::vector<int> &fresh,
                            bool quad, bool head_inside) {
  if (head_inside) update_head(p, r);
  set_mask(set);
  // Dfobj = G X + g, its tangent projection and norm: inside the inter-edge pass (kernels.h: InterUpdate::Df), or k_tangent_full
  const bool in_pass = !dynamic() && fused_;
  if (!dynamic()) update_inter_pass(cur_mask_, r, quad, in_pass, p.lazy_recv);
  if (!quad) launch_bdiag_dot(lc(), Dd_.p, r.zc, 0.5, DfE_.p, -1.0, r.pupd, 3);
  if (!in_pass) launch_tangent_full(lc(), r.xak, r.gx, nullptr, r.pupd, 4, r.gc, r.dfc);   // Dfobj = G X + g
  if (!fresh.empty()) {
    set_mask(fresh);
    copy_rows(GXp_.p, GXc_.p, false);
    set_mask(set);
  }
}

// evaluate_g_and_f0 / evaluate_g_and_f (DPGOProblem.cpp:222-267, 360-424); _rescale variants (:289-358, :426-514)
void Group::build_robust(const UpdatePlan &p, const UpdateRoles &r) {
  if (pending_recv_) {
    if (p.lazy_recv) pending_recv_ = nullptr;
    else flush_pending_recv();
  }
  const bool dyn = dynamic(), head_inside = !(p.both || dyn);
  if (!head_inside) {   // (the product covers every node of `locals`: it cannot sit inside one of two segments)
    sched_.flush_deferred();
    update_head(p, r);
  }
  for (int pass = 0; pass < 2; pass++) {
    const std::vector<int> &set = pass == 0 ? p.first : p.later;
    if (set.empty()) continue;
    std::vector<double> rho(num_local(), 0.0), gap(num_local(), 0.0);
    if (dyn) dynamic_detour(r, set, pass == 1, rho, gap);
    std::vector<int> fresh;
    if (keep_gx())
      for (int a : set)
        if (res_[a].iters == 0) fresh.push_back(a);
    NodeBits fresh_bits = 0;
    for (int a : fresh) fresh_bits |= 1ull << a;
    const unsigned long long variant = (p.split ? 1ull : 0ull) | (head_inside ? 2ull : 0ull) | (dyn ? 4ull : 0ull) | (fused_ ? 8ull : 0ull) |
                                       (p.lazy_recv ? 16ull : 0ull) | (fresh_bits << 5);
    close_update(p, r, 3 + pass, variant, 6, set,
                 [this, &p, &r, &set, &fresh, pass, head_inside] { robust_launches(p, r, set, fresh, pass == 1, head_inside); },
                 [this, set, pass, dyn, rho, gap] {
      for (int a : set) {
        NodeResults &n = res_[a];
        const double fobjE = 0.5 * (dyn ? rho[a] : uscal(a, 0));
        const double quad = uscal(a, 2) + uscal(a, 5);   // tr(X^T (g + 1/2 G X))
        double fobj, f;
        if (pass == 0) {
          f = 0.5 * fobjE + uscal(a, 3);
          fobj = f + quad;
        } else {
          fobj = n.Gk - 0.5 * n.fobjE - 0.5 * (dyn ? gap[a] : uscal(a, 1)) + 0.5 * fobjE;
          f = fobj - quad;
        }
        n.fobjE = fobjE;
        host_update_logic(a, fobj, f, std::sqrt(uscal(a, 4)));
      }
    });
  }
}

// The close of a build over the nodes of `set`.  `launches`: the rest of the surrogate build, which the closing reduction of
// its sums ends -- a branch-free sequence, replayed from a captured graph where the host's launch rate would bound it
// (segment()); not called when everything went out ahead (speculate_update).  `logic`: the scalar logic on the sums,
// now or deferred (it outlives this call: it captures by value).
void Group::close_update(const UpdatePlan &p, const UpdateRoles &r, int seg_id, unsigned long long variant, int nslots,
                         const std::vector<int> &set, const std::function<void()> &launches, std::function<void()> logic) {
  nslots = take_deferred_slots(nslots);
  NodeBits bits = 0;
  for (int a : set) bits |= 1ull << a;
  // the closing reduction is left to the next refinement's k_cg_scal_begin (group.h: UpdLazy) where the read-back is
  // deferred anyway and the launches are eager: one launch less on the stream
  // (only where the next iterate() starts its refinement unasked -- every node was refined in this one: otherwise the host
  // wants these sums before it enqueues anything that could carry them)
  bool lazy = p.can_defer && lazy_update_reduce() && spec_refined_ && r.pupd != partials_.p && nslots <= 6 && bits == all_bits();
  if (spec_upd_.on) {
    // the launches of this sequence went out ahead of the host's decision (speculate_update) and the decision was the
    // common one: what they were given must be what this call would have given them
    const SpecUpdate sp = spec_upd_;
    spec_upd_ = SpecUpdate();
    lazy = sp.lazy;   // (they decided for themselves: the policy may have changed since -- count_iteration() in update())
    const UpdateDesc found = {.roles = r, .seg_id = seg_id, .nslots = nslots, .bits = bits, .fuse_copy = p.fuse_copy, .split = p.split,
                              .lazy_recv = p.lazy_recv != nullptr, .deferred = p.can_defer, .tail = pending_tail_.on,
                              .seq_last = sched_.last_seq()};
    if (const char *field = found.differs(sp.what)) {
      failed_ = true;
      fprintf(stderr, "[dpgo_amd] ERROR: a speculative update was enqueued for another state than update() found: `%s` differs "
                      "(segment %d, slots %d, flags %llu / %llu)\n", field, seg_id, nslots, sp.what.seq_last, found.seq_last);
      throw DeviceError("a speculative update was enqueued for another state than update() found");
    }
    pending_tail_.on = false;   // (it rode on the enqueued product with G)
  } else
  segment(seg_id, bits & p.bits, {bits, p.bits, variant, (unsigned long long)nslots, p.fuse_copy ? 1ull : 0ull, (unsigned long long)(uintptr_t)p.lazy_recv},
          [this, &launches, &r, lazy, nslots] {
    launches();
    if (!lazy) update_reduce(nslots, r.pupd);
  });
  if (lazy) { upd_lazy_.pending = true; upd_lazy_.nslots = nslots; }
  if (p.can_defer) {
    pending_seq_ = lazy ? 0ull : sched_.last_seq();   // (lazy: whoever launches the reduction sets it -- run_tnt, or finish_update)
    for (int a : set) {
      host_update_pre(a);
      res_[a].updated = 1;
    }
    pending_update_ = std::move(logic);
  } else {
    wait_flag(sched_.last_seq());
    logic();
  }
}

int Group::update(const std::vector<int> &locals_in) {
  Schedule::InLib in_lib(sched_);
  if (failed_) { flush_pending_tail(); sched_.flush_deferred(); pending_recv_ = nullptr; return -1; }
  finish_update();
  const UpdatePlan p = plan_update(locals_in);
  if (p.locals.empty()) {
    flush_pending_tail();
    sched_.flush_deferred();
    flush_pending_recv();
    join_exchange();   // a pending exchange must still be ordered before whatever the caller does next on this stream
    return 0;
  }
  sched_.count_iteration();
  cur_mask_ = p.mask;
  // (launches that wait for this update()'s first segment -- step() -- go now if something eager comes before it)
  if (!p.rotate || !zc_ready_ || p.split || dynamic() || star_) sched_.flush_deferred();
  if (!p.fuse_copy) flush_pending_tail();
  advance_history(p);
  const UpdateRoles r = roles_now();
  if (p.split) {   // the product with G ahead of the exchange's arrival
    update_product(p.mask, r, p.trivial, false);
    join_exchange();
  }
  if (p.trivial) build_trivial(p, r);
  else build_robust(p, r);
  flush_pending_tail();   // (nothing, unless the product with G never came)
  return 0;
}

}  // namespace dpgo
