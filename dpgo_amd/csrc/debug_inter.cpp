// Test hooks for the robust inter-edge pass, the objective and the Dynamic rescale (group.h: debug_inter_update,
// debug_inter_iterate, debug_cost, debug_rescale).  Nothing here computes: each entry copies reference-layout inputs into
// record arrays, enqueues the launch the iteration makes through the iteration's own functions, and reads the results back.
#include <cstring>

#include "group.h"

namespace dpgo {

void Group::put_nbr_rows(int a, double *dev, const double *X, int ld, int row_t0, int row_r0) {
  const int n1 = info_[a].n[1];
  if (n1 == 0) return;
  std::vector<double> rec((size_t)n1 * RS_, 0.0);
  for (int k = 0; k < n1; k++)
    for (int c = 0; c < d_; c++) {
      rec[(size_t)k * RS_ + c] = X[(size_t)c * ld + row_t0 + k];
      for (int r = 0; r < d_; r++) rec[(size_t)k * RS_ + d_ + r * d_ + c] = X[(size_t)c * ld + row_r0 + k * d_ + r];
    }
  HIP_CHECK(hipMemcpy(dev + (size_t)(P0_ + nbr_off_[a]) * RS_, rec.data(), sizeof(double) * rec.size(), hipMemcpyHostToDevice));
}

void Group::get_nbr_rows(int a, const double *dev, double *X, int ld, int row_t0, int row_r0) {
  const int n1 = info_[a].n[1];
  if (n1 == 0) return;
  std::vector<double> rec((size_t)n1 * RS_);
  sync();
  HIP_CHECK(hipMemcpy(rec.data(), dev + (size_t)(P0_ + nbr_off_[a]) * RS_, sizeof(double) * rec.size(), hipMemcpyDeviceToHost));
  for (int k = 0; k < n1; k++)
    for (int c = 0; c < d_; c++) {
      X[(size_t)c * ld + row_t0 + k] = rec[(size_t)k * RS_ + c];
      for (int r = 0; r < d_; r++) X[(size_t)c * ld + row_r0 + k * d_ + r] = rec[(size_t)k * RS_ + d_ + r * d_ + c];
    }
}

namespace {
constexpr int PROX_SLOT = 2 * MAX_DOTS;   // where amm_head() has the proximal step's sum (iterate.cpp: DS)
}

// launch_inter_update through update_inter_pass, with the buffers in update()'s roles: Z = X[iter], Zprev = X[iter-1], Znbr = Xk
// (null: the pass reads Z's own neighbour rows), GX / X / Df the fused Dfobj
int Group::debug_inter_update(const InterUpdateDebug &q) {
  finish_update();
  const int a = q.local;
  if (a < 0 || a >= num_local() || opt_.loss == 0 || !q.Z || !q.DfE || !q.g || !q.sums) return -1;
  if ((q.quad && (!q.Zprev || !q.DfE_old)) || (q.with_Df && (!q.GX || !q.X || !q.Df)) || (q.recv && (!q.Znbr || !q.nsrc || q.nrecv <= 0)))
    return -1;
  const int n0 = info_[a].n[0], n1 = info_[a].n[1];
  const int own = (d_ + 1) * n0, all = (d_ + 1) * (n0 + n1);
  const size_t nall = (size_t)(P0_ + P1_) * RS_;
  sync();
  for (auto &b : dbg_all_)
    if (b.n != nall) b.alloc(nall);
  if (dbg_w_.n == 0) dbg_w_.alloc(std::max(E_.m, 1));
  for (auto &b : dbg_all_) HIP_CHECK(hipMemset(b.p, 0, sizeof(double) * nall));
  for (int k = 0; k < 5; k++) HIP_CHECK(hipMemset(tmp_[k].p, 0, sizeof(double) * tmp_[k].n));
  HIP_CHECK(hipMemset(DfE_.p, 0, sizeof(double) * nall));
  HIP_CHECK(hipMemset(dbg_w_.p, 0, sizeof(double) * dbg_w_.n));
  HIP_CHECK(hipMemset(partials_.p, 0, sizeof(double) * partials_.n));
  double *Z = dbg_all_[0].p, *Zprev = dbg_all_[1].p, *Znbr = dbg_all_[2].p;
  double *gx = tmp_[0].p, *xak = tmp_[1].p, *gc = tmp_[2].p, *dfc = tmp_[3].p;
  auto put_all = [&](double *dev, const double *X) {
    put_rows(a, dev, X, all, 0, n0, true);
    put_nbr_rows(a, dev, X, all, own, own + n1);
  };
  auto get_all = [&](const double *dev, double *X) {
    get_rows(a, dev, X, all, 0, n0, true);
    get_nbr_rows(a, dev, X, all, own, own + n1);
  };
  put_all(Z, q.Z);
  if (q.quad) { put_all(Zprev, q.Zprev); put_all(DfE_.p, q.DfE_old); }
  if (q.Znbr) put_all(Znbr, q.Znbr);
  if (q.with_Df) { put_rows(a, gx, q.GX, own, 0, n0, true); put_rows(a, xak, q.X, own, 0, n0, true); }
  const double *lazy = nullptr;
  DevBuf<double> recv;
  if (q.recv) {
    // what set_pending_recv() digests from an exchange's lists: a slot per neighbour row, and per incidence the slot of its other pose
    std::vector<int> nsrc((size_t)std::max(P1_, 1), -1);
    for (int k = 0; k < n1; k++) {
      if (q.nsrc[k] >= q.nrecv) return -1;
      nsrc[nbr_off_[a] + k] = q.nsrc[k];
    }
    std::vector<InterInc> rec = e_rec_host_;
    for (auto &r : rec) r.osrc = r.other >= P0_ ? nsrc[r.other - P0_] : -1;
    sched_.invalidate();
    HIP_CHECK(hipMemcpy(e_rec_.p, rec.data(), sizeof(InterInc) * rec.size(), hipMemcpyHostToDevice));
    recv_nsrc_.upload(nsrc);
    recv_lists_changed();   // (the digest of the group's own receive lists is gone)
    std::vector<double> buf((size_t)q.nrecv * RS_);
    for (int k = 0; k < q.nrecv; k++)
      for (int c = 0; c < d_; c++) {
        buf[(size_t)k * RS_ + c] = q.recv[(size_t)c * (d_ + 1) * q.nrecv + k];
        for (int r = 0; r < d_; r++) buf[(size_t)k * RS_ + d_ + r * d_ + c] = q.recv[(size_t)c * (d_ + 1) * q.nrecv + q.nrecv + k * d_ + r];
      }
    recv.upload(buf);
    lazy = recv.p;
  }
  HIP_CHECK(hipDeviceSynchronize());   // (the inputs went in on the null stream)
  if (q.whole) {
    std::vector<int> every(num_local());
    for (int b = 0; b < num_local(); b++) every[b] = b;
    set_mask(every);
  } else set_mask({a});
  const UpdateRoles r = {.xak = xak, .zp = Zprev, .xk = q.Znbr ? Znbr : nullptr, .zc = Z, .gc = gc, .dfc = dfc, .gx = gx, .pupd = partials_.p};
  update_inter_pass(cur_mask_, r, q.quad != 0, q.with_Df == 1, lazy, dbg_w_.p);
  // with_Df = 2: Dfobj = G X + g by a launch of its own, as robust_launches() has it where the pass does not take it along
  if (q.with_Df == 2) launch_tangent_full(lc(), r.xak, r.gx, nullptr, r.pupd, 4, r.gc, r.dfc);
  fetch(5, true);
  for (int s = 0; s < 5; s++) q.sums[s] = scal(a, s);
  get_all(DfE_.p, q.DfE);
  get_rows(a, gc, q.g, own, 0, n0, true);
  if (q.with_Df) get_rows(a, dfc, q.Df, own, 0, n0, true);
  if (q.Z_after) get_all(Z, q.Z_after);
  if (q.Znbr_after) get_all(Znbr, q.Znbr_after);
  if (q.w && e_off_[a + 1] > e_off_[a])
    HIP_CHECK(hipMemcpy(q.w, dbg_w_.p + e_off_[a], sizeof(double) * (e_off_[a + 1] - e_off_[a]), hipMemcpyDeviceToHost));
  if (q.recv) {   // the records as the group keeps them between exchanges
    sched_.invalidate();
    HIP_CHECK(hipMemcpy(e_rec_.p, e_rec_host_.data(), sizeof(InterInc) * e_rec_host_.size(), hipMemcpyHostToDevice));
  }
  return 0;
}

// launch_inter_iterate through prepare_extrapolated, the history in its own buffers: Zc = X[k], Zp = X[k-1], GXc / GXp the kept
// products, Xak the proximal step's reference point.  fused = 0: the launches of DPGO_FUSED=0 (k_extrapolate, the pass on Y,
// k_proximal); prox: the proximal half step as amm_head() takes it.
int Group::debug_inter_iterate(const InterIterateDebug &q) {
  finish_update();
  const int a = q.local, L = num_local();
  if (a < 0 || a >= L || opt_.loss == 0 || !q.Zc || !q.Zp || !q.gamma || !q.Y || !q.g || !q.sums) return -1;
  if (keep_gx() && (!q.GXc || !q.GXp || !q.Df)) return -1;
  if (q.prox && (!q.Xref || !q.Xout || !q.Xref_after)) return -1;
  const int n0 = info_[a].n[0], n1 = info_[a].n[1];
  const int own = (d_ + 1) * n0, all = (d_ + 1) * (n0 + n1);
  sync();
  for (DevBuf<double> *b : {&Zc_, &Zp_, &Y_, &Xak_, &Xakh_, &gx_, &Dfx_, &GXc_, &GXp_})
    if (b->n > 0) HIP_CHECK(hipMemset(b->p, 0, sizeof(double) * b->n));
  HIP_CHECK(hipMemset(partials_.p, 0, sizeof(double) * partials_.n));
  put_rows(a, Zc_.p, q.Zc, all, 0, n0, true);
  put_nbr_rows(a, Zc_.p, q.Zc, all, own, own + n1);
  put_rows(a, Zp_.p, q.Zp, all, 0, n0, true);
  put_nbr_rows(a, Zp_.p, q.Zp, all, own, own + n1);
  if (keep_gx()) { put_rows(a, GXc_.p, q.GXc, own, 0, n0, true); put_rows(a, GXp_.p, q.GXp, own, 0, n0, true); }
  if (q.prox) put_rows(a, Xak_.p, q.Xref, own, 0, n0, true);
  // gamma by value (the node results prepare_extrapolated reads) or in device memory -- then the by-value ones are WRONG on
  // purpose (0.5): a launch that reads them instead of the device's shows
  std::vector<double> saved(L), dev(MAX_LOCAL_NODES, 0.0);
  for (int b = 0; b < L; b++) {
    saved[b] = res_[b].gamma;
    dev[b] = q.gamma[b];
    res_[b].gamma = q.gamma_dev ? 0.5 : q.gamma[b];
  }
  if (q.gamma_dev) HIP_CHECK(hipMemcpy(coefs_dev_.p, dev.data(), sizeof(double) * MAX_LOCAL_NODES, hipMemcpyHostToDevice));
  HIP_CHECK(hipDeviceSynchronize());   // (the inputs went in on the null stream)
  if (q.whole) {
    std::vector<int> every(L);
    for (int b = 0; b < L; b++) every[b] = b;
    set_mask(every);
  } else set_mask({a});
  const bool fused_was = fused_;
  fused_ = q.fused != 0;
  const double *gd = q.gamma_dev ? coefs_dev_.p : nullptr;
  if (!prepare_extrapolated(gd, q.prox ? PROX_SLOT : -1) && q.prox)
    launch_proximal(lc(), Y_.p, Dfx_.p, Tinv_.p, N_.p, V_.p, Xakh_.p, Xak_.p, partials_.p, PROX_SLOT);
  fused_ = fused_was;
  for (int b = 0; b < L; b++) res_[b].gamma = saved[b];
  fetch(PROX_SLOT + 1, true);
  q.sums[0] = scal(a, 2);
  q.sums[1] = scal(a, PROX_SLOT);
  get_rows(a, Y_.p, q.Y, all, 0, n0, true);
  get_nbr_rows(a, Y_.p, q.Y, all, own, own + n1);
  get_rows(a, gx_.p, q.g, own, 0, n0, true);
  if (q.Df) get_rows(a, Dfx_.p, q.Df, own, 0, n0, true);
  if (q.prox) { get_rows(a, Xakh_.p, q.Xout, own, 0, n0, true); get_rows(a, Xak_.p, q.Xref_after, own, 0, n0, true); }
  return 0;
}

int Group::debug_cost(int a, int whole, int eform, const double *Zin, double *sums) {
  finish_update();
  if (a < 0 || a >= num_local() || !Zin || !sums) return -1;
  const int n0 = info_[a].n[0], n1 = info_[a].n[1];
  const int own = (d_ + 1) * n0, all = (d_ + 1) * (n0 + n1);
  sync();
  HIP_CHECK(hipMemset(Tall_.p, 0, sizeof(double) * Tall_.n));
  HIP_CHECK(hipMemset(partials_.p, 0, sizeof(double) * partials_.n));
  put_rows(a, Tall_.p, Zin, all, 0, n0, true);
  put_nbr_rows(a, Tall_.p, Zin, all, own, own + n1);
  HIP_CHECK(hipDeviceSynchronize());   // (the inputs went in on the null stream)
  if (whole) {
    std::vector<int> every(num_local());
    for (int b = 0; b < num_local(); b++) every[b] = b;
    set_mask(every);
  } else set_mask({a});
  launch_cost(lc(), Ei_, E_, eform != 0, opt_.loss, opt_.loss_reg, Tall_.p, partials_.p, 0);
  fetch(2, true);
  sums[0] = scal(a, 0);
  sums[1] = scal(a, 1);
  return 0;
}

// dynamic_detour()'s rescale: the test on given weights, then rescale_device() -- the block-diagonal terms, the numeric
// factorisation of G_tt, the panels
int Group::debug_rescale(const double *w, const double *scale, const int *count, int max_rescale_count, const int *nodes, int n,
                         int *flags, double *host_flags, double *scale_out, int *count_out) {
  finish_update();
  const int L = num_local();
  if (!dynamic() || !device_rescale_ || !w || !scale || !count || !nodes || !flags || !host_flags || !scale_out || !count_out) return -1;
  std::vector<int> set(nodes, nodes + n);
  for (int a : set)
    if (a < 0 || a >= L) return -1;
  sync();
  if (E_.m > 0) {
    HIP_CHECK(hipMemcpy(e_w_.p, w, sizeof(double) * E_.m, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(e_scale_.p, scale, sizeof(double) * E_.m, hipMemcpyHostToDevice));
  }
  HIP_CHECK(hipMemcpy(rs_count_.p, count, sizeof(int) * L, hipMemcpyHostToDevice));
  HIP_CHECK(hipDeviceSynchronize());
  set_mask(set);
  launch_rescale_decide(st_, L, cur_mask_.v, e_off_dev_.p, e_w_.p, e_scale_.p, rs_count_.p, max_rescale_count, rs_flags_.p, h_rs_);
  fetch(1, true);   // (the verdict rides with a read-back, as in dynamic_detour)
  for (int a = 0; a < L; a++) host_flags[a] = h_rs_[a];
  const std::vector<int> changed = rescale_device(set);
  sync();
  HIP_CHECK(hipMemcpy(flags, rs_flags_.p, sizeof(int) * L, hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(count_out, rs_count_.p, sizeof(int) * L, hipMemcpyDeviceToHost));
  if (E_.m > 0) HIP_CHECK(hipMemcpy(scale_out, e_scale_.p, sizeof(double) * E_.m, hipMemcpyDeviceToHost));
  return (int)changed.size();
}

// speculate_update()'s continuation under a given gate word (group.h): what a closed gate leaves untouched, what an open
// one does against the same launches without a gate.  Between iterate() and update() the
// buffers take the roles of the accepted step, as they do when speculate_update() enqueues these launches; behind update()
// the roles they have now (the launches then repeat what update() did).  Which of the two: whether the nodes are `updated`.
int Group::debug_gated_update(NodeBits go_word, int *report) {
  finish_update();
  if (!report || (go_word != 0 && go_word != ~0ull)) return -1;
  if (opt_.loss == 0 || dynamic() || !fused_ || !keep_gx() || star_ || spec_upd_.on || pending_recv_ || xchg_done_ ||
      sched_.has_deferred() || num_local() == 0)
    return -1;
  int updated = 0;
  for (int a = 0; a < num_local(); a++) {
    if (res_[a].iters < 1) return -1;
    updated += res_[a].updated != 0;
  }
  if (updated != 0 && updated != num_local()) return -1;
  flush_pending_tail();
  sync();
  const UpdateRoles r = updated == 0 ? roles_accepted(Xak_.p) : roles_now();
  DevBuf<double> *bufs[GATED_BUFFERS] = {&Xk_, &Zc_, &Zp_, &gc_, &gp_, &Dfc_, &Dfp_, &GXc_, &GXp_, &partials_, &DfE_, &e_w_};
  std::vector<std::vector<double>> saved(GATED_BUFFERS), gated(GATED_BUFFERS), plain(GATED_BUFFERS);
  const auto read = [&](std::vector<std::vector<double>> &to) {
    sync();
    for (int k = 0; k < GATED_BUFFERS; k++) {
      to[k].resize(bufs[k]->n);
      if (bufs[k]->n > 0) HIP_CHECK(hipMemcpy(to[k].data(), bufs[k]->p, sizeof(double) * bufs[k]->n, hipMemcpyDeviceToHost));
    }
  };
  const auto restore = [&] {
    sync();
    for (int k = 0; k < GATED_BUFFERS; k++)
      if (bufs[k]->n > 0) HIP_CHECK(hipMemcpy(bufs[k]->p, saved[k].data(), sizeof(double) * bufs[k]->n, hipMemcpyHostToDevice));
  };
  const auto same = [](const std::vector<double> &x, const std::vector<double> &y) {
    return x.size() == y.size() && (x.empty() || std::memcmp(x.data(), y.data(), sizeof(double) * x.size()) == 0);
  };
  NodeBits go_saved = 0;
  HIP_CHECK(hipMemcpy(&go_saved, go_.p, sizeof(NodeBits), hipMemcpyDeviceToHost));
  read(saved);
  HIP_CHECK(hipMemcpy(go_.p, &go_word, sizeof(NodeBits), hipMemcpyHostToDevice));
  update_continuation(r, go_.p);
  read(gated);
  restore();
  if (go_word != 0) {
    update_continuation(r, nullptr);
    read(plain);
    restore();
  }
  HIP_CHECK(hipMemcpy(go_.p, &go_saved, sizeof(NodeBits), hipMemcpyHostToDevice));
  for (int k = 0; k < GATED_BUFFERS; k++) {
    report[3 * k] = bufs[k]->n > 0;
    report[3 * k + 1] = same(gated[k], saved[k]);
    report[3 * k + 2] = go_word != 0 ? (int)same(gated[k], plain[k]) : -1;
  }
  return 0;
}

}  // namespace dpgo
