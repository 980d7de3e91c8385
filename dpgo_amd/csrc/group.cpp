#include "group.h"

#include <limits>
#include "graph.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <set>

namespace dpgo {

static bool g_leak_device_buffers = false;
void dev_leak_buffers(bool on) { g_leak_device_buffers = on; }
template <class T>
void DevBuf<T>::release() {
  if (g_leak_device_buffers) { p = nullptr; n = 0; return; }
  if (p) (void)hipFree(p);
  p = nullptr;
  n = 0;
}
template <class T>
void DevBuf<T>::alloc(size_t count, bool zero) {
  release();
  n = count;
  const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
  HIP_CHECK(hipMalloc((void **)&p, bytes));
  if (zero) HIP_CHECK(hipMemset(p, 0, bytes));
}
template <class T>
void DevBuf<T>::upload(const std::vector<T> &h) {
  alloc(h.size(), h.empty());
  if (!h.empty()) HIP_CHECK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
}
template <class T>
void DevBuf<T>::download(std::vector<T> &h) const {
  h.resize(n);
  if (n) HIP_CHECK(hipMemcpy(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost));
}
template struct DevBuf<int>;
template struct DevBuf<double>;
template struct DevBuf<int64_t>;
template struct DevBuf<int4>;
template struct DevBuf<Seg>;
template struct DevBuf<SpdItem>;
template struct DevBuf<unsigned>;
template struct DevBuf<CgNode>;
template struct DevBuf<NodeBits>;
template struct DevBuf<PanelSrc>;
template struct DevBuf<InterInc>;
template struct DevBuf<RootDesc>;
template struct DevBuf<RootRow>;
template struct DevBuf<float>;

// lambda_max of a symmetric matrix by Lanczos with full reorthogonalisation (stands in for the
// Spectra call of DPGOProblem.cpp:106-118, tolerance 1e-4).
static double lanczos_lambda_max(const CsrMatrix &A) {
  const int n = A.n, kmax = std::min(n, 60);
  if (n == 0) return 0.0;
  std::vector<std::vector<double>> Q;
  std::vector<double> alpha, beta, q(n), w(n);
  for (int i = 0; i < n; i++) q[i] = 1.0 + 0.37 * std::sin(1.7 * i + 0.3);
  double nrm = 0;
  for (double v : q) nrm += v * v;
  nrm = std::sqrt(nrm);
  for (double &v : q) v /= nrm;
  double lam_prev = 0, lam = 0;
  for (int k = 0; k < kmax; k++) {
    Q.push_back(q);
    for (int i = 0; i < n; i++) {
      double s = 0;
      for (int e = A.ptr[i]; e < A.ptr[i + 1]; e++) s += A.val[e] * q[A.col[e]];
      w[i] = s;
    }
    double a = 0;
    for (int i = 0; i < n; i++) a += w[i] * q[i];
    alpha.push_back(a);
    for (int pass = 0; pass < 2; pass++)
      for (const auto &qq : Q) {
        double c = 0;
        for (int i = 0; i < n; i++) c += w[i] * qq[i];
        for (int i = 0; i < n; i++) w[i] -= c * qq[i];
      }
    double b = 0;
    for (double v : w) b += v * v;
    b = std::sqrt(b);
    // largest eigenvalue of the tridiagonal (alpha, beta) by bisection on the Sturm sequence
    const int m = (int)alpha.size();
    double lo = -1e300, hi = -1e300;
    for (int i = 0; i < m; i++) {
      double r = (i > 0 ? std::fabs(beta[i - 1]) : 0) + (i < m - 1 ? std::fabs(beta[i]) : 0);
      hi = std::max(hi, alpha[i] + r);
      lo = std::max(lo, alpha[i] - r);
    }
    lo = std::min(lo, hi - 1.0);
    for (int it = 0; it < 200; it++) {
      const double mid = 0.5 * (lo + hi);
      int neg = 0;   // number of eigenvalues < mid
      double dd = 1.0;
      for (int i = 0; i < m; i++) {
        dd = alpha[i] - mid - (i > 0 ? beta[i - 1] * beta[i - 1] / dd : 0.0);
        if (dd == 0.0) dd = 1e-300;
        if (dd < 0) neg++;
      }
      if (neg == m) hi = mid; else lo = mid;
      if (hi - lo <= 1e-14 * std::fabs(hi)) break;
    }
    lam = 0.5 * (lo + hi);
    if (k > 3 && std::fabs(lam - lam_prev) <= 1e-6 * std::fabs(lam)) break;
    lam_prev = lam;
    if (b < 1e-12 * std::fabs(lam)) break;
    beta.push_back(b);
    for (int i = 0; i < n; i++) q[i] = w[i] / b;
  }
  return lam;
}

Group::Group(const Graph &g, const std::vector<int> &node_ids, const Options &opt, int device)
    : d_(g.d), device_(device), opt_(opt), nodes_(node_ids) {
  RS_ = (d_ + 1) * d_;
  B_ = d_ + 1;
  num_poses_global_ = g.num_poses;
  num_nodes_total_ = g.num_nodes;
  if (d_ != 2 && d_ != 3) {
    fprintf(stderr, "[dpgo_amd] ERROR: d must be 2 or 3.\n");
    return;
  }
  if (opt.preconditioner != 0 && opt.preconditioner != 1 && opt.preconditioner != 3) {
    fprintf(stderr, "[dpgo_amd] ERROR: preconditioner %d (IncompleteCholesky) is not implemented; use None (0), Jacobi (1) or "
                    "RegularizedCholesky (3).\n", opt.preconditioner);
    return;
  }
  if (opt.rescale != 0 && opt.rescale != 1) {
    fprintf(stderr, "[dpgo_amd] ERROR: rescale must be 0 (Static) or 1 (Dynamic).\n");
    return;
  }
  {
    std::set<int> uniq(node_ids.begin(), node_ids.end());
    if (uniq.size() != node_ids.size()) {
      fprintf(stderr, "[dpgo_amd] ERROR: a node appears twice in the group.\n");
      return;
    }
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    fprintf(stderr, "[dpgo_amd] ERROR: no HIP device available; the DPGO hot path has no CPU fallback.\n");
    return;
  }
  HIP_CHECK(hipSetDevice(device));
  const int L = (int)nodes_.size();
  const bool trivial = (opt.loss == 0);
  info_.resize(L);
  ops_.resize(L);
  scale_.assign(L, {});
  rescale_count_.assign(L, 0);
  res_.assign(L, NodeResults());
  lambda_max_.assign(L, 0.0);
  g_index_.resize(L);
  own_off_.assign(L + 1, 0);
  nbr_off_.assign(L + 1, 0);
  for (int a = 0; a < L; a++) {
    local_of_node_[nodes_[a]] = a;
    if (generate_data_info(nodes_[a], d_, g.measurements[nodes_[a]], info_[a]) != 0) return;
    // Rescale::Dynamic (robust losses): one scale per inter-node edge, all ones at construction (DPGOProblem.cpp:34)
    if (!trivial && opt.rescale == 1) scale_[a].assign(info_[a].inter.size(), 1.0);
    g_index_[a] = g.g_index[nodes_[a]];
    own_off_[a + 1] = own_off_[a] + info_[a].n[0];
    nbr_off_[a + 1] = nbr_off_[a] + info_[a].n[1];
  }
  P0_ = own_off_[L];
  P1_ = nbr_off_[L];
  {   // the operators of the nodes, one host thread per node
    int bad = 0;
#pragma omp parallel for schedule(dynamic, 1) num_threads(std::max(1, std::min(L, host_threads()))) reduction(+ : bad)
    for (int a = 0; a < L; a++)
      bad += assemble_node(info_[a], opt.regularizer, trivial, ops_[a], scale_[a].empty() ? nullptr : scale_[a].data()) != 0;
    if (bad) return;
  }
  auto uni = [&](int a, int p) { return p < info_[a].n[0] ? own_off_[a] + p : P0_ + nbr_off_[a] + (p - info_[a].n[0]); };

  // ---- segments
  {
    std::vector<Seg> segs;
    std::vector<int> optr(L + 1, 0), nptr(L + 1, 0);
    for (int a = 0; a < L; a++) {
      for (int r = own_off_[a]; r < own_off_[a + 1]; r += SEG_ROWS)
        segs.push_back({r, std::min(r + SEG_ROWS, own_off_[a + 1]), a, 0});
      optr[a + 1] = (int)segs.size();
    }
    const int nown = (int)segs.size();
    for (int a = 0; a < L; a++) {
      nptr[a] = (int)segs.size();
      for (int r = nbr_off_[a]; r < nbr_off_[a + 1]; r += SEG_ROWS)
        segs.push_back({P0_ + r, P0_ + std::min(r + SEG_ROWS, nbr_off_[a + 1]), a, 0});
    }
    nptr[L] = (int)segs.size();
    // nbr_ptr is used as [nptr[a], nptr[a+1]) : make it monotone per node
    segs_.upload(segs);
    own_seg_ptr_.upload(optr);
    own_seg_ptr_host_ = optr;
    nbr_seg_ptr_.upload(nptr);
    T_.segs = segs_.p;
    T_.nseg_own = nown;
    T_.nseg_all = (int)segs.size();
    T_.rows_own = P0_;
    T_.rows_all = P0_ + P1_;
    T_.own_ptr = own_seg_ptr_.p;
    T_.nbr_ptr = nbr_seg_ptr_.p;
  }
  if (L > MAX_LOCAL_NODES) {
    fprintf(stderr, "[dpgo_amd] ERROR: a group hosts at most %d nodes (%d requested).\n", MAX_LOCAL_NODES, L);
    return;
  }
  cur_mask_ = ALL_NODES;
  // pinned: [scalars of k_reduce | the schedule's flag | CG summaries | TNT summaries | rescale decisions | update()'s sums | gate]
  const size_t nsc = (size_t)std::max(L, 1) * MAX_SLOTS;
  sched_.open(nsc, (size_t)std::max(L, 1) * (CG_SUMMARY + TNT_SUMMARY + 1) + nsc + 8, P0_, L);
  st_ = sched_.stream();
  h_scal_ = sched_.pinned_front();
  h_cg_ = sched_.pinned_back();
  h_tnt_ = h_cg_ + (size_t)std::max(L, 1) * CG_SUMMARY;
  h_rs_ = h_tnt_ + (size_t)std::max(L, 1) * TNT_SUMMARY;
  h_upd_ = h_rs_ + std::max(L, 1);   // update()'s sums have a block of their own: the next refinement's sums may arrive before the host has read them
  h_gate_ = h_upd_ + nsc;            // the verdict of k_reduce_gate (group.h: SpecUpdate)
  h_gate_[0] = -1.0;
  for (int i = 0; i < std::max(L, 1) * (CG_SUMMARY + TNT_SUMMARY + 1); i++) h_cg_[i] = 0.0;
  fused_ = settings().fused;
  partials_.alloc((size_t)MAX_SLOTS * std::max(T_.nseg_all, 1));
  cg_.alloc(MAX_LOCAL_NODES);
  dmask_.alloc(4);
  go_.alloc(1);
  dev_sums_.alloc((size_t)MAX_LOCAL_NODES * MAX_SLOTS);
  dev_tnt_.alloc((size_t)MAX_LOCAL_NODES * TNT_SUMMARY);
  spec_update_enabled_ = settings().spec_update;
  coefs_dev_.alloc(MAX_LOCAL_NODES);

  upload_operators();
  // ---- inter-node edges (residual form) and their incidence lists
  {
    std::vector<int> tail, head;
    std::vector<double> R, t, kap, tau;
    std::vector<std::vector<int>> inc(P0_ + P1_);
    e_off_.assign(L + 1, 0);
    for (int a = 0; a < L; a++) e_off_[a + 1] = e_off_[a] + (int)info_[a].inter.size();
    for (int a = 0; a < L; a++)
      for (const auto &m : info_[a].inter) {
        const int e = (int)tail.size();
        const int p = uni(a, info_[a].tail(m)), q = uni(a, info_[a].head(m));
        tail.push_back(p); head.push_back(q);
        for (int k = 0; k < d_ * d_; k++) R.push_back(m.R[k]);
        for (int k = 0; k < d_; k++) t.push_back(m.t[k]);
        kap.push_back(m.kappa); tau.push_back(m.tau);
        inc[p].push_back(2 * e); inc[q].push_back(2 * e + 1);
      }
    std::vector<int> iptr(P0_ + P1_ + 1, 0), iv;
    for (int r = 0; r < P0_ + P1_; r++) {
      iptr[r + 1] = iptr[r] + (int)inc[r].size();
      iv.insert(iv.end(), inc[r].begin(), inc[r].end());
    }
    e_tail_.upload(tail); e_head_.upload(head); e_R_.upload(R); e_t_.upload(t); e_kappa_.upload(kap);
    e_tau_.upload(tau); e_inc_ptr_.upload(iptr); e_inc_.upload(iv);
    {
      // one 128-byte record per incidence, in the order of the incidence lists (kernels.h: InterInc)
      std::vector<InterInc> rec(std::max<size_t>(iv.size(), 1));
      std::memset(rec.data(), 0, sizeof(InterInc) * rec.size());
      for (size_t k = 0; k < iv.size(); k++) {
        const int e = iv[k] >> 1, role = iv[k] & 1;
        InterInc &r = rec[k];
        r.other = role ? tail[e] : head[e];
        r.osrc = -1;
        r.code = iv[k];
        r.tau = tau[e]; r.kappa = kap[e];
        for (int i = 0; i < d_; i++) r.t[i] = t[(size_t)e * d_ + i];
        for (int i = 0; i < d_ * d_; i++) r.R[i] = R[(size_t)e * d_ * d_ + i];
      }
      e_rec_.upload(rec);
      e_rec_host_ = rec;
      E_.rec = e_rec_.p;
    }
    E_.nrows_own = P0_; E_.nrows_all = P0_ + P1_;
    E_.m = (int)tail.size(); E_.tail = e_tail_.p; E_.head = e_head_.p; E_.R = e_R_.p; E_.t = e_t_.p;
    E_.kappa = e_kappa_.p; E_.tau = e_tau_.p; E_.inc_ptr = e_inc_ptr_.p; E_.inc = e_inc_.p;
    if (dynamic()) {
      e_w_.alloc(std::max<size_t>(tail.size(), 1));
      e_scale_.upload(std::vector<double>(std::max<size_t>(tail.size(), 1), 1.0));   // all ones at construction (DPGOProblem.cpp:34)
      e_off_dev_.upload(e_off_);
      rs_count_.alloc(std::max(L, 1));
      rs_flags_.alloc(std::max(L, 1));
    }
  }
  {
    std::vector<int> tail, head;
    std::vector<double> R, t, kap, tau;
    std::vector<std::vector<int>> inc(P0_);
    for (int a = 0; a < L; a++)
      for (const auto &m : info_[a].intra) {
        const int e = (int)tail.size();
        const int p = uni(a, info_[a].tail(m)), q = uni(a, info_[a].head(m));
        tail.push_back(p); head.push_back(q);
        for (int k = 0; k < d_ * d_; k++) R.push_back(m.R[k]);
        for (int k = 0; k < d_; k++) t.push_back(m.t[k]);
        kap.push_back(m.kappa); tau.push_back(m.tau);
        inc[p].push_back(2 * e);
      }
    std::vector<int> iptr(P0_ + 1, 0), iv;
    for (int r = 0; r < P0_; r++) {
      iptr[r + 1] = iptr[r] + (int)inc[r].size();
      iv.insert(iv.end(), inc[r].begin(), inc[r].end());
    }
    i_tail_.upload(tail); i_head_.upload(head); i_R_.upload(R); i_t_.upload(t); i_kappa_.upload(kap);
    i_tau_.upload(tau); i_inc_ptr_.upload(iptr); i_inc_.upload(iv);
    Ei_.nrows_own = P0_; Ei_.nrows_all = P0_;
    Ei_.m = (int)tail.size(); Ei_.tail = i_tail_.p; Ei_.head = i_head_.p; Ei_.R = i_R_.p; Ei_.t = i_t_.p;
    Ei_.kappa = i_kappa_.p; Ei_.tau = i_tau_.p; Ei_.inc_ptr = i_inc_ptr_.p; Ei_.inc = i_inc_.p;
  }
  // ---- SPD solvers: one block-diagonal system over all local nodes
  if (refactor_tt() != 0) return;
  if (dynamic() && Ltt_.F.numeric) setup_device_rescale();
  {
    SetupClock clk;
    CsrMatrix Arr;
    Arr.ptr.push_back(0);
    for (int a = 0; a < L; a++) {
      if (opt.preconditioner == 3 && opt.max_iterations > 0 && opt.max_iterations_accepted > 0) {
        const CsrMatrix &r = ops_[a].GRR;
        lambda_max_[a] = lanczos_lambda_max(r);
        const double shift = lambda_max_[a] / opt.reg_Cholesky_precon_max_condition_number;  // DPGOProblem.cpp:119-123
        for (int i = 0; i < r.n; i++) {
          for (int e = r.ptr[i]; e < r.ptr[i + 1]; e++) {
            Arr.col.push_back(own_off_[a] * d_ + r.col[e]);
            Arr.val.push_back(r.val[e] + (r.col[e] == i ? shift : 0.0));
          }
          Arr.ptr.push_back((int)Arr.col.size());
        }
      }
    }
    Arr.n = (int)Arr.ptr.size() - 1;
    clk.lap("G_RR: lambda_max (Lanczos) + shifted matrix");
    if (Arr.n > 0) {
      const Settings &s = settings();
      if (spd_factor(Arr, Lrr_.F, s.spd_leaf_rr, s.spd_collapse_rr, s.spd_quotient ? d_ : 1, s.spd_device_panels) != 0) return;
      clk.lap("G_RR: ordering + symbolic + numeric factor");
      warn_conditioning("G_RR + lambda I", Lrr_.F);
      std::vector<int> node_of_row((size_t)P0_ * d_);
      for (int a = 0; a < L; a++)
        for (int p = 0; p < info_[a].n[0] * d_; p++) node_of_row[(size_t)own_off_[a] * d_ + p] = a;
      Lrr_.upload(d_, d_, node_of_row);
      clk.lap("G_RR: panels (pack + upload)");
    }
  }
  if (opt.preconditioner == 1) {   // Preconditioner::Jacobi: diag(G_RR)^-1, fixed at construction (DPGOProblem.cpp:96-98)
    std::vector<double> dinv((size_t)P0_ * d_, 1.0);
    for (int a = 0; a < L; a++) {
      const CsrMatrix &r = ops_[a].GRR;
      for (int i = 0; i < r.n; i++)
        for (int e = r.ptr[i]; e < r.ptr[i + 1]; e++)
          if (r.col[e] == i) dinv[(size_t)own_off_[a] * d_ + i] = 1.0 / r.val[e];
    }
    jacobi_.upload(dinv);
  }
  // ---- halo lists
  {
    std::vector<int> gdst, gsrc;
    std::set<std::pair<int, int>> sent;
    for (int a = 0; a < L; a++) {
      for (int k = 0; k < info_[a].n[1]; k++) {
        const auto key = info_[a].nbr_key[k];
        auto it = local_of_node_.find(key.first);
        if (it != local_of_node_.end()) {
          gdst.push_back(P0_ + nbr_off_[a] + k);
          gsrc.push_back(own_off_[it->second] + info_[it->second].index.at(key));
        }
      }
      for (const auto &s : info_[a].sent)
        if (!local_of_node_.count(s.first))
          for (int row : s.second) sent.insert({nodes_[a], row});
    }
    gather_dst_.upload(gdst);
    gather_src_.upload(gsrc);
    for (const auto &s : sent) {
      const int a = local_of_node_.at(s.first);
      sent_rows_.push_back(own_off_[a] + s.second);
      sent_keys_.push_back({s.first, info_[a].own_pose[s.second]});
    }
    sent_rows_dev_.upload(sent_rows_);
  }
  // ---- vectors
  const size_t nall = (size_t)(P0_ + P1_) * RS_, nown = (size_t)P0_ * RS_;
  for (DevBuf<double> *b : {&Xk_, &Zc_, &Zp_, &Y_, &DfE_, &Tall_}) b->alloc(nall);
  for (DevBuf<double> *b : {&Xak_, &Xakh_, &gc_, &gp_, &Dfc_, &Dfp_, &gx_, &Dfx_, &T1_}) b->alloc(nown);
  if (keep_gx()) { GXc_.alloc(nown); GXp_.alloc(nown); }
  for (auto &b : tmp_) b.alloc(nown);
  if (settings().spd_dump) {
    spd_profile(d_, st_, Ltt_, T1_.p);
    if (Lrr_.F.n > 0) spd_profile(d_, st_, Lrr_, T1_.p);
    HIP_CHECK(hipMemsetAsync(T1_.p, 0, sizeof(double) * nown, st_));
  }
  HIP_CHECK(hipDeviceSynchronize());
  ok_ = true;
}

// The operators of every local node on the device (block-CSR G, S, P, P0, Q; the per-pose arrays D, T, N, V, robust Q).
// Called at construction and after a Dynamic rescale.
void Group::upload_operators() {
  sched_.invalidate();   // (captured launches carry the operators' addresses)
  const int L = num_local();
  const bool trivial = (opt_.loss == 0);
  auto uni = [&](int a, int p) { return p < info_[a].n[0] ? own_off_[a] + p : P0_ + nbr_off_[a] + (p - info_[a].n[0]); };
    std::vector<const BsrMatrix *> v(L);
    for (int a = 0; a < L; a++) v[a] = &ops_[a].G;
    upload_bsr(v, false, G_);
    if (trivial) {
      for (int a = 0; a < L; a++) v[a] = &ops_[a].S;
      upload_bsr(v, false, S_);
      for (int a = 0; a < L; a++) v[a] = &ops_[a].P;
      upload_bsr(v, true, P_);
      for (int a = 0; a < L; a++) v[a] = &ops_[a].P0;
      upload_bsr(v, true, P0m_);
      for (int a = 0; a < L; a++) v[a] = &ops_[a].Q;
      upload_bsr(v, true, Q_);
    }
    std::vector<double> Dd((size_t)P0_ * B_ * B_), Ti(P0_), Nn((size_t)P0_ * d_), Vv((size_t)P0_ * d_ * d_);
    std::vector<double> Qd((size_t)(P0_ + P1_) * B_ * B_, 0.0);
    for (int a = 0; a < L; a++) {
      const int n0 = info_[a].n[0];
      std::copy(ops_[a].D.begin(), ops_[a].D.end(), Dd.begin() + (size_t)own_off_[a] * B_ * B_);
      std::copy(ops_[a].Tinv.begin(), ops_[a].Tinv.end(), Ti.begin() + own_off_[a]);
      std::copy(ops_[a].N.begin(), ops_[a].N.end(), Nn.begin() + (size_t)own_off_[a] * d_);
      std::copy(ops_[a].V.begin(), ops_[a].V.end(), Vv.begin() + (size_t)own_off_[a] * d_ * d_);
      if (!trivial) {   // robust Q is block diagonal
        const BsrMatrix &Q = ops_[a].Q;
        for (int r = 0; r < Q.nrows; r++)
          for (int k = Q.ptr[r]; k < Q.ptr[r + 1]; k++)
            if (Q.col[k] == r)
              std::copy(&Q.val[(size_t)k * B_ * B_], &Q.val[(size_t)(k + 1) * B_ * B_],
                        Qd.begin() + (size_t)uni(a, r) * B_ * B_);
      }
      (void)n0;
    }
    Dd_.upload(Dd); Tinv_.upload(Ti); N_.upload(Nn); V_.upload(Vv); Qd_.upload(Qd);
}

// Factor G_tt of all local nodes (block diagonal): L_.compute / L_.factorize (DPGOProblem.cpp:93, 315, 479)
int Group::refactor_tt() {
  const int L = num_local();
  CsrMatrix Att;
  Att.ptr.push_back(0);
  for (int a = 0; a < L; a++) {
    const CsrMatrix &t = ops_[a].Gtt;
    for (int i = 0; i < t.n; i++) {
      for (int e = t.ptr[i]; e < t.ptr[i + 1]; e++) { Att.col.push_back(own_off_[a] + t.col[e]); Att.val.push_back(t.val[e]); }
      Att.ptr.push_back((int)Att.col.size());
    }
  }
  Att.n = (int)Att.ptr.size() - 1;
  SetupClock clk;
  // Rescale::Dynamic re-factors G_tt every few iterations: the numeric phase keeps its device state, and the values it
  // reads stay on the GPU where k_rescale_apply rewrites the diagonal (att_pos_: where each pose's diagonal entry is)
  const Settings &s = settings();
  const bool keep = dynamic() && !s.rescale_host && s.spd_device_panels && !s.spd_host_factor;
  Ltt_.F.keep_numeric = keep;
  if (keep && att_pos_.n == 0) {
    std::vector<int> pos(std::max(Att.n, 1), 0);
    for (int i = 0; i < Att.n; i++)
      for (int e = Att.ptr[i]; e < Att.ptr[i + 1]; e++)
        if (Att.col[e] == i) pos[i] = e;
    att_pos_.upload(pos);
  }
  if (Ltt_.F.n == Att.n && Ltt_.F.nfronts > 0 && !Ltt_.F.children.empty()) {
    // same pattern, new values (a Dynamic rescale): numeric phase only, on the GPU
    if (spd_refactor(Att, Ltt_.F) != 0) return -1;
  } else {
    // A factor that is re-done in every iteration (Dynamic) is ordered for the refactorisation, not for the three solves
    // it serves: small leaves and NO merged levels keep the fronts at the top of the trees narrow, and the chain of
    // dependent block columns there -- 33 at the merged roots of the headline, two launches each -- is what a
    // refactorisation costs (5.29 -> 4.17 ms per iteration at the headline size; the cost model of
    // spd_factor knows solves only).
    const int leaf = s.spd_leaf_tt.value_or(keep ? 64 : 128), collapse = s.spd_collapse_tt.value_or(keep ? 1 : 0);
    if (spd_factor(Att, Ltt_.F, leaf, collapse, 1, s.spd_device_panels) != 0) return -1;
  }
  clk.lap("G_tt: ordering + symbolic + numeric factor");
  warn_conditioning("G_tt", Ltt_.F);
  std::vector<int> node_of_pose(P0_);
  for (int a = 0; a < L; a++)
    for (int p = 0; p < info_[a].n[0]; p++) node_of_pose[own_off_[a] + p] = a;
  sched_.invalidate();   // (... and the panels')
  Ltt_.upload(1, d_, node_of_pose);
  clk.lap("G_tt: panels (pack + upload)");
  return 0;
}

Group::~Group() {
  if (sched_.host_timing()) {
    sched_.report_launches(num_local());
    fprintf(stderr, "[host] updates enqueued ahead of the host's decision: %ld, of which the decision let stand: %ld\n", n_spec_enqueued_, n_spec_stood_);
    sched_.report_waits();
  }
  // A replay may still be running, a kernel may still write the pinned block: the schedule waits for the stream with a bound
  // before any buffer goes, and leaks what the device might still touch where it never drains (schedule.h: close)
  sched_.close(failed_ ? 2.0 : 60.0);
  chordal_release();
  stair_release();
  robust_release();
  ml_release();
  marg_release();
  cov_release();
  cert_release();
}

void Group::upload_bsr(const std::vector<const BsrMatrix *> &per_node, bool rows_all, BsrBufs &out) {
  const int L = (int)per_node.size();
  const int nrows = rows_all ? P0_ + P1_ : P0_;
  auto uni = [&](int a, int p) { return p < info_[a].n[0] ? own_off_[a] + p : P0_ + nbr_off_[a] + (p - info_[a].n[0]); };
  std::vector<int> cnt(nrows, 0);
  for (int a = 0; a < L; a++)
    for (int r = 0; r < per_node[a]->nrows; r++) cnt[uni(a, r)] = per_node[a]->ptr[r + 1] - per_node[a]->ptr[r];
  std::vector<int> ptr(nrows + 1, 0);
  for (int r = 0; r < nrows; r++) ptr[r + 1] = ptr[r] + cnt[r];
  std::vector<int> col(ptr[nrows]);
  std::vector<double> val((size_t)ptr[nrows] * B_ * B_);
  for (int a = 0; a < L; a++) {
    const BsrMatrix &M = *per_node[a];
    for (int r = 0; r < M.nrows; r++) {
      int dst = ptr[uni(a, r)];
      for (int k = M.ptr[r]; k < M.ptr[r + 1]; k++, dst++) {
        col[dst] = uni(a, M.col[k]);
        std::copy(&M.val[(size_t)k * B_ * B_], &M.val[(size_t)(k + 1) * B_ * B_], &val[(size_t)dst * B_ * B_]);
      }
    }
  }
  out.ptr.upload(ptr);
  out.col.upload(col);
  if (&out == &G_) {   // compact copy of the translation column for launch_bsr_tcol
    std::vector<double> tc((size_t)ptr[nrows] * B_);
    for (size_t k = 0; k < (size_t)ptr[nrows]; k++)
      for (int r = 0; r < B_; r++) tc[k * B_ + r] = val[k * B_ * B_ + (size_t)r * B_];
    out.tcol.upload(tc);
  }
  {
    // k_bsr gives a block row to BSR_LPR lanes, lane j taking blocks j, j + BSR_LPR, ... of the row.  The values of the (up
    // to) BSR_LPR blocks one round reads are stored interleaved in 16-byte pieces (8-byte for the 3 x 3 blocks of SE(2)):
    // piece p of lane j at ((p * cnt + j) * PS), so that the quad's loads of one instruction are contiguous
    const int BB = B_ * B_, PS = BB % 2 == 0 ? 2 : 1;
    std::vector<double> il(val.size());
    for (int r = 0; r < nrows; r++)
      for (int k0 = ptr[r]; k0 < ptr[r + 1]; k0 += BSR_LPR) {
        const int cnt = std::min(BSR_LPR, ptr[r + 1] - k0);
        for (int j = 0; j < cnt; j++)
          for (int e = 0; e < BB; e++)
            il[(size_t)k0 * BB + (size_t)((e / PS) * cnt + j) * PS + e % PS] = val[(size_t)(k0 + j) * BB + e];
      }
    out.val.upload(il);
  }
  out.dev.nrows = nrows;
  out.dev.nnzb = ptr[nrows];
  out.dev.ptr = out.ptr.p;
  out.dev.col = out.col.p;
  out.dev.val = out.val.p;
}

void Group::sync() const {
  const_cast<Group *>(this)->flush_pending_recv();   // (whoever reads Xk next must find the neighbour rows in it)
  if (xchg_done_) HIP_CHECK(hipEventSynchronize(xchg_done_));   // an exchange on the communicator's stream
  HIP_CHECK(hipStreamSynchronize(st_));
  check_tt_verdict(false);
}

void Group::check_tt_verdict(bool wait) const {
  if (!tt_verdict_pending_) return;
  tt_verdict_pending_ = false;
  // (DPGO_DEBUG_FAIL_REFACTOR=1, a test hook: the verdict counts as "not positive definite")
  if (spd_refactor_finish(const_cast<SpdFactor &>(Ltt_.F), wait) != 0 || settings().debug_fail_refactor) {
    failed_ = true;
    fprintf(stderr, "[dpgo_amd] ERROR: G_tt is not positive definite after a rescale; the group cannot go on (create a new one).\n");
    throw DeviceError("G_tt is not positive definite after a rescale");
  }
}

// The nodes the following launches work on: a bit mask passed to every kernel by value (no upload).
void Group::set_mask(const std::vector<int> &locals) {
  NodeBits m = 0;
  for (int a : locals) m |= 1ull << a;
  cur_mask_ = live_mask(m, nullptr);
}

NodeMask Group::live_mask(NodeBits bits, const NodeBits *p) const {
  NodeMask m{bits, p};
  const int L = num_local();
  int n = 0, idle = -1;
  if ((int)own_seg_ptr_host_.size() != L + 1) return m;
  for (int a = 0; a < L; a++) {
    if ((bits >> a) & 1ull) n++;
    // (the surplus workgroups of the launch land on the idle node's FIRST segment and leave at once: it must be a segment
    // of that node -- a node without own rows has none, its "first" one would be the next node's)
    else if (idle < 0 && own_seg_ptr_host_[a + 1] > own_seg_ptr_host_[a]) idle = a;
  }
  if (n == 0 || n > MAX_LIVE_SEGS || idle < 0) return m;   // (every node, too many, or nowhere to park: the whole grid)
  for (int a = 0; a < L; a++)
    if ((bits >> a) & 1ull) {
      m.seg0[m.nlive] = own_seg_ptr_host_[a];
      m.nseg[m.nlive] = own_seg_ptr_host_[a + 1] - own_seg_ptr_host_[a];
      m.nlive++;
    }
  m.idle_seg = own_seg_ptr_host_[idle];
  return m;
}

// The segments of an iteration (group.h): the key of a replay is built here, the schedule runs it
void Group::segment(int id, NodeBits bits, std::initializer_list<unsigned long long> extra, const std::function<void()> &body,
                    int wanted) {
  if (sched_.capturing()) { body(); return; }   // (a segment inside a segment is part of it)
  if (!(wanted < 0 ? sched_.iter_graph_wanted() : wanted != 0) || bits != all_bits()) {
    sched_.segment(nullptr, body);
    return;
  }
  std::vector<unsigned long long> key;
  key.reserve(16 + extra.size());
  key.push_back((unsigned long long)id);
  key.push_back(sched_.graph_gen());
  // the buffers that rotate with the history or swap with an accepted step
  for (const DevBuf<double> *b : {&Zc_, &Zp_, &gc_, &gp_, &Dfc_, &Dfp_, &GXc_, &GXp_, &Xak_, &tmp_[7]})
    key.push_back((unsigned long long)(uintptr_t)b->p);
  key.insert(key.end(), extra.begin(), extra.end());
  key.push_back(sched_.deferred_key());   // (the launches that become the segment's head)
  sched_.segment(&key, body);
}

unsigned long long Group::fetch_async(int nslots, bool all_rows) {
  finish_update();   // (its scalars sit in the pinned slots the next reduction overwrites)
  nslots = take_deferred_slots(nslots);
  launch_reduce(st_, T_, num_local(), all_rows, nslots, partials_.p, h_scal_, sched_.flag());
  return sched_.last_seq();   // (under capture: the schedule adds the replay's flags itself, Schedule::segment())
}

void Group::fetch(int nslots, bool all_rows) { wait_flag(fetch_async(nslots, all_rows)); }

void Group::wait_flag(unsigned long long seq) {
  sched_.wait(seq);
  if (tt_verdict_pending_ && seq >= tt_verdict_seq_) check_tt_verdict(false);   // (the stream has passed the factorisation)
  if (spec_verdict_pending_ && seq >= spec_verdict_seq_) {   // (... and the gate of a speculative update)
    spec_verdict_pending_ = false;
    const double v = h_gate_[0];
    if ((v == 1.0) != spec_verdict_expected_) {
      failed_ = true;
      fprintf(stderr, "[dpgo_amd] ERROR: the device-side gate of the speculative update (%.0f) and the host (%d) disagree; the group cannot go on.\n",
              v, (int)spec_verdict_expected_);
      throw DeviceError("gate / host verdicts differ");
    }
  }
}

void Group::copy_rows(double *dst, const double *src, bool all_rows, int part) {
  launch_axpby(lc(), all_rows, 1.0, src, 0.0, nullptr, dst, part);
}

// (fronts of nodes outside the current mask are skipped: their entries of `out` stay as they are)
void Group::solve_tt(double *in, double *out, double scale) { spd_run(d_, st_, Ltt_, cur_mask_, in, out, scale, class_tt_); }
void Group::solve_rr(double *in, double *out, double scale) { spd_run(d_, st_, Lrr_, cur_mask_, in, out, scale, class_rr_); }

// X.t = -G_tt^-1 (g_t + G_tR X.R)    (DPGOProblem.h:275-294)
// Leaves T1_ = G [0 ; X.R] + g on all rows (its translation rows are the right-hand side of the solve):
// with the new translations, G X + g = T1_ + G_{:,t} X.t, which launch_bsr_tcol() adds at a quarter of the
// cost of another G X.
void Group::recover_translations(double *X, const double *g) {
  launch_bsr(lc(), G_.dev, {.x = X, .mode = BsrMode::NoTrans, .addv = g, .y = T1_.p});
  solve_tt(T1_.p, X, -1.0);
}

// partial[slot] = tr(X^T (g + 1/2 G X))     (DPGOProblem.cpp:180-205; + f on the host)
void Group::eval_G(const double *X, const double *g, int slot) {
  launch_bsr(lc(), G_.dev, {.x = X, .dot = {.v = X, .coef = 0.5, .add = g, .partials = partials_.p, .slot = slot}});
}

// ---------------------------------------------------------------------------
// layout conversion (reference column-major <-> pose records)
// ---------------------------------------------------------------------------
static void to_records(int d, int n, const double *X, int ld, int row_t0, int row_r0, double *rec) {
  // X rows [row_t0, row_t0+n) translations, [row_r0 + d k, ...) rotation blocks
  const int RS = (d + 1) * d;
  for (int k = 0; k < n; k++)
    for (int c = 0; c < d; c++) {
      rec[(size_t)k * RS + c] = X[(size_t)c * ld + row_t0 + k];
      for (int r = 0; r < d; r++) rec[(size_t)k * RS + d + r * d + c] = X[(size_t)c * ld + row_r0 + k * d + r];
    }
}
static void from_records(int d, int n, const double *rec, double *X, int ld, int row_t0, int row_r0) {
  const int RS = (d + 1) * d;
  for (int k = 0; k < n; k++)
    for (int c = 0; c < d; c++) {
      X[(size_t)c * ld + row_t0 + k] = rec[(size_t)k * RS + c];
      for (int r = 0; r < d; r++) X[(size_t)c * ld + row_r0 + k * d + r] = rec[(size_t)k * RS + d + r * d + c];
    }
}

int Group::initialize(int a, const double *X, int ld) {
  finish_update();
  zc_ready_ = false;   // (whatever an earlier iterate() left in the history buffers is overwritten here)
  packed_ = false;     // (... and whatever it packed for an exchange)
  if (a < 0 || a >= num_local()) return -1;
  const int n0 = info_[a].n[0], n1 = info_[a].n[1];
  if (ld < (d_ + 1) * (n0 + n1)) {
    fprintf(stderr, "[dpgo_amd] ERROR: initialize: inconsistent size of X for node %d.\n", nodes_[a]);
    return -1;
  }
  sync();
  std::vector<double> own((size_t)n0 * RS_), nbr((size_t)std::max(n1, 1) * RS_);
  to_records(d_, n0, X, ld, 0, n0, own.data());
  to_records(d_, n1, X, ld, (d_ + 1) * n0, (d_ + 1) * n0 + n1, nbr.data());
  for (double *dst : {Xk_.p, Zc_.p, Zp_.p}) {
    HIP_CHECK(hipMemcpy(dst + (size_t)own_off_[a] * RS_, own.data(), sizeof(double) * n0 * RS_, hipMemcpyHostToDevice));
    if (n1) HIP_CHECK(hipMemcpy(dst + (size_t)(P0_ + nbr_off_[a]) * RS_, nbr.data(), sizeof(double) * n1 * RS_, hipMemcpyHostToDevice));
  }
  HIP_CHECK(hipMemcpy(Xak_.p + (size_t)own_off_[a] * RS_, own.data(), sizeof(double) * n0 * RS_, hipMemcpyHostToDevice));
  for (double *dst : {gc_.p, gp_.p, Dfc_.p, Dfp_.p})
    HIP_CHECK(hipMemset(dst + (size_t)own_off_[a] * RS_, 0, sizeof(double) * n0 * RS_));
  res_[a] = NodeResults();
  res_[a].updated = 0;
  spec_refined_ = false;   // (a fresh start: nothing to guess the next iteration's refinements from)
  rescale_count_[a] = 0;   // DPGOResult::clear (DPGO_types.h:301); the scales belong to the problem and stay
  if (device_rescale_) HIP_CHECK(hipMemset(rs_count_.p + a, 0, sizeof(int)));
  return 0;
}

// Rows of a global X ((d+1)N x d, reference layout) that node a works on, as a (d+1)(n0+n1) x d matrix Z in
// the node's own ordering (dist_pgo.cpp:435-446 + DPGO::communicate)
void Group::node_rows_of_global(int a, const double *X, int ld, std::vector<double> &Z) const {
  const int N = num_poses_global_;
  const int n0 = info_[a].n[0], n1 = info_[a].n[1], rows = (d_ + 1) * (n0 + n1);
  Z.assign((size_t)rows * d_, 0.0);
  auto put = [&](int trow, int rrow, int gid) {
    for (int c = 0; c < d_; c++) {
      Z[(size_t)c * rows + trow] = X[(size_t)c * ld + gid];
      for (int r = 0; r < d_; r++) Z[(size_t)c * rows + rrow + r] = X[(size_t)c * ld + N + gid * d_ + r];
    }
  };
  for (int k = 0; k < n0; k++) put(k, n0 + k * d_, g_index_[a].at(info_[a].own_pose[k]));
  // neighbours: global id from the partition rule (DPGO_utils.cpp:147-158)
  const int q = N / num_nodes_total_, inc_n = N - num_nodes_total_ * q;
  for (int k = 0; k < n1; k++) {
    const int node = info_[a].nbr_key[k].first, pose = info_[a].nbr_key[k].second;
    const int start = node < inc_n ? node * (q + 1) : inc_n * (q + 1) + (node - inc_n) * q;
    put((d_ + 1) * n0 + k, (d_ + 1) * n0 + n1 + k * d_, start + pose);
  }
}

int Group::initialize_global(const double *X, int ld) {
  finish_update();
  const int N = num_poses_global_;
  if (ld < (d_ + 1) * N) return -1;
  std::vector<double> Z;
  for (int a = 0; a < num_local(); a++) {
    node_rows_of_global(a, X, ld, Z);
    if (initialize(a, Z.data(), (d_ + 1) * (info_[a].n[0] + info_[a].n[1])) != 0) return -1;
  }
  return 0;
}

// DPGOStar::evaluate_f / evaluate_grad at an arbitrary global X (C++/DPGO/src/DPGOStar.cpp:713-829), without
// touching the optimizer state.  Every node evaluates its intra edges and its inter edges (objective: charged 1/2
// per node; gradient: the rows of its own poses, which are DfobjE_top + (G - D) X = g + G X);
// F and |grad F|^2 are the sums over the nodes of this group, and over all groups when collectives are set.
// grad (optional): global (d+1)N x d, only the rows of this group's own poses are written.
int Group::evaluate_global(const double *X, int ld, double *F, double *grad_sqnorm, double *grad, int ldg) {
  finish_update();
  const int N = num_poses_global_;
  if (ld < (d_ + 1) * N || (grad && ldg < (d_ + 1) * N)) {
    fprintf(stderr, "[dpgo_amd] ERROR: evaluate: inconsistent size of X.\n");
    return -1;
  }
  join_exchange();
  sync();
  {
    std::vector<double> rec((size_t)(P0_ + P1_) * RS_), Z;
    for (int a = 0; a < num_local(); a++) {
      node_rows_of_global(a, X, ld, Z);
      const int n0 = info_[a].n[0], n1 = info_[a].n[1], rows = (d_ + 1) * (n0 + n1);
      to_records(d_, n0, Z.data(), rows, 0, n0, rec.data() + (size_t)own_off_[a] * RS_);
      to_records(d_, n1, Z.data(), rows, (d_ + 1) * n0, (d_ + 1) * n0 + n1, rec.data() + (size_t)(P0_ + nbr_off_[a]) * RS_);
    }
    HIP_CHECK(hipMemcpy(Tall_.p, rec.data(), sizeof(double) * rec.size(), hipMemcpyHostToDevice));
  }
  std::vector<int> all(num_local());
  for (int a = 0; a < num_local(); a++) all[a] = a;
  set_mask(all);
  double *g = tmp_[0].p, *Df = tmp_[1].p, *gr = tmp_[2].p;
  if (opt_.loss == 0)   // g = S Z
    launch_bsr(lc(), S_.dev, {.x = Tall_.p, .y = g});
  else                  // g = (B1^T W B1 Z)_own - D X   (weights at X)
    launch_inter_iterate(lc(), E_, opt_.loss, opt_.loss_reg, {.Z = Tall_.p, .Ddiag = Dd_.p, .g = g, .partials = partials_.p});
  launch_bsr(lc(), G_.dev, {.x = Tall_.p, .addv = g, .y = Df});
  launch_cost(lc(), Ei_, E_, opt_.loss == 0, opt_.loss, opt_.loss_reg, Tall_.p, partials_.p, 0);
  launch_tangent_full(lc(), Tall_.p, Df, gr, partials_.p, 2);
  fetch(3, true);
  double v[2] = {0, 0};
  for (int a = 0; a < num_local(); a++) {
    v[0] += 0.5 * scal(a, 0) + 0.25 * scal(a, 1);
    v[1] += scal(a, 2);
  }
  if (coll_allreduce_ && coll_allreduce_(coll_user_, v, 2) != 0) return -1;
  if (F) *F = v[0];
  if (grad_sqnorm) *grad_sqnorm = v[1];
  if (grad) {
    std::vector<double> own((size_t)P0_ * RS_);
    HIP_CHECK(hipMemcpy(own.data(), gr, sizeof(double) * own.size(), hipMemcpyDeviceToHost));
    for (int a = 0; a < num_local(); a++)
      for (int k = 0; k < info_[a].n[0]; k++) {
        const int gid = g_index_[a].at(info_[a].own_pose[k]);
        const double *rec = &own[(size_t)(own_off_[a] + k) * RS_];
        for (int c = 0; c < d_; c++) {
          grad[(size_t)c * ldg + gid] = rec[c];
          for (int r = 0; r < d_; r++) grad[(size_t)c * ldg + N + gid * d_ + r] = rec[d_ + r * d_ + c];
        }
      }
  }
  return 0;
}

// DPGOHash::set_options (DPGOHash.h:93-96).  The reference swaps the optimizer's options and keeps the problem it
// built at construction; here the fields baked into the problem (operators, factorizations) must not change.
int Group::set_options(const Options &o) {
  finish_update();
  if (o.loss != opt_.loss || o.loss_reg != opt_.loss_reg || o.regularizer != opt_.regularizer || o.rescale != opt_.rescale ||
      o.preconditioner != opt_.preconditioner ||
      o.reg_Cholesky_precon_max_condition_number != opt_.reg_Cholesky_precon_max_condition_number) {
    fprintf(stderr, "[dpgo_amd] ERROR: set_options: loss, loss_reg, regularizer, rescale and the preconditioner are part of "
                    "the problem built at construction; create a new group to change them.\n");
    return -1;
  }
  if (o.preconditioner == 3 && Lrr_.F.n == 0 && o.max_iterations > 0 && o.max_iterations_accepted > 0) {
    fprintf(stderr, "[dpgo_amd] ERROR: set_options: the group was created without refinement (max_iterations = 0), so "
                    "the preconditioner was never factorised.\n");
    return -1;
  }
  opt_ = o;
  sched_.invalidate();   // (captured launches carry tolerances and iteration limits by value)
  spec_refined_ = false;
  return 0;
}

int Group::get_Xk(int a, double *X, int ld) const {
  if (a < 0 || a >= num_local()) return -1;
  sync();
  const int n0 = info_[a].n[0], n1 = info_[a].n[1];
  std::vector<double> own((size_t)n0 * RS_), nbr((size_t)std::max(n1, 1) * RS_);
  HIP_CHECK(hipMemcpy(own.data(), Xk_.p + (size_t)own_off_[a] * RS_, sizeof(double) * n0 * RS_, hipMemcpyDeviceToHost));
  if (n1) HIP_CHECK(hipMemcpy(nbr.data(), Xk_.p + (size_t)(P0_ + nbr_off_[a]) * RS_, sizeof(double) * n1 * RS_, hipMemcpyDeviceToHost));
  from_records(d_, n0, own.data(), X, ld, 0, n0);
  from_records(d_, n1, nbr.data(), X, ld, (d_ + 1) * n0, (d_ + 1) * n0 + n1);
  return 0;
}

int Group::get_X_own(int a, double *X, int ld) const {
  if (a < 0 || a >= num_local()) return -1;
  sync();
  const int n0 = info_[a].n[0];
  std::vector<double> own((size_t)n0 * RS_);
  HIP_CHECK(hipMemcpy(own.data(), Xak_.p + (size_t)own_off_[a] * RS_, sizeof(double) * n0 * RS_, hipMemcpyDeviceToHost));
  from_records(d_, n0, own.data(), X, ld, 0, n0);
  return 0;
}

int Group::scatter_global(double *X, int ld) const {
  sync();
  const int N = num_poses_global_;
  std::vector<double> own((size_t)P0_ * RS_);
  HIP_CHECK(hipMemcpy(own.data(), Xk_.p, sizeof(double) * P0_ * RS_, hipMemcpyDeviceToHost));
  for (int a = 0; a < num_local(); a++) {
    for (int k = 0; k < info_[a].n[0]; k++) {
      const int gid = g_index_[a].at(info_[a].own_pose[k]);
      const double *rec = &own[(size_t)(own_off_[a] + k) * RS_];
      for (int c = 0; c < d_; c++) {
        X[(size_t)c * ld + gid] = rec[c];
        for (int r = 0; r < d_; r++) X[(size_t)c * ld + N + gid * d_ + r] = rec[d_ + r * d_ + c];
      }
    }
  }
  return 0;
}

// ---------------------------------------------------------------------------
// halo exchange
// ---------------------------------------------------------------------------
int Group::communicate_local() {
  // neighbour rows whose owner lives in this group: one indexed device copy (DPGOHash.h:64-82)
  if (gather_dst_.n == 0) return 0;
  if (spec_upd_.on) return 0;   // (enqueued ahead, under the gate: speculate_update)
  if (pending_tail_.on) {
    // Xk's own rows are still on their way (they ride on the next update()'s product with G): the neighbour rows come
    // from Xak, which holds the same records
    const double *src = pending_tail_.xak;
    sched_.submit(0x6c6f63ull, [this, src] { launch_copy_indexed(d_, st_, (int)gather_dst_.n, gather_dst_.p, gather_src_.p, src, Xk_.p); });
    return 0;
  }
  sched_.submit(0x6c6f63ull, [this] { launch_copy_indexed(d_, st_, (int)gather_dst_.n, gather_dst_.p, gather_src_.p, Xk_.p, Xk_.p); });
  return 0;
}

int Group::step(const std::vector<int> &locals, const std::function<int()> &exchange) {
  struct Disarm {   // (whatever happens in between -- an error return, an exception on its way to the C ABI -- nothing stays deferred)
    Group *g;
    ~Disarm() { g->sched_.arm_defer(false); g->tail_fusable_ = false; g->spec_update_armed_ = false; g->pending_tail_.on = false; g->sched_.drop_deferred(); }
  } disarm{this};
  sched_.arm_defer(!exchange && sched_.iter_graph_wanted());
  tail_fusable_ = !exchange;
  spec_update_armed_ = !exchange;
  int rc = iterate(locals);
  tail_fusable_ = false;
  if (rc == 0 && exchange) rc = exchange();
  if (rc == 0) rc = communicate_local();
  sched_.arm_defer(false);
  if (rc == 0) rc = update(locals);
  flush_pending_tail();   // (nothing, unless update() had nothing to do)
  sched_.flush_deferred();
  return rc;
}

int Group::num_recv(int a, int beta) const {
  if (a < 0 || a >= num_local()) return -1;
  auto it = info_[a].recv.find(beta);
  return it == info_[a].recv.end() ? 0 : (int)it->second.size();
}
int Group::num_send(int a, int beta) const {
  if (a < 0 || a >= num_local()) return -1;
  auto it = info_[a].sent.find(beta);
  return it == info_[a].sent.end() ? 0 : (int)it->second.size();
}

int Group::receive(int a, int beta, const double *msg, int ld) {
  finish_update();
  if (a < 0 || a >= num_local()) return -1;
  auto it = info_[a].recv.find(beta);
  if (it == info_[a].recv.end()) {
    fprintf(stderr, "[dpgo_amd] ERROR: Can not find information for node %d\n", beta);   // DPGOHash.cpp:77
    return -1;
  }
  const int np = (int)it->second.size();
  if (ld < (d_ + 1) * np) return -1;
  sync();
  // the poses of one neighbour occupy consecutive neighbour rows (ordering of generate_data_info)
  std::vector<double> rec((size_t)np * RS_);
  for (int k = 0; k < np; k++)
    for (int c = 0; c < d_; c++) {
      rec[(size_t)k * RS_ + c] = msg[(size_t)c * ld + k];
      for (int r = 0; r < d_; r++) rec[(size_t)k * RS_ + d_ + r * d_ + c] = msg[(size_t)c * ld + np + k * d_ + r];
    }
  const int first = it->second.front().second;
  HIP_CHECK(hipMemcpy(Xk_.p + (size_t)(P0_ + nbr_off_[a] + first) * RS_, rec.data(), sizeof(double) * rec.size(),
                      hipMemcpyHostToDevice));
  res_[a].updated = 0;
  return 0;
}

int Group::send(int a, int beta, double *msg, int ld) const {
  if (a < 0 || a >= num_local()) return -1;
  auto it = info_[a].sent.find(beta);
  if (it == info_[a].sent.end()) return -1;
  const int np = (int)it->second.size();
  if (ld < (d_ + 1) * np) return -1;
  sync();
  std::vector<double> own((size_t)info_[a].n[0] * RS_);
  HIP_CHECK(hipMemcpy(own.data(), Xk_.p + (size_t)own_off_[a] * RS_, sizeof(double) * own.size(), hipMemcpyDeviceToHost));
  for (int k = 0; k < np; k++) {
    const double *rec = &own[(size_t)it->second[k] * RS_];
    for (int c = 0; c < d_; c++) {
      msg[(size_t)c * ld + k] = rec[c];
      for (int r = 0; r < d_; r++) msg[(size_t)c * ld + np + k * d_ + r] = rec[d_ + r * d_ + c];
    }
  }
  return 0;
}

int Group::pack_sent(double *dev_buf, hipStream_t st) {
  launch_copy_indexed(d_, st ? st : st_, (int)sent_rows_.size(), nullptr, sent_rows_dev_.p, Xk_.p, dev_buf);
  return 0;
}

void Group::join_exchange() {
  if (!xchg_done_) return;
  HIP_CHECK(hipStreamWaitEvent(st_, xchg_done_, 0));
  xchg_done_ = nullptr;
}

int Group::set_recv_layout(int nranks, int stride, const int *counts, const int *nodes, const int *poses) {
  flush_pending_recv();   // (a lazy unpack still pending reads the lists re-uploaded below: it lands as the old lay-out said)
  std::map<std::pair<int, int>, int> slot;
  int off = 0;
  for (int r = 0; r < nranks; r++) {
    for (int k = 0; k < counts[r]; k++) slot[{nodes[off + k], poses[off + k]}] = r * stride + k;
    off += counts[r];
  }
  std::vector<int> dst, src;
  for (int a = 0; a < num_local(); a++)
    for (int k = 0; k < info_[a].n[1]; k++) {
      const auto key = info_[a].nbr_key[k];
      if (local_of_node_.count(key.first)) continue;
      auto it = slot.find(key);
      if (it == slot.end()) {
        fprintf(stderr, "[dpgo_amd] ERROR: No information for pose [%d, %d].\n", key.first, key.second);
        return -1;
      }
      dst.push_back(P0_ + nbr_off_[a] + k);
      src.push_back(it->second);
    }
  recv_dst_.upload(dst);
  recv_src_.upload(src);
  recv_lists_changed();   // (upload() frees and re-allocates: the same size very likely comes back at the same address)
  return 0;
}

int Group::unpack_recv(const double *dev_gathered, hipStream_t st) {
  if ((!st || st == st_) && set_pending_recv(dev_gathered, (int)recv_dst_.n, recv_dst_.p, recv_src_.p) == 0) return 0;   // (lazily: below)
  launch_copy_indexed(d_, st ? st : st_, (int)recv_dst_.n, recv_dst_.p, recv_src_.p, dev_gathered, Xk_.p);
  return 0;
}

// A LAZY unpack: the neighbour rows an exchange on the group's own stream delivered stay in its receive buffer; the next
// update()'s inter-edge pass reads them from there and stores them into Xk on the way (kernels.h: InterEdgesDev::recv) -- no
// unpack kernel.  Whoever else looks at Xk's neighbour rows first (flush_pending_recv) gets the plain indexed copy.  The
// lists (dst: neighbour rows, src: slots of the buffer; device arrays that outlive the exchange) are digested once per list:
// a slot per neighbour row, and per incidence record the slot of its other pose.  Robust losses only (the trivial loss has
// no inter-edge pass); -1: not taken, the caller unpacks as before.
int Group::set_pending_recv(const double *buf, int count, const int *dst_dev, const int *src_dev) {
  flush_pending_recv();
  if (!settings().lazy_unpack || !fused_ || opt_.loss == 0 || star_ || count <= 0 || e_rec_host_.empty()) return -1;
  if (recv_key_ != dst_dev || recv_count_ != count || recv_key_gen_ != recv_gen_) {
    std::vector<int> dst(count), src(count), nsrc((size_t)std::max(P1_, 1), -1);
    HIP_CHECK(hipMemcpy(dst.data(), dst_dev, sizeof(int) * count, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(src.data(), src_dev, sizeof(int) * count, hipMemcpyDeviceToHost));
    for (int k = 0; k < count; k++) {
      if (dst[k] < P0_ || dst[k] >= P0_ + P1_) return -1;   // (not a neighbour row: not ours to interpret)
      nsrc[dst[k] - P0_] = src[k];
    }
    std::vector<InterInc> rec = e_rec_host_;
    for (auto &r : rec) r.osrc = r.other >= P0_ ? nsrc[r.other - P0_] : -1;
    sched_.invalidate();   // (captured launches carry the records' address -- unchanged -- but let nothing replay mid-upload)
    HIP_CHECK(hipMemcpyAsync(e_rec_.p, rec.data(), sizeof(InterInc) * rec.size(), hipMemcpyHostToDevice, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
    recv_nsrc_.upload(nsrc);
    recv_key_ = dst_dev; recv_count_ = count; recv_key_gen_ = recv_gen_;
    recv_dst_dev_ = dst_dev; recv_src_dev_ = src_dev;
  }
  pending_recv_ = buf;
  return 0;
}

void Group::flush_pending_recv() {
  if (!pending_recv_) return;
  const double *buf = pending_recv_;
  pending_recv_ = nullptr;
  launch_copy_indexed(d_, st_, recv_count_, recv_dst_dev_, recv_src_dev_, buf, Xk_.p);
}

void Group::needed_keys(std::vector<std::pair<int, int>> &keys, std::vector<int> &rows) const {
  keys.clear();
  rows.clear();
  for (int a = 0; a < num_local(); a++)
    for (int k = 0; k < info_[a].n[1]; k++) {
      const auto key = info_[a].nbr_key[k];
      if (local_of_node_.count(key.first)) continue;
      keys.push_back(key);
      rows.push_back(P0_ + nbr_off_[a] + k);
    }
}

void Group::copy_records(hipStream_t st, int count, const int *didx, const int *sidx, const double *src, double *dst) const {
  launch_copy_indexed(d_, st, count, didx, sidx, src, dst);
}

int Group::set_collectives(double *send_dev, double *gathered_dev, AllGatherFn ag, AllReduceFn ar, void *user) {
  if ((ag && (!send_dev || !gathered_dev)) || (ag && !ar)) return -1;
  coll_send_ = send_dev;
  coll_gathered_ = gathered_dev;
  coll_allgather_ = ag;
  coll_allreduce_ = ar;
  coll_allreduce_dev_ = nullptr;   // (belongs to whoever lends the collectives: set again by set_device_allreduce)
  coll_user_ = user;
  return 0;
}

// The rescale test of evaluate_g_and_f*_rescale (DPGOProblem.cpp:300-321, 464-485) for the nodes of `set`: a node
// is rescaled when its counter has reached max_rescale_count or some edge weight exceeds the edge's scale; its new
// scales are clamp(1.25 w, min_rescale_, max_rescale_) (DPGOProblem.h:17-18), update_quadratic_mat (:751-840) and
// L_.factorize follow.  The preconditioner keeps the factor of the constructor, as in the reference.
std::vector<int> Group::maybe_rescale(const std::vector<int> &set) {
  SetupClock clk;   // (DPGO_SETUP_TIMING=1)
  std::vector<int> changed;
  std::vector<double> w(std::max<size_t>(e_w_.n, 1));
  sync();
  if (E_.m > 0) HIP_CHECK(hipMemcpy(w.data(), e_w_.p, sizeof(double) * E_.m, hipMemcpyDeviceToHost));
  for (int a : set) {
    const int m1 = e_off_[a + 1] - e_off_[a];
    bool rescaled = rescale_count_[a] >= opt_.max_rescale_count;
    for (int e = 0; e < m1 && !rescaled; e++) rescaled = w[e_off_[a] + e] > scale_[a][e];
    if (!rescaled) {
      rescale_count_[a]++;
      continue;
    }
    for (int e = 0; e < m1; e++) scale_[a][e] = std::min(1.0, std::max(0.01, 1.25 * w[e_off_[a] + e]));
    rescale_count_[a] = 0;
    changed.push_back(a);
  }
  if (!changed.empty()) {
    int bad = 0;
    const int nc = (int)changed.size();
#pragma omp parallel for schedule(dynamic, 1) num_threads(std::max(1, std::min(nc, host_threads()))) reduction(+ : bad)
    for (int i = 0; i < nc; i++) {
      const int a = changed[i];
      bad += assemble_node(info_[a], opt_.regularizer, false, ops_[a], scale_[a].data()) != 0;
    }
    if (bad) throw DeviceError("assemble_node");
    clk.lap("rescale: weights + host assembly");
    upload_operators();
    clk.lap("rescale: operators to the device");
    if (refactor_tt() != 0) throw DeviceError("G_tt is not positive definite after a rescale");
  }
  return changed;
}

// What the device-side rescale needs beside the scales: the diagonal blocks of G and of the proximal majoriser H with
// every scale at zero (the intra-node part + the regulariser), and where the diagonal block of every own pose sits in
// the uploaded block values of G.
void Group::setup_device_rescale() {
  const int L = num_local(), BB = B_ * B_;
  std::vector<double> Gb((size_t)std::max(P0_, 1) * BB, 0.0), Hb((size_t)std::max(P0_, 1) * BB, 0.0);
  std::vector<int> gpos((size_t)std::max(P0_, 1) * 4, 0);
  int bad = 0;
#pragma omp parallel for schedule(dynamic, 1) num_threads(std::max(1, std::min(L, host_threads()))) reduction(+ : bad)
  for (int a = 0; a < L; a++) {
    NodeOperators base;
    const std::vector<double> zeros(std::max<size_t>(info_[a].inter.size(), 1), 0.0);
    if (assemble_node(info_[a], opt_.regularizer, false, base, zeros.data()) != 0) { bad++; continue; }
    for (int r = 0; r < info_[a].n[0]; r++) {
      for (int k = base.G.ptr[r]; k < base.G.ptr[r + 1]; k++)
        if (base.G.col[k] == r) std::copy(&base.G.val[(size_t)k * BB], &base.G.val[(size_t)(k + 1) * BB], &Gb[(size_t)(own_off_[a] + r) * BB]);
      std::copy(&base.Hd[(size_t)r * BB], &base.Hd[(size_t)(r + 1) * BB], &Hb[(size_t)(own_off_[a] + r) * BB]);
    }
  }
  if (bad) throw DeviceError("assemble_node");
  // the unified block-CSR of G (upload_bsr): rows of node a at own_off_[a], its blocks in the order of ops_[a].G
  int kuni = 0;
  for (int a = 0; a < L; a++) {
    const BsrMatrix &M = ops_[a].G;
    for (int r = 0; r < M.nrows; r++) {
      const int k0row = kuni, cntrow = M.ptr[r + 1] - M.ptr[r];
      for (int k = M.ptr[r]; k < M.ptr[r + 1]; k++)
        if (M.col[k] == r) {
          const int kk = k - M.ptr[r], round0 = k0row + (kk / BSR_LPR) * BSR_LPR;
          int *g = &gpos[(size_t)(own_off_[a] + r) * 4];
          g[0] = round0 * BB;
          g[1] = std::min(BSR_LPR, k0row + cntrow - round0);
          g[2] = kk % BSR_LPR;
          g[3] = k0row + kk;
        }
      kuni += cntrow;
    }
  }
  Gbase_.upload(Gb);
  Hbase_.upload(Hb);
  gpos_.upload(gpos);
  device_rescale_ = true;
}

// The decision of k_rescale_decide has arrived (h_rs_): rebuild the block-diagonal terms of the rescaled nodes on the
// device, re-factor G_tt from the values that are already there, cut the solve's panels again.
std::vector<int> Group::rescale_device(const std::vector<int> &set) {
  SetupClock clk;   // (DPGO_SETUP_TIMING=1)
  std::vector<int> changed;
  for (int a : set)
    if (h_rs_[a] != 0.0) changed.push_back(a);
  if (changed.empty()) return changed;
  RescaleArgs A;
  A.flags = rs_flags_.p; A.scale = e_scale_.p; A.Gbase = Gbase_.p; A.Hbase = Hbase_.p; A.gpos = gpos_.p; A.att_pos = att_pos_.p;
  A.Gval = G_.val.p; A.Gtcol = G_.tcol.p; A.Dd = Dd_.p; A.Qd = Qd_.p; A.Tinv = Tinv_.p; A.N = N_.p; A.V = V_.p;
  A.att_val = spd_numeric_values(Ltt_.F);
  A.xi = opt_.regularizer;
  launch_rescale_apply(d_, st_, T_, E_, A);
  // everything on the group's stream, enqueued in one go: the new values, the factorisation, the panels (three waits
  // before, with the GPU idle across each)
  if (spd_refactor_device(Ltt_.F, (void *)st_, true) != 0) throw DeviceError("G_tt: refactorisation could not be enqueued");
  if (Ltt_.repack(st_) != 0) throw DeviceError("repack");
  // the verdict is read at the next read-back that was enqueued behind the factorisation: nothing waits for it here
  tt_verdict_pending_ = true;
  tt_verdict_seq_ = sched_.last_seq() + 1;
  if (clk.on) {
    sync();
    fprintf(stderr, "[setup] rescale: %zu of %zu nodes\n", changed.size(), set.size());
  }
  clk.lap("rescale: block-diagonal terms, numeric factorisation of G_tt, panels (device)");
  return changed;
}

}  // namespace dpgo

namespace dpgo {

void Group::put_rows(int a, double *dev, const double *X, int ld, int row_t0, int row_r0, bool has_t) {
  const int n0 = info_[a].n[0];
  std::vector<double> rec((size_t)n0 * RS_, 0.0);
  for (int k = 0; k < n0; k++)
    for (int c = 0; c < d_; c++) {
      if (has_t) rec[(size_t)k * RS_ + c] = X[(size_t)c * ld + row_t0 + k];
      for (int r = 0; r < d_; r++) rec[(size_t)k * RS_ + d_ + r * d_ + c] = X[(size_t)c * ld + row_r0 + k * d_ + r];
    }
  (void)hipMemcpy(dev + (size_t)own_off_[a] * RS_, rec.data(), sizeof(double) * rec.size(), hipMemcpyHostToDevice);
}

void Group::get_rows(int a, const double *dev, double *X, int ld, int row_t0, int row_r0, bool has_t) {
  const int n0 = info_[a].n[0];
  std::vector<double> rec((size_t)n0 * RS_);
  sync();
  (void)hipMemcpy(rec.data(), dev + (size_t)own_off_[a] * RS_, sizeof(double) * rec.size(), hipMemcpyDeviceToHost);
  for (int k = 0; k < n0; k++)
    for (int c = 0; c < d_; c++) {
      if (has_t) X[(size_t)c * ld + row_t0 + k] = rec[(size_t)k * RS_ + c];
      for (int r = 0; r < d_; r++) X[(size_t)c * ld + row_r0 + k * d_ + r] = rec[(size_t)k * RS_ + d_ + r * d_ + c];
    }
}

// Single operators on reference-layout inputs, for the parity tests.  Each enqueues the launches the iteration uses for it
// (tnt.cpp, update(), iterate()).  "op" runs under the node's own mask (the compacted live-segment mapping, live_mask);
// "op:all" under the whole group's (the whole-grid mapping of the iteration's common case), with the other nodes' rows zero.
int Group::debug_apply(int a, const char *op_c, const double *in, int ld_in, double *out, int ld_out) {
  finish_update();
  if (a < 0 || a >= num_local()) return -1;
  std::string op(op_c);
  const bool whole = op.size() > 4 && op.compare(op.size() - 4, 4, ":all") == 0;
  if (whole) op.resize(op.size() - 4);
  const int n0 = info_[a].n[0], n1 = info_[a].n[1];
  const int R0 = (d_ + 1) * n0;   // rows of one stacked operand
  sync();
  for (auto &t : tmp_) HIP_CHECK(hipMemsetAsync(t.p, 0, sizeof(double) * t.n, st_));
  HIP_CHECK(hipStreamSynchronize(st_));   // (before the inputs are copied in on the null stream)
  if (whole) {
    std::vector<int> all(num_local());
    for (int b = 0; b < num_local(); b++) all[b] = b;
    set_mask(all);
  } else set_mask({a});
  auto put_own = [&](double *dev, const double *X, int ld, int row_t0, int row_r0, bool has_t) { put_rows(a, dev, X, ld, row_t0, row_r0, has_t); };
  auto get_own = [&](const double *dev, double *X, int ld, int row_t0, int row_r0, bool has_t) { get_rows(a, dev, X, ld, row_t0, row_r0, has_t); };
  double *A = tmp_[0].p, *Bv = tmp_[1].p, *C = tmp_[2].p;
  if (op == "project") {
    (void)hipMemset(A + (size_t)own_off_[a] * RS_, 0, sizeof(double) * n0 * RS_);
    put_own(Bv, in, ld_in, 0, 0, false);
    launch_retract_rot(lc(), A, Bv, C);
    get_own(C, out, ld_out, 0, 0, false);
  } else if (op == "solve_tt" || op == "solve_rr") {
    put_own(A, in, ld_in, 0, n0, true);
    put_own(Bv, in, ld_in, 0, n0, true);   // (the solve writes the unknowns' entries only: the rest of the answer is the input's)
    if (op == "solve_tt") solve_tt(A, Bv, 1.0);
    else {
      if (Lrr_.F.n == 0) return -1;
      solve_rr(A, Bv, 1.0);
    }
    get_own(Bv, out, ld_out, 0, n0, true);
  } else if (op == "G") {
    put_own(A, in, ld_in, 0, n0, true);
    launch_bsr(lc(), G_.dev, {.x = A, .y = Bv});
    get_own(Bv, out, ld_out, 0, n0, true);
  } else if (op == "proximal") {
    // in = [Z ((d+1)(n0+n1) rows) ; Df ((d+1) n0 rows)]
    const int zr = (d_ + 1) * (n0 + n1);
    put_own(A, in, ld_in, 0, n0, true);
    put_own(Bv, in, ld_in, zr, zr + n0, true);
    launch_proximal(lc(), A, Bv, Tinv_.p, N_.p, V_.p, C, nullptr, nullptr, 0);
    get_own(C, out, ld_out, 0, n0, true);
  } else if (op == "hess") {
    // in = [Y ; nabla ; Ydot ; r]; out = [Hess[Ydot] (rotation rows) ; <p,Hp>, <Hp,Hp>, <p,p>, <p,r> in column 0], p = Ydot:
    // a CG step's first half (tnt.cpp, stepA) with the sums reduced as k_cg_scal reduces them (k_reduce's order)
    double *X = tmp_[0].p, *nabla = tmp_[1].p, *pk = tmp_[2].p, *rk = tmp_[3].p, *w1 = tmp_[4].p, *w3 = tmp_[5].p, *Hp = tmp_[6].p;
    put_own(X, in, ld_in, 0, n0, true);
    put_own(nabla, in, ld_in, R0, R0 + n0, true);
    put_own(pk, in, ld_in, 0, 2 * R0 + n0, false);   // (tangent vectors carry no translation: p.x = r.x = 0 in the iteration)
    put_own(rk, in, ld_in, 0, 3 * R0 + n0, false);
    launch_bsr(lc(), G_.dev, {.x = pk, .mode = BsrMode::NoTrans, .y = w1});   // G [0 ; p.R]
    solve_tt(w1, w3, -1.0);
    launch_bsr_tcol_hess(lc(), g_tcol(),
                         {.xt = w3, .base = w1, .X = X, .nabla = nabla, .p = pk, .Hp = Hp, .r = rk, .partials = partials_.p});
    fetch(4, false);
    get_own(Hp, out, ld_out, 0, n0, false);
    for (int q = 0; q < 4; q++) out[R0 + q] = scal(a, q);
  } else if (op == "rgrad") {
    // in = [Y ; g]; out = [Y' ; nabla' ; grad' ; nabla ; grad ; 4 sums], rows R0 each.  nabla = G Y + g, grad = Proj_Y(nabla.R)
    // at Y as given (launch_bsr + launch_tangent_rot, tnt.cpp quad_model); the primed ones at Y' = [t recovered from Y.R and
    // g ; Y.R] (recover_translations + launch_bsr_tcol_begin, quad_model's from_base path) with its epilogue sums
    // |grad'|^2, <Y', nabla'>, <Y', g>, <Y', g> in column 0 of the last 4 rows
    double *X = tmp_[0].p, *g = tmp_[1].p, *nab = tmp_[2].p, *grad = tmp_[3].p, *nab1 = tmp_[4].p, *grad1 = tmp_[5].p;
    put_own(X, in, ld_in, 0, n0, true);
    put_own(g, in, ld_in, R0, R0 + n0, true);
    launch_bsr(lc(), G_.dev, {.x = X, .addv = g, .y = nab});
    launch_tangent_rot(lc(), {.X = X, .in = nab, .out = grad});
    recover_translations(X, g);
    launch_bsr_tcol_begin(lc(), g_tcol(),
                          {.xt = X, .base = T1_.p, .y = nab1, .X = X, .grad = grad1, .partials = partials_.p, .g = g, .ga = g});
    fetch(4, false);
    get_own(X, out, ld_out, 0, n0, true);
    get_own(nab1, out, ld_out, R0, R0 + n0, true);
    get_own(grad1, out, ld_out, 2 * R0, 2 * R0 + n0, true);
    get_own(nab, out, ld_out, 3 * R0, 3 * R0 + n0, true);
    get_own(grad, out, ld_out, 4 * R0, 4 * R0 + n0, true);
    for (int q = 0; q < 4; q++) out[5 * R0 + q] = scal(a, q);
  } else if (op == "precon") {
    // in = [Y ; v]; out = [Proj_Y(M^-1 v.R) (rotation rows) ; <v, out> in column 0]: the preconditioner of a CG step (tnt.cpp,
    // stepB), M = G_RR + lambda I (RegularizedCholesky) or diag(G_RR) (Jacobi), whichever the group was built with
    double *X = tmp_[0].p, *v = tmp_[1].p, *w1 = tmp_[2].p, *pv = tmp_[3].p;
    put_own(X, in, ld_in, 0, n0, true);
    put_own(v, in, ld_in, 0, R0 + n0, false);
    if (opt_.preconditioner == 1 && jacobi_.n > 0) launch_rot_rowscale(lc(), jacobi_.p, v, w1);
    else if (Lrr_.F.n > 0) solve_rr(v, w1, 1.0);
    else return -1;
    launch_tangent_rot(lc(), {.X = X, .in = w1, .out = pv, .dotv = v, .partials = partials_.p});
    fetch(1, false);
    get_own(pv, out, ld_out, 0, n0, false);
    out[R0] = scal(a, 0);
  } else if (op == "retract") {
    // in = [Y ; Ydot ; g]; out = [-G_tt^-1 (g_t + G_tR R+) ; R+ = proj(Y.R + Ydot.R)] (tnt.cpp, enqueue_trial)
    double *X = tmp_[0].p, *sk = tmp_[1].p, *g = tmp_[2].p, *xprop = tmp_[3].p;
    put_own(X, in, ld_in, 0, n0, true);
    put_own(sk, in, ld_in, 0, R0 + n0, false);
    put_own(g, in, ld_in, 2 * R0, 2 * R0 + n0, true);
    launch_retract_rot(lc(), X, sk, xprop);
    recover_translations(xprop, g);
    get_own(xprop, out, ld_out, 0, n0, true);
  } else if (op == "lambda_max") {
    out[0] = lambda_max_[a];   // (the host's Lanczos estimate the shift of G_RR was formed with)
  } else {
    fprintf(stderr, "[dpgo_amd] ERROR: debug_apply: unknown operator %s\n", op_c);
    return -1;
  }
  return 0;
}


int Group::debug_seg_layout(int *nseg_all, int *own_ptr, int *nbr_ptr) const {
  const int L = num_local();
  if (nseg_all) *nseg_all = T_.nseg_all;
  if (own_ptr) HIP_CHECK(hipMemcpy(own_ptr, T_.own_ptr, sizeof(int) * (L + 1), hipMemcpyDeviceToHost));
  if (nbr_ptr) HIP_CHECK(hipMemcpy(nbr_ptr, T_.nbr_ptr, sizeof(int) * (L + 1), hipMemcpyDeviceToHost));
  return 0;
}

// The CG's scalar kernels on given partial sums, for tests/test_gpu_cg_scalars.py: every launch is the one tnt.cpp makes
// (later_round, enqueue_device_start, step_a, step_b, scal_begin) with the vectors' passes left out -- their sums are handed in.
// reduce_gate / reduce: the trial point's reduction with the gate of a speculative update (speculate_update's launch, the gate's
// scalars and options from the script), and launch_reduce over own rows on the same sums (tests/test_gpu_gate.py).
int Group::debug_cg_scalars(const CgDebugLaunch *script, int n, double *records, unsigned long long *masks, double *cg_summary,
                            double *tnt_summary, double *dev_tnt, unsigned long long *seq, unsigned *arrived, double *gate_sums,
                            unsigned long long *gate_words) {
  finish_update();
  const int L = num_local();
  if (!script || n < 0 || !records || !masks || !cg_summary || !tnt_summary || !dev_tnt || !seq || !arrived) return -1;
  for (int i = 0; i < n; i++) {
    const CgDebugLaunch &q = script[i];
    const bool begins = q.kind == CG_DBG_BEGIN_HOST || q.kind == CG_DBG_BEGIN_DEVICE || q.kind == CG_DBG_SCAL_BEGIN;
    if (q.kind < 0 || q.kind >= CG_DBG_KINDS || q.slots < 0 || q.slots > MAX_SLOTS || (q.slots > 0 && !q.partials)) return -1;
    if (begins && (q.max_it < 0 || (q.bits & ~all_bits()) || !q.Delta)) return -1;
    if (q.kind == CG_DBG_BEGIN_HOST && (!q.rv || !q.target)) return -1;
    if (q.kind == CG_DBG_REDUCE_GATE || q.kind == CG_DBG_REDUCE) {
      const GateDebug *g = q.gate;
      if (!g || !gate_sums || !gate_words || g->nslots <= 0 || g->nslots > MAX_SLOTS || L == 0) return -1;
      if (q.kind == CG_DBG_REDUCE_GATE && (!g->f || !g->Fk0 || !g->Fk1 || !g->fobj || !g->hits0 || !g->hits1)) return -1;
    }
  }
  sync();
  std::vector<CgNode> rec(L);
  for (int i = 0; i < n; i++) {
    const CgDebugLaunch &q = script[i];
    if (q.slots > 0)
      HIP_CHECK(hipMemcpy(partials_.p, q.partials, sizeof(double) * (size_t)q.slots * T_.nseg_all, hipMemcpyHostToDevice));
    bool flagged = true;
    if (q.kind == CG_DBG_BEGIN_HOST) {
      CgStart cs;
      for (int a = 0; a < MAX_LOCAL_NODES; a++) {
        cs.rv[a] = a < L ? q.rv[a] : 0.0;
        cs.Delta[a] = a < L ? q.Delta[a] : 0.0;
        cs.target[a] = a < L ? q.target[a] : 0.0;
      }
      launch_cg_begin(st_, L, q.bits, cs, q.max_it, cg_.p, dmask_.p);
      flagged = false;
    } else if (q.kind == CG_DBG_SCAL0 || q.kind == CG_DBG_SCAL1) {
      launch_cg_scal(st_, T_, L, q.kind == CG_DBG_SCAL0 ? 0 : 1, partials_.p, cg_.p, dmask_.p, h_cg_, sched_.flag());
    } else if (q.kind == CG_DBG_REDUCE) {
      launch_reduce(st_, T_, L, false, q.gate->nslots, partials_.p, h_scal_, sched_.flag());
    } else if (q.kind == CG_DBG_REDUCE_GATE) {
      const GateDebug &g = *q.gate;
      Options o = opt_;
      o.max_iterations = g.max_it; o.max_iterations_accepted = g.max_acc;
      o.max_soft_restart_hits[0] = g.max_hits0; o.max_soft_restart_hits[1] = g.max_hits1;
      o.rel_func_decrease_tol = g.rel_tol; o.stepsize_tol = g.step_tol; o.psi = g.psi; o.phi = g.phi;
      const AmmGate G = amm_gate(L, o, [&g](int a) { return GateNode{g.f[a], g.Fk0[a], g.Fk1[a], g.fobj[a], g.hits0[a], g.hits1[a]}; });
      launch_reduce_gate(st_, T_, L, g.nslots, partials_.p, h_scal_, sched_.flag(), dev_sums_.p, G, dev_tnt_.p, cg_.p, go_.p, h_gate_);
    } else {
      const TntStart start = {.nnodes = L, .bits = q.bits, .use_precon = q.use_precon != 0, .max_it = q.max_it,
                              .grad_tol = q.grad_tol, .pgrad_tol = q.pgrad_tol, .kappa = q.kappa, .theta = q.theta, .Delta = q.Delta,
                              .partials = partials_.p, .cg = cg_.p, .dmask = dmask_.p, .host_tnt = h_tnt_};
      if (q.kind == CG_DBG_BEGIN_DEVICE) {
        launch_tnt_begin(st_, T_, start);
        flagged = false;
      } else launch_cg_scal_begin(st_, T_, start, h_cg_, sched_.flag(), dev_tnt_.p, 0, h_upd_);
    }
    if (flagged) wait_flag(sched_.last_seq());
    HIP_CHECK(hipStreamSynchronize(st_));
    HIP_CHECK(hipMemcpy(rec.data(), cg_.p, sizeof(CgNode) * L, hipMemcpyDeviceToHost));
    for (int a = 0; a < L; a++) {
      const CgNode &c = rec[a];
      const double w[CG_DBG_RECORD] = {c.sk_M_pk, c.sk_M_2, c.pk_M_2, c.rv, c.Delta, c.Delta_2, c.target, c.h_M_norm, c.c1, c.cr,
                                       c.al, c.kap, c.be, (double)c.cg_it, (double)c.max_it, (double)c.live, (double)c.stop_ord};
      std::copy(w, w + CG_DBG_RECORD, records + ((size_t)i * L + a) * CG_DBG_RECORD);
    }
    NodeBits m[3];
    HIP_CHECK(hipMemcpy(m, dmask_.p, sizeof(m), hipMemcpyDeviceToHost));
    for (int k = 0; k < 3; k++) masks[(size_t)i * 3 + k] = m[k];
    std::copy(h_cg_, h_cg_ + (size_t)L * CG_SUMMARY, cg_summary + (size_t)i * L * CG_SUMMARY);
    std::copy(h_tnt_, h_tnt_ + (size_t)L * TNT_SUMMARY, tnt_summary + (size_t)i * L * TNT_SUMMARY);
    HIP_CHECK(hipMemcpy(dev_tnt + (size_t)i * L * TNT_SUMMARY, dev_tnt_.p, sizeof(double) * L * TNT_SUMMARY, hipMemcpyDeviceToHost));
    seq[(size_t)i * 2] = sched_.flag_value();
    seq[(size_t)i * 2 + 1] = sched_.last_seq();
    arrived[i] = sched_.arrived_count();
    if (q.kind == CG_DBG_REDUCE_GATE || q.kind == CG_DBG_REDUCE) {
      const size_t ns = (size_t)L * MAX_SLOTS;
      std::copy(h_scal_, h_scal_ + ns, gate_sums + (size_t)i * 2 * ns);
      HIP_CHECK(hipMemcpy(gate_sums + ((size_t)i * 2 + 1) * ns, dev_sums_.p, sizeof(double) * ns, hipMemcpyDeviceToHost));
      NodeBits go = 0;
      HIP_CHECK(hipMemcpy(&go, go_.p, sizeof(go), hipMemcpyDeviceToHost));
      gate_words[(size_t)i * 2] = go;
      static_assert(sizeof(unsigned long long) == sizeof(double), "");
      std::memcpy(&gate_words[(size_t)i * 2 + 1], h_gate_, sizeof(double));
    }
  }
  return 0;
}

// AMM-PGO*'s master sums on given partial sums, for tests/test_gpu_star_sums.py: the two launches star_sums() ends with
int Group::debug_star_sums(const double *partials, unsigned valid, double *out, unsigned long long *seq) {
  finish_update();
  if (!partials || !out || !seq || (valid & ~0x3fu) || num_local() == 0) return -1;
  sync();
  if (star_vals_.n == 0) star_vals_.alloc(8);
  HIP_CHECK(hipMemcpy(partials_.p, partials, sizeof(double) * (size_t)MAX_SLOTS * T_.nseg_all, hipMemcpyHostToDevice));
  launch_star_sums(st_, T_, num_local(), valid, star_slots(), partials_.p, star_vals_.p);
  launch_publish(st_, star_vals_.p, 4, h_scal_, sched_.flag());
  wait_flag(sched_.last_seq());
  std::copy(h_scal_, h_scal_ + 4, out + 4);
  HIP_CHECK(hipStreamSynchronize(st_));
  HIP_CHECK(hipMemcpy(out, star_vals_.p, sizeof(double) * 4, hipMemcpyDeviceToHost));
  seq[0] = sched_.flag_value();
  seq[1] = sched_.last_seq();
  return 0;
}

}  // namespace dpgo


namespace dpgo {

// ---------------------------------------------------------------------------
// AMM-PGO*  (DPGOStar, C++/DPGO/src/DPGOStar.cpp)
// ---------------------------------------------------------------------------
// Global objective F(X) (DPGOStar::evaluate_f, :713-761) at the point whose own rows are X_own:
// neighbour rows are gathered from the same trial vector, every node evaluates its intra edges and
// its inter edges (charged 1/2 per node), the host adds the per-node sums (the master's aggregate).
void Group::enqueue_objective(const double *X_own, int slot0) {
  copy_rows(Tall_.p, X_own, false, 0);
  launch_copy_indexed(d_, st_, (int)gather_dst_.n, gather_dst_.p, gather_src_.p, Tall_.p, Tall_.p);
  if (coll_allgather_) {   // boundary poses of the trial point hosted by other groups
    launch_copy_indexed(d_, st_, (int)sent_rows_.size(), nullptr, sent_rows_dev_.p, X_own, coll_send_);
    if (coll_allgather_(coll_user_) != 0) throw DeviceError("all-gather callback failed");
    launch_copy_indexed(d_, st_, (int)recv_dst_.n, recv_dst_.p, recv_src_.p, coll_gathered_, Tall_.p);
  }
  launch_cost(lc(), Ei_, E_, opt_.loss == 0, opt_.loss, opt_.loss_reg, Tall_.p, partials_.p, slot0);
}

// Where star_sums() keeps its six partial sums.  update() and evaluate_global() reduce slots 0..2 over ALL rows and count on the
// neighbour segments of slot 2 never having been written; k_cost writes every segment of its two slots.  So the first point's
// pair is 0, 1 (as it always was) and the second point's pair the last two slots, which nobody else touches; the distances are
// own-row sums.
const int *Group::star_slots() {
  static const int slots[6] = {0, 1, MAX_SLOTS - 2, MAX_SLOTS - 1, 4, 5};
  return slots;
}

// Everything the master's tests of one AMM-PGO* iteration need (DPGOStar.cpp:147-192), enqueued back to back and read
// ONCE: the passes leave their partial sums in slots 0..5, k_star_sums folds them over the nodes on the device, the sum
// over the groups -- if there are several -- is an all-reduce on the same stream (set_device_allreduce) or, for a host
// that lent only host collectives, one call after the read-back; k_publish raises the flag.  (Before: up to four
// read-backs and as many host-staged all-reduces per iteration.)
int Group::star_sums(const double *X1_own, const double *X2_own, const double *ref_own, double *F1, double *F2, double *d1, double *d2) {
  finish_update();
  std::vector<int> all(num_local());
  for (int a = 0; a < num_local(); a++) all[a] = a;
  set_mask(all);
  if (star_vals_.n == 0) star_vals_.alloc(8);
  const int *slots = star_slots();
  unsigned valid = 0;
  if (F1) { enqueue_objective(X1_own, slots[0]); valid |= 0x3; }
  if (X2_own && F2) { enqueue_objective(X2_own, slots[2]); valid |= 0xc; }
  if (ref_own) {
    if (d1) { launch_sqdist(lc(), X1_own, ref_own, partials_.p, slots[4]); valid |= 0x10; }
    if (X2_own && d2) { launch_sqdist(lc(), X2_own, ref_own, partials_.p, slots[5]); valid |= 0x20; }
  }
  launch_star_sums(st_, T_, num_local(), valid, slots, partials_.p, star_vals_.p);
  const bool dev_sum = coll_allreduce_dev_ != nullptr;
  if (dev_sum && coll_allreduce_dev_(coll_user_, star_vals_.p, 4) != 0) return -1;
  launch_publish(st_, star_vals_.p, 4, h_scal_, sched_.flag());
  wait_flag(sched_.last_seq());
  double v[4] = {h_scal_[0], h_scal_[1], h_scal_[2], h_scal_[3]};
  if (!dev_sum && coll_allreduce_ && coll_allreduce_(coll_user_, v, 4) != 0) return -1;
  if (F1) *F1 = v[0];
  if (F2) *F2 = v[1];
  if (d1) *d1 = v[2];
  if (d2) *d2 = v[3];
  return 0;
}

double Group::global_objective(const double *X_own) {
  double F = NAN;
  if (star_sums(X_own, nullptr, nullptr, &F, nullptr, nullptr, nullptr) != 0) return NAN;
  return F;
}

int Group::star_initialize_global(const double *X, int ld) {
  finish_update();
  if (num_local() != num_nodes_total_ && !coll_allgather_) {
    fprintf(stderr, "[dpgo_amd] ERROR: AMM-PGO* needs every node of the graph in one group, or collectives "
                    "(dpgo_group_set_collectives) that connect the groups.\n");
    return -1;
  }
  if (initialize_global(X, ld) != 0) return -1;
  star_ = true;
  star_fobj_ = global_objective(Xk_.p);
  starF_ = star_fobj_;
  star_fobjh_ = star_fobj_;
  return 0;
}

int Group::star_update() {
  finish_update();
  if (!star_) return -1;
  std::vector<int> all(num_local());
  for (int a = 0; a < num_local(); a++) all[a] = a;
  return update(all);
}

int Group::star_iterate() {
  Schedule::InLib in_lib(sched_);
  finish_update();
  if (!star_) return -1;
  const Options &o = opt_;
  const int L = num_local();
  std::vector<int> all(L);
  for (int a = 0; a < L; a++) all[a] = a;
  for (int a : all)
    if (!res_[a].updated) {
      fprintf(stderr, "[dpgo_amd] ERROR: The optimizer has not been updated (node %d).\n", nodes_[a]);
      return -1;
    }
  star_branches_ = 0;
  // ---- amm_pgo_n for every node (:392-550)
  set_mask(all);
  prepare_extrapolated();
  std::vector<int> ref;
  for (int a : all) {
    NodeResults &r = res_[a];
    r.refined = (r.gradFnorm * r.gradFnorm / r.fobj) > o.accepted_delta;   // :515-516
    if (r.refined) ref.push_back(a);
  }
  launch_proximal(lc(), Y_.p, Dfx_.p, Tinv_.p, N_.p, V_.p, Xakh_.p, nullptr, nullptr, 0);
  copy_rows(Xak_.p, Xakh_.p, false, 2);
  recover_translations(Xak_.p, gx_.p);
  if (!ref.empty()) run_tnt(ref, Xak_.p, gx_.p, nullptr, true);
  // ---- the master's tests (:147-192); Xk = own rows of X[k] (Zc_).  The two objectives and the two distances of the
  // common path come with one read-back (the first test's branch changes Xakh only, so F(Xak) may be taken before it)
  double fobjh = NAN, fobj = NAN, sqh = NAN, sq = NAN;
  if (star_sums(Xakh_.p, Xak_.p, Zc_.p, &fobjh, &fobj, &sqh, &sq) != 0) return -1;
  set_mask(all);
  if (fobjh > starF_ - o.psi * sqh) {
    star_branches_ |= 1;   // pm_pgo_n (:685-711)
    launch_proximal(lc(), Zc_.p, Dfc_.p, Tinv_.p, N_.p, V_.p, Xakh_.p, nullptr, nullptr, 0);
    fobjh = global_objective(Xakh_.p);
  }
  set_mask(all);
  if (fobj > starF_ - o.psi * sq) {
    star_branches_ |= 2;   // mm_pgo_n (:552-683) and halve s
    copy_rows(Xak_.p, Xakh_.p, false, 2);
    recover_translations(Xak_.p, gc_.p);
    refine_or_evaluate(all, gc_.p);   // sets Gk = Results.f
    for (int a : all) res_[a].s1 = std::max(0.5 * res_[a].s1, 1.0);
    fobj = global_objective(Xak_.p);
  }
  if (starF_ - fobj < o.phi * (starF_ - fobjh)) {
    star_branches_ |= 4;   // fall back to the proximal rotations (:171-192)
    set_mask(all);
    copy_rows(Xak_.p, Xakh_.p, false, 2);
    recover_translations(Xak_.p, gc_.p);
    fobj = global_objective(Xak_.p);
  }
  set_mask(all);
  copy_rows(Xk_.p, Xak_.p, false);
  for (int a : all) {
    res_[a].iters++;
    res_[a].updated = 0;
  }
  star_fobj_ = fobj;
  star_fobjh_ = fobjh;
  starF_ = starF_ * (1 - o.eta[0]) + fobj * o.eta[0];
  return 0;
}

}  // namespace dpgo
