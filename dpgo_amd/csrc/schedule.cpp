#include "schedule.h"

#include <cstdio>

namespace dpgo {

void Schedule::open(size_t front, size_t back, int rows, int nodes) {
  rows_ = rows;
  nodes_ = nodes;
  HIP_CHECK(hipStreamCreate(&st_));
  HIP_CHECK(hipHostMalloc((void **)&pinned_, sizeof(double) * (front + 16 + back), hipHostMallocMapped | hipHostMallocCoherent));
  host_flag_ = reinterpret_cast<unsigned long long *>(pinned_ + front + 8);
  *host_flag_ = 0;
  back_ = pinned_ + front + 16;
  arrived_.alloc(1);
  dev_seq_.alloc(1);
}

bool Schedule::close(double seconds) {
  const bool idle = drain(seconds);
  if (!idle) dev_leak_buffers(true);   // (the group's buffers are destroyed after this: hipFree would wait for the stuck stream)
  if (idle) {
    destroy_graphs();
  } else {
    fprintf(stderr, "[dpgo_amd] WARNING: the group's stream did not drain; its graphs, pinned block and stream are leaked.\n");
    graphs_.clear();
  }
  if (pinned_ && idle) (void)hipHostFree(pinned_);
  if (st_ && idle) (void)hipStreamDestroy(st_);
  pinned_ = back_ = nullptr;
  host_flag_ = nullptr;
  st_ = nullptr;
  return idle;
}

unsigned Schedule::arrived_count() const {
  unsigned v = 0;
  HIP_CHECK(hipMemcpy(&v, arrived_.p, sizeof(v), hipMemcpyDeviceToHost));
  return v;
}

void Schedule::wait(unsigned long long seq) {
  const auto t0 = std::chrono::steady_clock::now();
  struct Acc {   // (what the host-bound test and DPGO_HOST_TIMING need: the time spent in here)
    Schedule *s; std::chrono::steady_clock::time_point t;
    ~Acc() {
      const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count();
      s->win_wait_s_ += dt;
      if (!s->host_timing_) return;
      s->t_wait_ += dt; s->n_wait_++;
      s->wait_hist_[dt < 50e-6 ? 0 : dt < 200e-6 ? 1 : dt < 1e-3 ? 2 : dt < 5e-3 ? 3 : dt < 50e-3 ? 4 : 5]++;
    }
  } acc{this, t0};
  auto arrived = [&] { return __atomic_load_n(host_flag_, __ATOMIC_ACQUIRE) >= seq; };
  win_nwait_++;
  if (arrived()) win_nlate_++;
  for (unsigned spins = 0; !arrived(); spins++) {
    __builtin_ia32_pause();
    if ((spins & 0xfffff) != 0xfffff) continue;
    if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(60)) {
      // surfaces a kernel fault, if that is why the flag never came -- without waiting for ever on a stream that is itself
      // waiting for an exchange whose peer is gone
      const hipError_t q = poll_stream(st_, 60.0, std::chrono::milliseconds(100), arrived);
      if (q != hipErrorNotReady) HIP_CHECK(q);
      if (arrived()) break;
      fprintf(stderr, "[dpgo_amd] ERROR: read-back flag never arrived\n");
      if (stuck_fn_) stuck_fn_(stuck_user_);   // (a collective on this stream that never ends: its communicator aborts it now)
      throw DeviceError("read-back flag never arrived");
    }
  }
  // (debug hook: a host that comes late to every read-back -- the stream runs ahead of it by that much; the results must not
  // depend on it, tests/test_gpu_parity.py)
  const int late_us = settings().debug_late_host_us;
  if (late_us > 0) {
    const auto until = std::chrono::steady_clock::now() + std::chrono::microseconds(late_us);
    while (std::chrono::steady_clock::now() < until) __builtin_ia32_pause();
  }
}

// ---------------------------------------------------------------------------
// segments
// ---------------------------------------------------------------------------
void Schedule::destroy_graphs() {
  for (auto &g : graphs_)
    if (g.exec) (void)hipGraphExecDestroy(g.exec);
  graphs_.clear();
}

void Schedule::invalidate() {
  graph_gen_++;
  seg_captures_live_ = 0;   // (the cap below is on captures of one generation of arguments, not of the group's life)
  if (graphs_.empty()) return;
  if (drain(60.0)) destroy_graphs();
  else graphs_.clear();
}

void Schedule::flush_deferred() {
  if (deferred_.empty()) return;
  std::vector<std::function<void()>> d;
  d.swap(deferred_);
  deferred_key_ = 0;
  for (auto &f : d) f();
}

void Schedule::segment(const std::vector<unsigned long long> *key, const std::function<void()> &body_in) {
  // launches that were waiting for a segment to carry them (Group::step()) become its head
  std::vector<std::function<void()>> pro;
  pro.swap(deferred_);
  deferred_key_ = 0;
  const std::function<void()> with_pro = [&] {
    for (auto &f : pro) f();
    body_in();
  };
  const std::function<void()> &body = pro.empty() ? body_in : with_pro;
  if (!key) {
    seg_eager_++;
    const auto t0 = std::chrono::steady_clock::now();
    body();
    if (host_timing_) t_eager_seg_ += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return;
  }
  SegGraph *hit = nullptr;
  for (auto &g : graphs_)
    if (g.key == *key) { hit = &g; break; }
  if (!hit && seg_captures_live_ >= 256) {
    if (!capture_cap_warned_) {
      capture_cap_warned_ = true;
      fprintf(stderr, "[dpgo_amd] WARNING: more than 256 segment variants captured without the arguments changing; further new variants "
                      "run eagerly (the replayed ones stay).\n");
    }
    // (more variants than a steady state has: whatever keeps changing, capturing it again and again is not the cure)
    seg_eager_++;
    body();
    return;
  }
  if (!hit) {
    hipGraph_t graph = nullptr;
    capturing_ = true;
    captured_flags_ = 0;
    bool ok = hipStreamBeginCapture(st_, hipStreamCaptureModeThreadLocal) == hipSuccess;
    if (ok) {
      try {
        body();
      } catch (...) {
        ok = false;
      }
      if (hipStreamEndCapture(st_, &graph) != hipSuccess) ok = false;
    }
    capturing_ = false;
    hipGraphExec_t exec = nullptr;
    if (ok && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) ok = false;
    if (graph) (void)hipGraphDestroy(graph);
    if (!ok) {
      // nothing of the body has run (a capture only records): run it eagerly, and stop trying
      (void)hipGetLastError();
      graphs_broken_ = true;
      fprintf(stderr, "[dpgo_amd] WARNING: a segment of the iteration could not be captured as a graph; eager launches from here on.\n");
      seg_eager_++;
      body();
      return;
    }
    if (graphs_.size() >= 32) {   // (a handful of keys per segment is normal: the history rotates, the iterate swaps)
      size_t old = 0;
      for (size_t i = 1; i < graphs_.size(); i++)
        if (graphs_[i].used < graphs_[old].used) old = i;
      // (never destroy a graph that may be executing: the least recently used one was replayed many read-backs ago -- the
      // flag says so -- and only if it does not is the stream waited for)
      if (__atomic_load_n(host_flag_, __ATOMIC_ACQUIRE) >= graphs_[old].done_seq || drain(60.0)) (void)hipGraphExecDestroy(graphs_[old].exec);
      graphs_.erase(graphs_.begin() + old);
    }
    graphs_.push_back(SegGraph{*key, exec, captured_flags_, 0, 0});
    hit = &graphs_.back();
    seg_captures_++;
    seg_captures_live_++;
  }
  hit->used = ++seg_clock_;
  if (host_timing_) {
    const auto t0 = std::chrono::steady_clock::now();
    HIP_CHECK(hipGraphLaunch(hit->exec, st_));
    t_graph_launch_ += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  } else
  HIP_CHECK(hipGraphLaunch(hit->exec, st_));
  seq_ += hit->flags;   // the flag-raising kernels of the replay count on from the device's own word
  hit->done_seq = seq_ + 1;   // (a flag raised BEHIND the replay says it is over: its own flag need not be its last kernel)
  seg_replays_++;
}

// ---------------------------------------------------------------------------
// the replay policy
// ---------------------------------------------------------------------------
// A host that waits most of the time (more than 40 % of it) keeps up with eager launches, which are the faster way then (a
// replay costs the GPU ~8 us of start-up); a host that waits less is what bounds the group -- a slow or busy box, a small
// graph whose kernels are shorter than a launch -- and its segments are replayed from then on.
bool Schedule::iter_graph_wanted() const {
  const int force = settings().iter_graph.value_or(-1);
  if (graphs_broken_ || force == 0 || prof_enabled()) return false;   // (never while launches are timed)
  if (force == 1) return true;
  // Where a segment streams gigabytes (the headline's eight nodes on one GPU) the host is never what bounds it, and its
  // launches shrink with the set of nodes that still iterate, which a replay's frozen grids cannot do.  Below that size:
  // replays once the host has been seen to be the slower side (count_iteration).
  return rows_ <= 40000 && host_bound_;
}

// The CG steps of a group go out as one graph replay each (a step is 13-21 launches with fixed arguments): wherever the
// segments of the iteration are replayed, and -- round 4's default, measured +8..13 % on city10000 -- from the start for
// groups of at least two nodes and at most 40 000 poses, whose steps are bound by the host's launch rate.  DPGO_CG_GRAPH=0
// keeps just these eager (A/B hook), DPGO_ITER_GRAPH=0 everything.
bool Schedule::cg_graph_wanted() const {
  if (!settings().cg_graph || settings().iter_graph == 0 || graphs_broken_ || prof_enabled()) return false;
  if (iter_graph_wanted()) return true;
  return rows_ <= 40000 && nodes_ >= 2;
}

// Every 32 iterations: the share of its time inside iterate() / update() that this group's host thread spent waiting for
// read-backs.  Measured: 0.68 at one node per GPU of the headline on an idle host (eager launches are the faster way there:
// replays cost 4-8 %), between 0.4 and 0.55 for the same on a slower box, 0.06-0.15 for sphere2500, city10000, M3500.  Below
// 0.4 the host is what bounds the group.  (The CG steps of small multi-node groups are replayed whatever this says:
// cg_graph_wanted.)
void Schedule::count_iteration() {
  if (host_bound_ || ++win_iters_ < 32) return;
  const double below = settings().host_bound_below;
  // (round 6: ... and at least half of its waits found the flag already raised -- the GPU had been waiting for the HOST.  A host
  // that enqueues ahead of the GPU's decisions -- Group::SpecUpdate -- spends less of its time waiting without being the slower side)
  const bool late = below >= 1.0 || 2 * win_nlate_ >= win_nwait_;
  if (win_lib_s_ > 0 && win_wait_s_ < below * win_lib_s_ && late) host_bound_ = true;
  win_iters_ = 0;
  win_wait_s_ = 0;
  win_lib_s_ = 0;
  win_nwait_ = win_nlate_ = 0;
}

// ---------------------------------------------------------------------------
// DPGO_HOST_TIMING=1
// ---------------------------------------------------------------------------
void Schedule::report_launches(int nodes) const {
  fprintf(stderr, "[host] node group of %d: %ld replays %.3f s in hipGraphLaunch (%.1f us each), %ld eager segments %.3f s, %ld waits %.3f s (%.1f us each)\n",
          nodes, seg_replays_, t_graph_launch_, seg_replays_ ? 1e6 * t_graph_launch_ / seg_replays_ : 0.0, seg_eager_, t_eager_seg_,
          n_wait_, t_wait_, n_wait_ ? 1e6 * t_wait_ / n_wait_ : 0.0);
}

void Schedule::report_waits() const {
  fprintf(stderr, "[host] waits of < 50 us / 200 us / 1 ms / 5 ms / 50 ms / longer: %ld %ld %ld %ld %ld %ld; segments replayed since the host was found to be the slower side: %s\n",
          wait_hist_[0], wait_hist_[1], wait_hist_[2], wait_hist_[3], wait_hist_[4], wait_hist_[5], host_bound_ ? "yes" : "no");
}

}  // namespace dpgo
