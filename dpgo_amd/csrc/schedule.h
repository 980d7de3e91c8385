// How a group's launches reach the GPU and how its host learns that they are done.  A Group holds one Schedule and asks it
// for the stream, for the flag of the next flag-raising launch, for a wait, for a segment run and for its counters.
//
//  * The read-back flag.  A kernel that finishes a set of sums writes them to pinned host memory and then raises a pinned
//    flag to a sequence number (kernels.h: ReadbackFlag); the host spins until the flag has reached that number (wait()).
//  * Segments (round 5).  Between two read-backs an iteration is a fixed sequence of launches whose arguments are pointers,
//    node sets and constants: everything that changes from one iteration to the next lives in device memory.  segment()
//    runs such a sequence eagerly, or -- when the host's launch rate is what bounds the group -- captures it once per key and
//    replays it with ONE submission.  Under capture a flag-raising kernel takes the device's count + 1 (sequence number 0),
//    and the host counts along when the graph is replayed.  Bitwise the same results.
//  * The replay policy, decided by measurement (count_iteration()).
//  * Deferred launches: launches that wait for the next segment to carry them (Group::step()).
//  * DPGO_HOST_TIMING=1: where the host's time goes, on stderr when the group goes.
//  * The stream's lifetime: close() waits for it with a bound, then frees -- or leaks -- what the device might still touch.
#pragma once
#include <chrono>
#include <functional>
#include <thread>
#include <vector>

#include <hip/hip_runtime.h>

#include "devbuf.h"
#include "kernels.h"
#include "settings.h"

namespace dpgo {

// Poll `st` until it is idle or has failed, until done() holds, or for at most `seconds`: the last hipStreamQuery result
// (hipErrorNotReady: done() or the deadline came first).  hipStreamSynchronize would wait for ever behind an exchange
// whose peer is gone.
template <class Done>
hipError_t poll_stream(hipStream_t st, double seconds, std::chrono::microseconds nap, Done done) {
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    const hipError_t q = hipStreamQuery(st);
    if (q != hipErrorNotReady || done()) return q;
    if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > seconds) return q;
    std::this_thread::sleep_for(nap);
  }
}
inline hipError_t poll_stream(hipStream_t st, double seconds) {
  return poll_stream(st, seconds, std::chrono::microseconds(50), [] { return false; });
}

class Schedule {
 public:
  Schedule() = default;
  Schedule(const Schedule &) = delete;
  Schedule &operator=(const Schedule &) = delete;
  ~Schedule() { close(60.0); }

  // ---- the stream and the pinned block
  // The stream, the flag's device words and the pinned block: `front` doubles, the flag one cache line further on a cache line
  // of its own, then `back` doubles.  rows / nodes: the group's own rows and nodes (the replay policy).
  void open(size_t front, size_t back, int rows, int nodes);
  hipStream_t stream() const { return st_; }
  double *pinned_front() const { return pinned_; }
  double *pinned_back() const { return back_; }
  // Wait until the stream is idle, for at most `seconds`: true when it is.
  bool drain(double seconds) const { return !st_ || poll_stream(st_, seconds) == hipSuccess; }
  // drain(seconds), then the graphs, the pinned block and the stream go.  A stream that never drains -- it waits for an exchange
  // whose peer is gone, or a kernel faulted -- keeps them, LEAKED rather than freed under the device's feet, and from then on
  // no device buffer is freed (dev_leak_buffers: hipFree would wait for the stuck stream).  Returns whether it drained.
  bool close(double seconds);

  // ---- the read-back flag
  // what the next flag-raising launch carries: a fresh sequence number, or 0 under capture
  ReadbackFlag flag() {
    unsigned long long seq = 0;
    if (capturing_) captured_flags_++;
    else seq = ++seq_;
    return ReadbackFlag{arrived_.p, host_flag_, seq, dev_seq_.p};
  }
  unsigned long long last_seq() const { return seq_; }   // the last sequence number given out (or counted for a replay)
  // (test hooks, Group::debug_cg_scalars: the value the host's flag holds now; the arrival counter, read with a copy)
  unsigned long long flag_value() const { return __atomic_load_n(host_flag_, __ATOMIC_ACQUIRE); }
  unsigned arrived_count() const;
  // Wait until the kernel that raises the flag to `seq` (or a later one of the in-order stream) has run: seeing the flag
  // means everything enqueued before that kernel is done.
  void wait(unsigned long long seq);
  // called when a wait ran into its deadline, before the error is raised (a collective enqueued on the stream never ends)
  void set_stuck_handler(void (*fn)(void *), void *user) { stuck_fn_ = fn; stuck_user_ = user; }

  // ---- segments
  bool capturing() const { return capturing_; }
  unsigned long long graph_gen() const { return graph_gen_; }   // bumped by whatever invalidates captured arguments
  // Run `body` behind the deferred launches: eagerly without a key, else as the replay of the graph captured under *key
  // (captured now if there is none).  The key holds everything the launches carry that can change (Group::segment).
  void segment(const std::vector<unsigned long long> *key, const std::function<void()> &body);
  // Whatever a captured launch carries by value has changed (operators re-uploaded, panels re-cut, options set): the graphs
  // go.  A graph that may still be executing must not be destroyed, so the stream is drained first -- bounded; a stream that
  // never drains keeps (leaks) its graphs.
  void invalidate();

  // ---- the replay policy
  // Whether segments are replayed.  A group starts with eager launches and keeps an eye on how much of the time it spends
  // inside iterate() / update() is waiting for the GPU (count_iteration); DPGO_ITER_GRAPH=0 / 1 forces either.
  bool iter_graph_wanted() const;
  // Whether the CG steps are replayed (tnt.cpp): wherever the segments are, and for small groups of several nodes from the start.
  bool cg_graph_wanted() const;
  void count_iteration();   // once per iteration (update())
  // iterate() / update() hold one while they run: the caller's own time between the calls is not the library's host being slow
  struct InLib {
    Schedule &s;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    explicit InLib(Schedule &ss) : s(ss) {}
    ~InLib() { s.win_lib_s_ += std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count(); }
  };

  // ---- deferred launches (captured pointer values, launched in order as the head of the next segment; key: what the
  // segment's key holds for them)
  void arm_defer(bool on) { defer_armed_ = on; }
  bool defer_armed() const { return defer_armed_; }
  void defer(unsigned long long key, std::function<void()> fn) {
    deferred_.push_back(std::move(fn));
    deferred_key_ = deferred_key_ * 1000003ull + key;
  }
  // launched now, or -- while armed (Group::step()) -- deferred
  void submit(unsigned long long key, std::function<void()> fn) {
    if (!defer_armed_) { fn(); return; }
    defer(key, std::move(fn));
  }
  bool has_deferred() const { return !deferred_.empty(); }
  unsigned long long deferred_key() const { return deferred_.empty() ? 0ull : deferred_key_; }   // (part of a segment's key)
  void flush_deferred();   // launched now
  void drop_deferred() { deferred_.clear(); deferred_key_ = 0; }

  // ---- counters
  void stats(long *replays, long *captures, long *eager) const { *replays = seg_replays_; *captures = seg_captures_; *eager = seg_eager_; }
  bool host_timing() const { return host_timing_; }
  void report_launches(int nodes) const;   // the [host] lines of DPGO_HOST_TIMING=1
  void report_waits() const;

 private:
  hipStream_t st_ = nullptr;
  double *pinned_ = nullptr, *back_ = nullptr;
  unsigned long long *host_flag_ = nullptr, seq_ = 0;
  DevBuf<unsigned> arrived_;                 // the zeroed counter the workgroups of a flag-raising launch arrive at
  DevBuf<unsigned long long> dev_seq_;       // the device's copy of the last sequence number a kernel raised the flag to
  void (*stuck_fn_)(void *) = nullptr;
  void *stuck_user_ = nullptr;
  int rows_ = 0, nodes_ = 0;

  // done_seq: once the read-back flag has reached it, the graph's last replay is over (it may be destroyed)
  struct SegGraph { std::vector<unsigned long long> key; hipGraphExec_t exec = nullptr; int flags = 0; unsigned long long used = 0, done_seq = 0; };
  std::vector<SegGraph> graphs_;
  unsigned long long seg_clock_ = 0, graph_gen_ = 0;
  bool capturing_ = false, graphs_broken_ = false;
  int captured_flags_ = 0;
  long seg_replays_ = 0, seg_captures_ = 0, seg_eager_ = 0, seg_captures_live_ = 0;   // _live_: since the last invalidate()
  bool capture_cap_warned_ = false;
  void destroy_graphs();   // (the stream is known to be idle)

  bool host_bound_ = false;
  double win_wait_s_ = 0, win_lib_s_ = 0;   // of the window: seconds waiting for read-backs / seconds inside iterate() and update()
  int win_iters_ = 0;
  long win_nwait_ = 0, win_nlate_ = 0;      // of the window: waits for a read-back, and those that found it there already

  std::vector<std::function<void()>> deferred_;
  unsigned long long deferred_key_ = 0;
  bool defer_armed_ = false;

  // DPGO_HOST_TIMING=1: seconds in hipGraphLaunch, in eagerly launched segments, in waits
  bool host_timing_ = settings().host_timing;
  double t_graph_launch_ = 0, t_eager_seg_ = 0, t_wait_ = 0;
  long n_wait_ = 0, wait_hist_[6] = {0, 0, 0, 0, 0, 0};   // waits of < 50 us, < 200 us, < 1 ms, < 5 ms, < 50 ms, longer
};

}  // namespace dpgo
