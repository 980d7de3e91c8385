// The refusal and the verdict of the anchored tangent-space Hessian's factor (hess.h), behind cov_analyse (cov.cpp).
#include "hess.h"

#include <chrono>

#include "cov_state.h"
#include "group.h"

namespace dpgo {

// Nothing that cannot fit is asked of a shared device: bytes still to allocate against half of the free memory (asked only
// when something remains).
bool Group::device_has_room(long long remain) {
  if (remain <= 0) return true;
  size_t free_b = 0, total_b = 0;
  HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
  return (unsigned long long)remain <= free_b / 2;
}

// The refusal of every consumer of the factor: device_bytes <- the sum of the parts' bytes; 1 (SKIPPED) where that is more than
// max_bytes (when > 0), or where what the parts say is still to allocate has no room; otherwise the numeric context on its
// first use -- the block-column map and spd_prepare_device -- and 0.  Nothing is allocated on a refusal.
int Group::hess_reserve(long long max_bytes, const char *who, std::initializer_list<HessPart> parts, HessAnalysis &out) {
  CovState &s = *cov_;
  long long bytes = 0, remain = 0;
  for (const HessPart &p : parts) {
    bytes += p.bytes;
    remain += p.remain;
  }
  out.device_bytes = bytes;
  if ((max_bytes > 0 && bytes > max_bytes) || !device_has_room(remain)) return 1;
  if (!s.F.numeric) {
    s.bcol.upload(s.bcol_h);
    if (spd_prepare_device(s.A, s.F) != 0) {
      fprintf(stderr, "[dpgo_amd] ERROR: %s: the device state of the factorisation could not be set up.\n", who);
      return -1;
    }
  }
  return 0;
}

// The factorisation of the values in place and its pivots: 0 factored, 1 a non-positive pivot (the verdict NOT_PD), -1 failed.
int Group::hess_refactor(const char *who, HessAnalysis &out) {
  CovState &s = *cov_;
  const int rc = spd_refactor_device(s.F, st_, false);   // (returns with the verdict read)
  if (rc != 0 && !s.F.not_pd) {
    fprintf(stderr, "[dpgo_amd] ERROR: %s: the factorisation failed on the device.\n", who);
    return -1;
  }
  out.pivot_max = s.F.pivot_max;
  out.pivot_min = s.F.pivot_max > 0 ? s.F.pivot_min : 0.0;   // (no front factored: nothing recorded)
  return rc != 0;
}

// write_H launches what writes H into spd_numeric_values(F); factor_ms runs from there to the verdict.  Returns as
// hess_refactor, behind a synchronise where the verdict is NOT_PD.
int Group::hess_factor(const char *who, const std::function<void()> &write_H, HessAnalysis &out) {
  const auto t0 = std::chrono::steady_clock::now();
  write_H();
  const int rc = hess_refactor(who, out);
  if (rc < 0) return -1;
  out.factor_ms = 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (rc != 0) HIP_CHECK(hipStreamSynchronize(st_));
  return rc;
}

}  // namespace dpgo
