// The reductions over the 64 lanes of a wave, device only: lane 0 ends with the result, the other lanes with partial ones.
// The order is fixed -- lane l takes lane l + 32, then l + 16, ... l + 1 -- and every "the same bits run to run" in this
// library's headers rests on it: a sum that changes this order changes results.
#pragma once
#include <hip/hip_runtime.h>

namespace dpgo {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_down(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
  return v;
}

}  // namespace dpgo
