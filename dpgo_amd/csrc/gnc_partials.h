// Device only: the tail the edge kernels of graduated non-convexity share (k_gnc_edge, gnc.hip; k_ml_gnc_edge, ml_gnc.hip).
// Every lane of the workgroup's one wave calls it, lanes past the last edge with the neutral values (0, 0, 0, 0, +inf, no
// flag).  Lane 0 stores the workgroup's GNC_PARTIAL_SLOTS sums and one count per flag where k_gnc_final<NC> reads them: slot s of
// workgroup b at [s * gridDim.x + b].  The sums run in wave_reduce.h's order.
#pragma once
#include <hip/hip_runtime.h>

#include "wave_reduce.h"

namespace dpgo {

// flag...: per lane, in the order of the summary's counts (w == 0, w == 1, 0 < w < 1; then near_pi over w > 0, near_pi over
// all).  They are separate bool parameters, not an array: the compiler then keeps each as a lane mask in scalar registers.
template <typename... Flag>
__device__ __forceinline__ void gnc_store_partials(double f_out, double f_ws, double f_rho, double smax, double wmin,
                                                   double *__restrict__ partials, long long *__restrict__ counts, Flag... flag) {
  constexpr int NC = sizeof...(Flag);
  const long long n[NC] = {(long long)__popcll(__ballot(flag))...};
  f_out = wave_sum(f_out);
  f_ws = wave_sum(f_ws);
  f_rho = wave_sum(f_rho);
  smax = wave_max(smax);
  wmin = wave_min(wmin);
  if (threadIdx.x == 0) {
    const size_t nb = gridDim.x, bk = blockIdx.x;
    partials[bk] = f_out;
    partials[nb + bk] = f_ws;
    partials[2 * nb + bk] = f_rho;
    partials[3 * nb + bk] = smax;
    partials[4 * nb + bk] = wmin;
#pragma unroll
    for (int c = 0; c < NC; c++) counts[c * nb + bk] = n[c];
  }
}

}  // namespace dpgo
