// The kernels of a Newton step for gfx950 (polish.h): the tangent gradient, the Levenberg-Marquardt shift inside the
// factorisation's value array, the retraction.
//
// One wave per own segment of the group's SegTable, lane = pose, on the certificate's record buffers (cert_state.h).  fp64
// throughout, no fast-math.  Every sum is a fixed tree -- lanes of a wave, then the segments in order (k_polish_reduce): the
// same bits run to run, no floating-point atomics.
#include "polish.h"

#include "cov.h"
#include "wave_reduce.h"

namespace dpgo {
namespace {

__device__ __forceinline__ bool node_on(const NodeMask &m, int node) { return ((m.p ? (m.v & *m.p) : m.v) >> node) & 1ull; }

template <int D>
__global__ __launch_bounds__(SEG_ROWS) void k_polish_grad(const Seg *segs, NodeMask mask, const double *__restrict__ X,
                                                          const double *__restrict__ MX, int anchor, double *__restrict__ g,
                                                          int slot_g2, int slot_F, double *partial, int nseg) {
  constexpr int RS = (D + 1) * D, DOF = cov_dof(D);
  const Seg s = segs[blockIdx.x];
  if (!node_on(mask, s.node)) return;
  const int row = s.begin + threadIdx.x;
  double g2 = 0, F = 0;
  if (row < s.end) {
    double x[RS], mx[RS], gr[DOF];
#pragma unroll
    for (int k = 0; k < RS; k++) {
      x[k] = X[(size_t)row * RS + k];
      mx[k] = MX[(size_t)row * RS + k];
      F = fma(x[k], mx[k], F);
    }
#pragma unroll
    for (int a = 0; a < D; a++) gr[a] = mx[a];
#pragma unroll
    for (int k = 0; k < DOF - D; k++) {
      int r1, r2;
      cov_rot_rows<D>(k, r1, r2);
      double v = 0;
#pragma unroll
      for (int c = 0; c < D; c++) v = fma(x[D + r2 * D + c], mx[D + r1 * D + c], fma(-x[D + r1 * D + c], mx[D + r2 * D + c], v));
      gr[D + k] = v;
    }
#pragma unroll
    for (int a = 0; a < DOF; a++) {
      const double v = row == anchor ? 0.0 : gr[a];
      if (g) g[(size_t)row * DOF + a] = v;
      g2 = fma(v, v, g2);
    }
  }
  g2 = wave_sum(g2);
  F = wave_sum(0.5 * F);
  if (threadIdx.x == 0) {
    if (slot_g2 >= 0) partial[(size_t)slot_g2 * nseg + blockIdx.x] = g2;
    partial[(size_t)slot_F * nseg + blockIdx.x] = F;
  }
}

template <int D>
__global__ __launch_bounds__(SEG_ROWS) void k_polish_shift(const Seg *segs, NodeMask mask, const int *__restrict__ bptr,
                                                           const int *__restrict__ diag_pose, int anchor, double mu, int save,
                                                           double *__restrict__ hdiag, double *__restrict__ val, int slot_hmax,
                                                           double *partial, int nseg) {
  constexpr int DOF = cov_dof(D);
  const Seg s = segs[blockIdx.x];
  if (!node_on(mask, s.node)) return;
  const int row = s.begin + threadIdx.x;
  double hm = -__builtin_huge_val();
  if (row < s.end) {
    const int b0 = bptr[row], nb = bptr[row + 1] - b0;
    int jd = -1;
    for (int j = 0; j < nb; j++)
      if (diag_pose[b0 + j] >= 0) jd = j;
    if (jd >= 0) {
      double *blk = val + (size_t)DOF * DOF * b0 + (size_t)jd * DOF;
#pragma unroll
      for (int a = 0; a < DOF; a++) {
        double *e = blk + (size_t)a * DOF * nb + a;
        double h;
        if (save) {
          h = *e;
          hdiag[(size_t)row * DOF + a] = h;
        } else {
          h = hdiag[(size_t)row * DOF + a];
        }
        if (row != anchor) {
          hm = fmax(hm, h);
          *e = h + mu;
        }
      }
    }
  }
  hm = wave_max(hm);
  if (threadIdx.x == 0 && save) partial[(size_t)slot_hmax * nseg + blockIdx.x] = hm;
}

template <int D>
__global__ __launch_bounds__(SEG_ROWS) void k_polish_retract(const Seg *segs, NodeMask mask, const double *__restrict__ X,
                                                             const double *__restrict__ sol, const double *__restrict__ g,
                                                             int anchor, double *__restrict__ Z, int slot_gd, int slot_dd,
                                                             double *partial, int nseg) {
  constexpr int RS = (D + 1) * D, DOF = cov_dof(D);
  const Seg s = segs[blockIdx.x];
  if (!node_on(mask, s.node)) return;
  const int row = s.begin + threadIdx.x;
  double gd = 0, dd = 0;
  if (row < s.end) {
    double x[RS], z[RS];
#pragma unroll
    for (int k = 0; k < RS; k++) x[k] = X[(size_t)row * RS + k];
    if (row == anchor) {
#pragma unroll
      for (int k = 0; k < RS; k++) z[k] = x[k];
    } else {
      double dl[DOF];
#pragma unroll
      for (int a = 0; a < DOF; a++) {
        dl[a] = -sol[(size_t)row * DOF + a];
        gd = fma(g[(size_t)row * DOF + a], dl[a], gd);
        dd = fma(dl[a], dl[a], dd);
      }
#pragma unroll
      for (int a = 0; a < D; a++) z[a] = x[a] + dl[a];
      if constexpr (D == 2) {
        const double c = cos(dl[2]), sn = sin(dl[2]);
#pragma unroll
        for (int j = 0; j < 2; j++) {
          z[2 + j] = fma(c, x[2 + j], sn * x[4 + j]);
          z[4 + j] = fma(c, x[4 + j], -(sn * x[2 + j]));
        }
      } else {
        const double w0 = dl[D], w1 = dl[D + 1], w2 = dl[D + 2];
        const double t2 = fma(w0, w0, fma(w1, w1, w2 * w2));
        double a, b;
        if (t2 < 1e-8) {
          a = 1.0 - t2 / 6.0;
          b = 0.5 - t2 / 24.0;
        } else {
          const double th = sqrt(t2), sh = sin(0.5 * th);
          a = sin(th) / th;
          b = 2.0 * sh * sh / t2;
        }
        // Exp(K)^T Y = Y - a K Y + b K (K Y), K = hat(omega), column by column
#pragma unroll
        for (int j = 0; j < D; j++) {
          const double y0 = x[D + j], y1 = x[D + D + j], y2 = x[D + 2 * D + j];
          const double k0 = fma(w1, y2, -(w2 * y1)), k1 = fma(w2, y0, -(w0 * y2)), k2 = fma(w0, y1, -(w1 * y0));
          const double q0 = fma(w1, k2, -(w2 * k1)), q1 = fma(w2, k0, -(w0 * k2)), q2 = fma(w0, k1, -(w1 * k0));
          z[D + j] = fma(b, q0, fma(-a, k0, y0));
          z[D + D + j] = fma(b, q1, fma(-a, k1, y1));
          z[D + 2 * D + j] = fma(b, q2, fma(-a, k2, y2));
        }
      }
    }
#pragma unroll
    for (int k = 0; k < RS; k++) Z[(size_t)row * RS + k] = z[k];
  }
  gd = wave_sum(gd);
  dd = wave_sum(dd);
  if (threadIdx.x == 0) {
    partial[(size_t)slot_gd * nseg + blockIdx.x] = gd;
    partial[(size_t)slot_dd * nseg + blockIdx.x] = dd;
  }
}

// One wave per slot: the segments' partials in a fixed order, the result straight into pinned host memory; the last wave to
// arrive raises the group's read-back flag (the protocol of k_cert_reduce, cert.hip).
__global__ __launch_bounds__(64) void k_polish_reduce(int nseg, unsigned max_mask, const double *partials, double *host,
                                                      unsigned *arrived, unsigned long long *host_flag, unsigned long long seq,
                                                      unsigned long long *dev_seq) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const double *p = partials + (size_t)s * nseg;
  const bool is_max = (max_mask >> s) & 1u;
  double v = is_max ? -__builtin_huge_val() : 0.0;
  for (int k = lane; k < nseg; k += 64) v = is_max ? fmax(v, p[k]) : v + p[k];
  v = is_max ? wave_max(v) : wave_sum(v);
  if (lane == 0) {
    __hip_atomic_store(host + s, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __atomic_thread_fence(__ATOMIC_RELEASE);
    const unsigned done = __hip_atomic_fetch_add(arrived, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_SYSTEM);
    if (done == gridDim.x - 1) {
      __hip_atomic_store(arrived, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (seq == 0) seq = *dev_seq + 1;
      *dev_seq = seq;
      __hip_atomic_store(host_flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

}  // namespace

#define POLISH_DISPATCH_D(d, ...)      \
  do {                                 \
    if ((d) == 3) {                    \
      constexpr int D = 3;             \
      __VA_ARGS__;                     \
    } else {                           \
      constexpr int D = 2;             \
      __VA_ARGS__;                     \
    }                                  \
  } while (0)

void launch_polish_grad(const LaunchCtx &lc, const double *X, const double *MX, int anchor, double *g, int slot_g2, int slot_F,
                        double *partials) {
  const auto &[d, st, T, mask] = lc;
  if (T.nseg_own == 0) return;
  POLISH_DISPATCH_D(d, hipLaunchKernelGGL((k_polish_grad<D>), dim3(T.nseg_own), dim3(SEG_ROWS), 0, st, T.segs, mask, X, MX, anchor, g,
                                          slot_g2, slot_F, partials, T.nseg_own));
}

void launch_polish_shift(const LaunchCtx &lc, const int *bptr, const int *diag_pose, int anchor, double mu, bool save, double *hdiag,
                         double *val, int slot_hmax, double *partials) {
  const auto &[d, st, T, mask] = lc;
  if (T.nseg_own == 0) return;
  POLISH_DISPATCH_D(d, hipLaunchKernelGGL((k_polish_shift<D>), dim3(T.nseg_own), dim3(SEG_ROWS), 0, st, T.segs, mask, bptr, diag_pose,
                                          anchor, mu, save ? 1 : 0, hdiag, val, slot_hmax, partials, T.nseg_own));
}

void launch_polish_retract(const LaunchCtx &lc, const double *X, const double *sol, const double *g, int anchor, double *Z,
                           int slot_gd, int slot_dd, double *partials) {
  const auto &[d, st, T, mask] = lc;
  if (T.nseg_own == 0) return;
  POLISH_DISPATCH_D(d, hipLaunchKernelGGL((k_polish_retract<D>), dim3(T.nseg_own), dim3(SEG_ROWS), 0, st, T.segs, mask, X, sol, g,
                                          anchor, Z, slot_gd, slot_dd, partials, T.nseg_own));
}

void launch_polish_reduce(hipStream_t st, const SegTable &T, int nslots, unsigned max_mask, const double *partials, double *host,
                          ReadbackFlag flag) {
  hipLaunchKernelGGL(k_polish_reduce, dim3(nslots), dim3(64), 0, st, T.nseg_own, max_mask, partials, host, flag.arrived, flag.host,
                     flag.seq, flag.dev_seq);
}

}  // namespace dpgo
