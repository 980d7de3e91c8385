// The kernels of the maximum-likelihood objective for gfx950 (ml.h): the edge pass, the gradient's gather, and the Gauss-Newton
// Hessian written where the factorisation reads it.  fp64 throughout, no fast-math; every sum runs in a fixed order (an edge
// list ascending, the lanes of a wave by shuffle, the workgroups' partials strided in one final wave): the same bits run to
// run, no floating-point atomics, no LDS, no inline assembly.
#include "ml.h"

#include <cmath>

#include "cov.h"
#include "edge_math.h"
#include "ml_math.h"
#include "wave_reduce.h"

namespace dpgo {
namespace {

__device__ __forceinline__ bool node_on(const NodeMask &m, int node) { return ((m.p ? (m.v & *m.p) : m.v) >> node) & 1ull; }

// FULL: r, Omega r, chi2, the gradient terms and the record [J_i | J_j | Omega J_i | Omega J_j] are written; otherwise F_ml
// and near_pi alone (the trial point)
template <int D, bool FULL>
__global__ __launch_bounds__(EDGE_BLOCK) void k_ml_edge(int m, const double2 *__restrict__ rec, const double *__restrict__ omega,
                                                        const double2 *__restrict__ poses, MlEdgeOut out,
                                                        double *__restrict__ partials, long long *__restrict__ counts) {
  constexpr int EU = edge_rec_doubles(D) / 2, PU = pose_rec_doubles(D) / 2, RS = pose_rec_doubles(D), DOF = cov_dof(D), DD = DOF * DOF;
  static_assert(edge_rec_doubles(D) % 2 == 0 && pose_rec_doubles(D) % 2 == 0, "records are whole 16-byte units");
  const int e = blockIdx.x * EDGE_BLOCK + threadIdx.x;
  double chi2 = 0;
  bool near = false;
  if (e < m) {
    double q[2 * EU];
#pragma unroll
    for (int k = 0; k < EU; k++) {
      const double2 u = rec[(size_t)e * EU + k];
      q[2 * k] = u.x;
      q[2 * k + 1] = u.y;
    }
    int i, j;
    bool inter;
    edge_head(q, i, j, inter);
    double a[RS], b[RS];
#pragma unroll
    for (int k = 0; k < PU; k++) {
      const double2 u = poses[(size_t)i * PU + k], v = poses[(size_t)j * PU + k];
      a[2 * k] = u.x;
      a[2 * k + 1] = u.y;
      b[2 * k] = v.x;
      b[2 * k + 1] = v.y;
    }
    double Om[DD], r[DOF], wr[DOF], Ji[DD], Jj[DD];
#pragma unroll
    for (int k = 0; k < DD; k++) Om[k] = omega[(size_t)e * DD + k];
    near = ml_residual<D>(q, a, b, r, Ji, Jj);
    chi2 = ml_weigh<D>(Om, r, wr);
    if (FULL) {
      out.chi2[e] = chi2;
      double *jw = out.jw + (size_t)e * 4 * DD;
#pragma unroll
      for (int k = 0; k < DOF; k++) {
        out.r[(size_t)e * DOF + k] = r[k];
        out.wr[(size_t)e * DOF + k] = wr[k];
        out.g[(size_t)2 * e * DOF + k] = ml_grad_entry<D>(Ji, wr, k);
        out.g[((size_t)2 * e + 1) * DOF + k] = ml_grad_entry<D>(Jj, wr, k);
      }
#pragma unroll
      for (int k = 0; k < DD; k++) {
        jw[k] = Ji[k];
        jw[DD + k] = Jj[k];
      }
#pragma unroll
      for (int k = 0; k < DOF; k++)
#pragma unroll
        for (int c = 0; c < DOF; c++) {
          jw[2 * DD + k * DOF + c] = ml_w_entry<D>(Om, Ji, k, c);
          jw[3 * DD + k * DOF + c] = ml_w_entry<D>(Om, Jj, k, c);
        }
    }
  }
  const long long n_near = __popcll(__ballot(near));
  chi2 = wave_sum(chi2);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = chi2;
    counts[blockIdx.x] = n_near;
  }
}

// F_ml = 1/2 of the partials' sum in strided order; and F where the polish's reduction will look for it: fslot[0] = F, the
// other nslot - 1 partials of that slot zero
__global__ __launch_bounds__(64) void k_ml_final(int nb, const double *__restrict__ partials, const long long *__restrict__ counts,
                                                 MlSummaryDev *__restrict__ sum, double *__restrict__ fslot, int nslot) {
  const int lane = threadIdx.x;
  double f = 0;
  long long nn = 0;
  for (int k = lane; k < nb; k += 64) {
    f += partials[k];
    nn += counts[k];
  }
  f = wave_sum(f);
  nn = wave_sum(nn);
  if (fslot)
    for (int k = lane == 0 ? 64 : lane; k < nslot; k += 64) fslot[k] = 0.0;
  if (lane == 0) {
    sum->F = 0.5 * f;
    sum->near_pi = nn;
    if (fslot) fslot[0] = 0.5 * f;
  }
}

template <int D>
__global__ __launch_bounds__(SEG_ROWS) void k_ml_gather(const Seg *segs, NodeMask mask, const int *__restrict__ inc_ptr,
                                                        const int *__restrict__ inc, const double *__restrict__ ge, int anchor,
                                                        double *__restrict__ g, int slot_g2, double *partial, int nseg) {
  constexpr int DOF = cov_dof(D);
  const Seg s = segs[blockIdx.x];
  if (!node_on(mask, s.node)) return;
  const int row = s.begin + threadIdx.x;
  double g2 = 0;
  if (row < s.end) {
    double acc[DOF];
#pragma unroll
    for (int k = 0; k < DOF; k++) acc[k] = 0.0;
    if (row != anchor)
      for (int t = inc_ptr[row]; t < inc_ptr[row + 1]; t++) {
        const double *r = ge + (size_t)inc[t] * DOF;   // (2 e + role) terms in
#pragma unroll
        for (int k = 0; k < DOF; k++) acc[k] += r[k];
      }
#pragma unroll
    for (int k = 0; k < DOF; k++) {
      g[(size_t)row * DOF + k] = acc[k];
      g2 = fma(acc[k], acc[k], g2);
    }
  }
  g2 = wave_sum(g2);
  if (threadIdx.x == 0) partial[(size_t)slot_g2 * nseg + blockIdx.x] = g2;
}

template <int D>
__global__ __launch_bounds__(256) void k_ml_hessian(int nposes, const int *__restrict__ bptr, const int *__restrict__ bcol,
                                                    const int *__restrict__ blk_ptr, const int *__restrict__ blk,
                                                    const double *__restrict__ jw, int anchor, double *__restrict__ val) {
  constexpr int DOF = cov_dof(D), JW = 4 * DOF * DOF;
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= nposes) return;
  const int b0 = bptr[p], nb = bptr[p + 1] - b0, rowlen = DOF * nb, len = DOF * rowlen;
  const size_t base_out = (size_t)DOF * DOF * b0;
  for (int l = lane; l < len; l += 64) {
    const int a = l / rowlen, rem = l - a * rowlen, j = rem / DOF, b = rem - j * DOF;
    const int q = bcol[b0 + j];
    if (p == anchor || q == anchor) {   // the gauge: the anchor's row and column are those of the identity
      val[base_out + l] = (p == q && a == b) ? 1.0 : 0.0;
      continue;
    }
    double acc = 0.0;
    for (int t = blk_ptr[b0 + j]; t < blk_ptr[b0 + j + 1]; t++) {
      const int it = blk[t];
      acc += ml_block_entry<D>(jw + (size_t)(it >> 2) * JW, (it >> 1) & 1, it & 1, a, b);
    }
    val[base_out + l] = acc;
  }
}

}  // namespace

void launch_ml_edge(int d, hipStream_t st, int m, const double *rec, const double *omega, const double *X, const MlEdgeOut &out,
                    double *partials, long long *counts, MlSummaryDev *sum, double *fslot, int nslot) {
  if (m <= 0) return;
  const int nb = (m + EDGE_BLOCK - 1) / EDGE_BLOCK;
  const double2 *r2 = (const double2 *)rec, *x2 = (const double2 *)X;
  if (d == 3) {
    if (out.r) hipLaunchKernelGGL((k_ml_edge<3, true>), dim3(nb), dim3(EDGE_BLOCK), 0, st, m, r2, omega, x2, out, partials, counts);
    else hipLaunchKernelGGL((k_ml_edge<3, false>), dim3(nb), dim3(EDGE_BLOCK), 0, st, m, r2, omega, x2, out, partials, counts);
  } else {
    if (out.r) hipLaunchKernelGGL((k_ml_edge<2, true>), dim3(nb), dim3(EDGE_BLOCK), 0, st, m, r2, omega, x2, out, partials, counts);
    else hipLaunchKernelGGL((k_ml_edge<2, false>), dim3(nb), dim3(EDGE_BLOCK), 0, st, m, r2, omega, x2, out, partials, counts);
  }
  hipLaunchKernelGGL(k_ml_final, dim3(1), dim3(64), 0, st, nb, partials, counts, sum, fslot, nslot);
}

void launch_ml_gather(const LaunchCtx &lc, const int *inc_ptr, const int *inc, const double *ge, int anchor, double *g, int slot_g2,
                      double *partials) {
  const auto &[d, st, T, mask] = lc;
  if (T.nseg_own == 0) return;
  if (d == 3)
    hipLaunchKernelGGL(k_ml_gather<3>, dim3(T.nseg_own), dim3(SEG_ROWS), 0, st, T.segs, mask, inc_ptr, inc, ge, anchor, g, slot_g2,
                       partials, T.nseg_own);
  else
    hipLaunchKernelGGL(k_ml_gather<2>, dim3(T.nseg_own), dim3(SEG_ROWS), 0, st, T.segs, mask, inc_ptr, inc, ge, anchor, g, slot_g2,
                       partials, T.nseg_own);
}

void launch_ml_hessian(int d, hipStream_t st, int nposes, const int *bptr, const int *bcol, const int *blk_ptr, const int *blk,
                       const double *jw, int anchor, double *val) {
  if (nposes == 0) return;
  if (d == 3)
    hipLaunchKernelGGL(k_ml_hessian<3>, dim3((nposes + 3) / 4), dim3(256), 0, st, nposes, bptr, bcol, blk_ptr, blk, jw, anchor, val);
  else
    hipLaunchKernelGGL(k_ml_hessian<2>, dim3((nposes + 3) / 4), dim3(256), 0, st, nposes, bptr, bcol, blk_ptr, blk, jw, anchor, val);
}

}  // namespace dpgo
