// The kernels of the robust objective for gfx950 (robust.h): per-edge values and rows, the weighted gather, M_w, and the
// rank-one curvature terms behind k_cov_hessian.  fp64 throughout, no fast-math; every sum runs in a fixed order (an edge
// list ascending, the lanes of a wave by shuffle, the workgroups' partials strided in one final wave): the same bits run to
// run, no floating-point atomics, no LDS, no inline assembly.
#include "robust.h"

#include <cmath>

#include "cov.h"
#include "robust_math.h"
#include "wave_reduce.h"

namespace dpgo {
namespace {

__device__ __forceinline__ bool node_on(const NodeMask &m, int node) { return ((m.p ? (m.v & *m.p) : m.v) >> node) & 1ull; }

// k_edge_eval (edges.hip) on the group's record array of X, with c_e and, behind with_rows, the rows of M_e X
template <int D>
__global__ __launch_bounds__(EDGE_BLOCK) void k_robust_edge(int m, const double2 *__restrict__ rec, const double2 *__restrict__ poses,
                                                            int loss, double dl, double *__restrict__ out, double *__restrict__ rows,
                                                            double *__restrict__ partials, long long *__restrict__ counts) {
  constexpr int EU = edge_rec_doubles(D) / 2, PU = pose_rec_doubles(D) / 2, RS = pose_rec_doubles(D);
  static_assert(edge_rec_doubles(D) % 2 == 0 && pose_rec_doubles(D) % 2 == 0, "records are whole 16-byte units");
  const int e = blockIdx.x * EDGE_BLOCK + threadIdx.x;
  double f_intra = 0, f_inter = 0, wmin = INFINITY;
  bool is_inter = false, down = false;
  if (e < m) {
    double q[2 * EU];
#pragma unroll
    for (int k = 0; k < EU; k++) {
      const double2 u = rec[(size_t)e * EU + k];
      q[2 * k] = u.x;
      q[2 * k + 1] = u.y;
    }
    int i, j;
    edge_head(q, i, j, is_inter);
    double a[RS], b[RS];
#pragma unroll
    for (int k = 0; k < PU; k++) {
      const double2 u = poses[(size_t)i * PU + k], v = poses[(size_t)j * PU + k];
      a[2 * k] = u.x;
      a[2 * k + 1] = u.y;
      b[2 * k] = v.x;
      b[2 * k + 1] = v.y;
    }
    double v[4];
    edge_lane<D>(q, a, b, is_inter, loss, dl, v);
    const double s_rot = v[0], s_trans = v[1], rho = v[2], w = v[3];
    double s;
    {
#pragma clang fp contract(off)
      s = s_rot + s_trans;
    }
    out[e] = s_rot;
    out[(size_t)m + e] = s_trans;
    out[2 * (size_t)m + e] = rho;
    out[3 * (size_t)m + e] = w;
    out[4 * (size_t)m + e] = robust_curv(loss, dl, s, w, is_inter);
    if (rows) {
      double ri[RS], rj[RS];
      robust_rows<D>(q, a, b, ri, rj);
      double2 *dst = (double2 *)rows + (size_t)e * 2 * PU;
#pragma unroll
      for (int k = 0; k < PU; k++) {
        dst[k] = make_double2(ri[2 * k], ri[2 * k + 1]);
        dst[PU + k] = make_double2(rj[2 * k], rj[2 * k + 1]);
      }
    }
    if (is_inter) f_inter = rho;
    else f_intra = rho;
    wmin = w;
    down = w < 1.0;
  }
  const long long n_inter = __popcll(__ballot(is_inter)), n_down = __popcll(__ballot(down));
  f_intra = wave_sum(f_intra);
  f_inter = wave_sum(f_inter);
  wmin = wave_min(wmin);
  if (threadIdx.x == 0) {
    const size_t nb = gridDim.x, bk = blockIdx.x;
    partials[bk] = f_intra;
    partials[nb + bk] = f_inter;
    partials[2 * nb + bk] = wmin;
    counts[bk] = n_inter;
    counts[nb + bk] = n_down;
  }
}

// k_edge_final, and F where the polish's reduction will look for it: fslot[0] = F, the other nslot - 1 partials of that slot zero
__global__ __launch_bounds__(64) void k_robust_final(int nb, const double *__restrict__ partials, const long long *__restrict__ counts,
                                                     EdgeSummaryDev *__restrict__ sum, double *__restrict__ fslot, int nslot) {
  const int lane = threadIdx.x;
  double fi = 0, fe = 0, wmin = INFINITY;
  long long ni = 0, nd = 0;
  for (int k = lane; k < nb; k += 64) {
    fi += partials[k];
    fe += partials[(size_t)nb + k];
    wmin = fmin(wmin, partials[2 * (size_t)nb + k]);
    ni += counts[k];
    nd += counts[(size_t)nb + k];
  }
  fi = wave_sum(fi);
  fe = wave_sum(fe);
  wmin = wave_min(wmin);
  ni = wave_sum(ni);
  nd = wave_sum(nd);
  if (fslot)
    for (int k = lane == 0 ? 64 : lane; k < nslot; k += 64) fslot[k] = 0.0;
  if (lane == 0) {
    sum->F_intra = 0.5 * fi;
    sum->F_inter = 0.5 * fe;
    sum->weight_min = wmin;
    sum->num_inter = ni;
    sum->num_downweighted = nd;
    if (fslot) fslot[0] = 0.5 * fi + 0.5 * fe;
  }
}

template <int D>
__global__ __launch_bounds__(SEG_ROWS) void k_robust_gather(const Seg *segs, NodeMask mask, const int *__restrict__ inc_ptr,
                                                            const int *__restrict__ inc, const double *__restrict__ w,
                                                            const double *__restrict__ rows, double *__restrict__ MX) {
  constexpr int RS = (D + 1) * D;
  const Seg s = segs[blockIdx.x];
  if (!node_on(mask, s.node)) return;
  const int row = s.begin + threadIdx.x;
  if (row >= s.end) return;
  double acc[RS];
#pragma unroll
  for (int k = 0; k < RS; k++) acc[k] = 0.0;
  for (int t = inc_ptr[row]; t < inc_ptr[row + 1]; t++) {
    const int it = inc[t];
    const double we = w[it >> 1];
    const double *r = rows + (size_t)it * RS;   // (2 e + role) records in
#pragma unroll
    for (int k = 0; k < RS; k++) acc[k] = fma(we, r[k], acc[k]);
  }
#pragma unroll
  for (int k = 0; k < RS; k++) MX[(size_t)row * RS + k] = acc[k];
}

template <int D>
__global__ __launch_bounds__(256) void k_robust_mval(int nposes, const int *__restrict__ bptr, const int *__restrict__ blk_ptr,
                                                     const int *__restrict__ blk, const double *__restrict__ rec,
                                                     const double *__restrict__ w, double *__restrict__ Mw) {
  constexpr int B = D + 1, L = edge_rec_doubles(D);
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= nposes) return;
  const int b0 = bptr[p], nb = bptr[p + 1] - b0, rowlen = B * nb, len = B * rowlen;
  const size_t base = (size_t)B * B * b0;
  for (int l = lane; l < len; l += 64) {
    const int r = l / rowlen, rem = l - r * rowlen, j = rem / B, c = rem - j * B;
    double acc = 0.0;
    for (int t = blk_ptr[b0 + j]; t < blk_ptr[b0 + j + 1]; t++) {
      const int it = blk[t], e = it >> 2;
      acc = fma(w[e], robust_m_entry<D>(rec + (size_t)e * L, (it >> 1) & 1, it & 1, r, c), acc);
    }
    Mw[base + l] = acc;
  }
}

template <int D>
__global__ __launch_bounds__(256) void k_robust_rank1(int nposes, const int *__restrict__ bptr, const int *__restrict__ bcol,
                                                      const int *__restrict__ blk_ptr, const int *__restrict__ blk,
                                                      const double *__restrict__ ce, const double *__restrict__ rows,
                                                      const double *__restrict__ X, int anchor, double *__restrict__ val) {
  constexpr int RS = (D + 1) * D, DOF = cov_dof(D);
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= nposes || p == anchor) return;
  const int b0 = bptr[p], nb = bptr[p + 1] - b0, rowlen = DOF * nb, len = DOF * rowlen;
  const size_t base_out = (size_t)DOF * DOF * b0;
  const double *xp = X + (size_t)p * RS;
  for (int l = lane; l < len; l += 64) {
    const int a = l / rowlen, rem = l - a * rowlen, j = rem / DOF, b = rem - j * DOF;
    const int q = bcol[b0 + j];
    if (q == anchor) continue;
    const double *xq = X + (size_t)q * RS;
    double acc = 0.0;
    bool any = false;
    for (int t = blk_ptr[b0 + j]; t < blk_ptr[b0 + j + 1]; t++) {
      const int it = blk[t], e = it >> 2;
      const double c = ce[e];
      if (c == 0.0) continue;
      const double gp = robust_ghat_entry<D>(xp, rows + ((size_t)2 * e + ((it >> 1) & 1)) * RS, a);
      const double gq = robust_ghat_entry<D>(xq, rows + ((size_t)2 * e + (it & 1)) * RS, b);
      acc = fma(c, gp * gq, acc);
      any = true;
    }
    if (any) val[base_out + l] += acc;
  }
}

}  // namespace

void launch_robust_edge(int d, hipStream_t st, int m, const double *rec, const double *X, int loss, double loss_reg, double *out,
                        double *rows, double *partials, long long *counts, EdgeSummaryDev *sum, double *fslot, int nslot) {
  if (m <= 0) return;
  const int nb = (m + EDGE_BLOCK - 1) / EDGE_BLOCK;
  if (d == 3)
    hipLaunchKernelGGL(k_robust_edge<3>, dim3(nb), dim3(EDGE_BLOCK), 0, st, m, (const double2 *)rec, (const double2 *)X, loss,
                       loss_reg, out, rows, partials, counts);
  else
    hipLaunchKernelGGL(k_robust_edge<2>, dim3(nb), dim3(EDGE_BLOCK), 0, st, m, (const double2 *)rec, (const double2 *)X, loss,
                       loss_reg, out, rows, partials, counts);
  hipLaunchKernelGGL(k_robust_final, dim3(1), dim3(64), 0, st, nb, partials, counts, sum, fslot, nslot);
}

void launch_robust_gather(const LaunchCtx &lc, const int *inc_ptr, const int *inc, const double *w, const double *rows, double *MX) {
  const auto &[d, st, T, mask] = lc;
  if (T.nseg_own == 0) return;
  if (d == 3)
    hipLaunchKernelGGL(k_robust_gather<3>, dim3(T.nseg_own), dim3(SEG_ROWS), 0, st, T.segs, mask, inc_ptr, inc, w, rows, MX);
  else
    hipLaunchKernelGGL(k_robust_gather<2>, dim3(T.nseg_own), dim3(SEG_ROWS), 0, st, T.segs, mask, inc_ptr, inc, w, rows, MX);
}

void launch_robust_mval(int d, hipStream_t st, int nposes, const int *bptr, const int *blk_ptr, const int *blk, const double *rec,
                        const double *w, double *Mw) {
  if (nposes == 0) return;
  if (d == 3)
    hipLaunchKernelGGL(k_robust_mval<3>, dim3((nposes + 3) / 4), dim3(256), 0, st, nposes, bptr, blk_ptr, blk, rec, w, Mw);
  else
    hipLaunchKernelGGL(k_robust_mval<2>, dim3((nposes + 3) / 4), dim3(256), 0, st, nposes, bptr, blk_ptr, blk, rec, w, Mw);
}

void launch_robust_rank1(int d, hipStream_t st, int nposes, const int *bptr, const int *bcol, const int *blk_ptr, const int *blk,
                         const double *c, const double *rows, const double *X, int anchor, double *val) {
  if (nposes == 0) return;
  if (d == 3)
    hipLaunchKernelGGL(k_robust_rank1<3>, dim3((nposes + 3) / 4), dim3(256), 0, st, nposes, bptr, bcol, blk_ptr, blk, c, rows, X,
                       anchor, val);
  else
    hipLaunchKernelGGL(k_robust_rank1<2>, dim3((nposes + 3) / 4), dim3(256), 0, st, nposes, bptr, bcol, blk_ptr, blk, c, rows, X,
                       anchor, val);
}

}  // namespace dpgo
