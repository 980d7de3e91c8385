// Per-edge residuals, loss values and weights on gfx950 (edges.h has the definitions).
//
// k_edge_eval<D>: one lane per edge in graph order, one wave per workgroup.  A lane reads its edge record and the two pose
// records it names as whole 16-byte units (global_load_dwordx4), evaluates s_rot, s_trans, rho and w in fp64 and writes the
// four values to four arrays (consecutive lanes, consecutive doubles).  The summary is reduced the project's way: wave
// shuffles, one partial per workgroup written by lane 0, then k_edge_final -- one wave that adds the partials in a fixed
// strided order.  No atomics, no LDS, no inline assembly: a second call gives the same bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "edge_math.h"
#include "edges.h"
#include "wave_reduce.h"

namespace dpgo {

namespace {

template <int D>
__global__ __launch_bounds__(EDGE_BLOCK) void k_edge_eval(int m, const double2 *__restrict__ rec,
                                                          const double2 *__restrict__ poses, int loss, double dl,
                                                          double *__restrict__ out, double *__restrict__ partials,
                                                          long long *__restrict__ counts) {
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
    double a[RS], b[RS];   // [t | rows of Y] of pose i and of pose j
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
    const double s_rot = v[0], s_trans = v[1], rho = v[2], w = v[3];   // (rho = s on an intra edge)
    out[e] = s_rot;
    out[(size_t)m + e] = s_trans;
    out[2 * (size_t)m + e] = rho;
    out[3 * (size_t)m + e] = w;
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

// one wave: lane l adds the partials l, l + 64, ... in order, then the wave's shuffle tree
__global__ __launch_bounds__(64) void k_edge_final(int nb, const double *__restrict__ partials,
                                                   const long long *__restrict__ counts, EdgeSummaryDev *__restrict__ sum) {
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
  if (lane == 0) {
    sum->F_intra = 0.5 * fi;
    sum->F_inter = 0.5 * fe;
    sum->weight_min = wmin;
    sum->num_inter = ni;
    sum->num_downweighted = nd;
  }
}

}  // namespace

int edge_eval_launch(int d, int m, const double *rec, const double *poses, int loss, double loss_reg, double *out,
                     double *partials, long long *counts, EdgeSummaryDev *summary, void *stream) {
  if (m <= 0 || (d != 2 && d != 3) || !rec || !poses || !out || !partials || !counts || !summary) return -1;
  const int nb = (m + EDGE_BLOCK - 1) / EDGE_BLOCK;
  hipStream_t st = (hipStream_t)stream;
  if (d == 2)
    hipLaunchKernelGGL(k_edge_eval<2>, dim3(nb), dim3(EDGE_BLOCK), 0, st, m, (const double2 *)rec, (const double2 *)poses, loss,
                       loss_reg, out, partials, counts);
  else
    hipLaunchKernelGGL(k_edge_eval<3>, dim3(nb), dim3(EDGE_BLOCK), 0, st, m, (const double2 *)rec, (const double2 *)poses, loss,
                       loss_reg, out, partials, counts);
  hipLaunchKernelGGL(k_edge_final, dim3(1), dim3(64), 0, st, nb, partials, counts, summary);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    fprintf(stderr, "[dpgo_amd] ERROR: k_edge_eval launch: %s\n", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

}  // namespace dpgo
