// Kernels of the sensitivities of the robust objective for gfx950 (rsens.h): the per-edge preparation pass and the per-edge
// mixed derivative of every (edge, column).  fp64, fixed order, no atomics, no LDS.  The right-hand sides and the adjoint's
// read-out are sens.hip's.
#include "rsens.h"

#include "edges.h"
#include "rsens_math.h"
#include "sens_math.h"

namespace dpgo {
namespace {

// One lane per edge in graph order, 64 per workgroup: what k_rsens_edge needs of an edge and every column shares.
template <int D>
__global__ __launch_bounds__(EDGE_BLOCK) void k_rsens_prep(int m, const double *__restrict__ rec, const double *__restrict__ X,
                                                           const double *__restrict__ eo, int loss, double dl,
                                                           double *__restrict__ prep) {
  constexpr int DOF = D + D * (D - 1) / 2, L = edge_rec_doubles(D), RS = pose_rec_doubles(D), NO = 2 + DOF;
  const int e = blockIdx.x * EDGE_BLOCK + threadIdx.x;
  if (e >= m) return;
  double q[L], a[RS], b[RS];
#pragma unroll
  for (int k = 0; k < L; k++) q[k] = rec[(size_t)e * L + k];
  int i, j;
  bool inter;
  edge_head(q, i, j, inter);
#pragma unroll
  for (int k = 0; k < RS; k++) {
    a[k] = X[(size_t)i * RS + k];
    b[k] = X[(size_t)j * RS + k];
  }
  double v[NO + 1];
  rsens_ds<D>(q, a, b, v);
  const double s = eo[e] + eo[(size_t)m + e];   // k_robust_edge's s: the sum of the two rounded parts
  v[NO] = rsens_dw(loss, dl, s, eo[3 * (size_t)m + e], inter);
  double *o = prep + (size_t)e * (NO + 1);
#pragma unroll
  for (int k = 0; k < NO + 1; k++) o[k] = v[k];
}

// One thread per (edge, column of the batch), the column fastest, as k_sens_edge: with ldx = 64 a wave is one edge, and the
// edge's record, pose records, w, c and preparation are the same addresses for the whole wave.  The arithmetic of a thread
// is sens_one and rsens_combine on its own column's numbers and nothing else.
template <int D>
__global__ __launch_bounds__(256) void k_rsens_edge(int m, const double *__restrict__ rec, const double *__restrict__ X,
                                                    const double *__restrict__ eo, const double *__restrict__ prep,
                                                    const double *__restrict__ Xb, int ldx, int nc, double *__restrict__ out) {
  constexpr int DOF = D + D * (D - 1) / 2, L = edge_rec_doubles(D), RS = pose_rec_doubles(D), NO = 2 + DOF;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const int e = (int)(idx / ldx), j = (int)(idx - (long long)e * ldx);
  if (e >= m || j >= nc) return;
  const double *q = rec + (size_t)e * L;
  int i, jj;
  bool inter;
  edge_head(q, i, jj, inter);
  double li[DOF], lj[DOF], v[NO], phi;
#pragma unroll
  for (int a = 0; a < DOF; a++) {
    li[a] = Xb[((size_t)DOF * i + a) * ldx + j];
    lj[a] = Xb[((size_t)DOF * jj + a) * ldx + j];
  }
  sens_one<D>(q, X + (size_t)i * RS, X + (size_t)jj * RS, li, lj, v, &phi);
  const double *pe = prep + (size_t)e * (NO + 1);
  double r[NO + 1];
  rsens_combine<D>(eo[3 * (size_t)m + e], eo[4 * (size_t)m + e], phi, pe, pe[NO], v, r);
  double *o = out + ((size_t)j * m + e) * (NO + 1);
#pragma unroll
  for (int a = 0; a < NO + 1; a++) o[a] = r[a];
}

unsigned blocks_of(long long total, int per) { return (unsigned)((total + per - 1) / per); }

}  // namespace

void launch_rsens_prep(int d, hipStream_t st, int m, const double *rec, const double *X, const double *eo, int loss, double loss_reg,
                       double *prep) {
  if (m <= 0) return;
  if (d == 3)
    hipLaunchKernelGGL((k_rsens_prep<3>), dim3(blocks_of(m, EDGE_BLOCK)), dim3(EDGE_BLOCK), 0, st, m, rec, X, eo, loss, loss_reg, prep);
  else
    hipLaunchKernelGGL((k_rsens_prep<2>), dim3(blocks_of(m, EDGE_BLOCK)), dim3(EDGE_BLOCK), 0, st, m, rec, X, eo, loss, loss_reg, prep);
}

void launch_rsens_edge(int d, hipStream_t st, int m, const double *rec, const double *X, const double *eo, const double *prep,
                       const double *Xb, int ldx, int nc, double *out) {
  const long long total = (long long)m * ldx;
  if (total <= 0 || nc <= 0) return;
  if (d == 3)
    hipLaunchKernelGGL((k_rsens_edge<3>), dim3(blocks_of(total, 256)), dim3(256), 0, st, m, rec, X, eo, prep, Xb, ldx, nc, out);
  else
    hipLaunchKernelGGL((k_rsens_edge<2>), dim3(blocks_of(total, 256)), dim3(256), 0, st, m, rec, X, eo, prep, Xb, ldx, nc, out);
}

}  // namespace dpgo
