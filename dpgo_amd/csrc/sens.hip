// Kernels of the measurement sensitivities for gfx950 (sens.h): the upstream columns of a batch as right-hand sides, the
// adjoint's read-out, and the per-edge mixed derivative of every (edge, column).  fp64, fixed order, no atomics.
#include "sens.h"
#include "sens_math.h"

namespace dpgo {
namespace {

// one thread per (unknown by global pose, column), the column fastest: the writes of a wave are one run of a row of Xb
__global__ __launch_bounds__(256) void k_sens_rhs(int dof, long long n, const int *__restrict__ row_of, int anchor,
                                                  const double *__restrict__ U, int nc, double *__restrict__ Xb, int ldx) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * nc) return;
  const long long u = idx / nc;
  const int j = (int)(idx - u * nc), p = (int)(u / dof), a = (int)(u - (long long)p * dof);
  if (p == anchor) return;
  Xb[((size_t)dof * row_of[p] + a) * ldx + j] = U[(size_t)j * n + u];
}

// one thread per (unknown by unified own row, column), the column fastest
__global__ __launch_bounds__(256) void k_sens_adjoint(int dof, long long n, const int *__restrict__ gid, int anchor,
                                                      const double *__restrict__ Xb, int ldx, int nc, double *__restrict__ A) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * nc) return;
  const long long u = idx / nc;
  const int j = (int)(idx - u * nc), row = (int)(u / dof), a = (int)(u - (long long)row * dof), p = gid[row];
  A[(size_t)j * n + (size_t)dof * p + a] = p == anchor ? 0.0 : Xb[(size_t)u * ldx + j];
}

// One thread per (edge, column of the batch), the column fastest: with ldx = 64 a wave is one edge, its record and its two
// pose records are wave-uniform, and every coordinate of lambda is one run of consecutive doubles of a row of Xb.  The
// arithmetic of a thread is sens_one on its own column's numbers and nothing else.
template <int D>
__global__ __launch_bounds__(256) void k_sens_edge(int m, const double *__restrict__ rec, const double *__restrict__ X,
                                                   const double *__restrict__ Xb, int ldx, int nc, double *__restrict__ out) {
  constexpr int DOF = D + D * (D - 1) / 2, L = 4 + D * D + D, RS = (D + 1) * D, NO = 2 + DOF;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const int e = (int)(idx / ldx), j = (int)(idx - (long long)e * ldx);
  if (e >= m || j >= nc) return;
  const double *q = rec + (size_t)e * L;
  int i, jj;
  bool inter;
  edge_head(q, i, jj, inter);
  double li[DOF], lj[DOF], v[NO];
#pragma unroll
  for (int a = 0; a < DOF; a++) {
    li[a] = Xb[((size_t)DOF * i + a) * ldx + j];
    lj[a] = Xb[((size_t)DOF * jj + a) * ldx + j];
  }
  sens_one<D>(q, X + (size_t)i * RS, X + (size_t)jj * RS, li, lj, v, nullptr);
  double *o = out + ((size_t)j * m + e) * NO;
#pragma unroll
  for (int a = 0; a < NO; a++) o[a] = v[a];
}

unsigned blocks_of(long long total) { return (unsigned)((total + 255) / 256); }

}  // namespace

void launch_sens_rhs(hipStream_t st, int dof, int nposes, const int *row_of, int anchor, const double *U, int nc, double *Xb, int ldx) {
  const long long n = (long long)dof * nposes;
  if (n * nc > 0) hipLaunchKernelGGL(k_sens_rhs, dim3(blocks_of(n * nc)), dim3(256), 0, st, dof, n, row_of, anchor, U, nc, Xb, ldx);
}

void launch_sens_adjoint(hipStream_t st, int dof, int nposes, const int *gid, int anchor, const double *Xb, int ldx, int nc, double *A) {
  const long long n = (long long)dof * nposes;
  if (n * nc > 0) hipLaunchKernelGGL(k_sens_adjoint, dim3(blocks_of(n * nc)), dim3(256), 0, st, dof, n, gid, anchor, Xb, ldx, nc, A);
}

void launch_sens_edge(int d, hipStream_t st, int m, const double *rec, const double *X, const double *Xb, int ldx, int nc, double *out) {
  const long long total = (long long)m * ldx;
  if (total <= 0 || nc <= 0) return;
  if (d == 3)
    hipLaunchKernelGGL((k_sens_edge<3>), dim3(blocks_of(total)), dim3(256), 0, st, m, rec, X, Xb, ldx, nc, out);
  else
    hipLaunchKernelGGL((k_sens_edge<2>), dim3(blocks_of(total)), dim3(256), 0, st, m, rec, X, Xb, ldx, nc, out);
}

}  // namespace dpgo
