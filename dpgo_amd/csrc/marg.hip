// Kernels of the joint marginals for gfx950 (marg.h): the gather of Sigma_KK out of a solved batch, the relative covariance
// block by block, the un-permutation of the dense factor's inverse and its log-determinant.  fp64, explicit fma, fixed order,
// no atomics, 64-bit offsets.
#include "marg.h"
#include "marg_math.h"

namespace dpgo {
namespace {

// one thread per entry (i, j) of the ns x ns square; those with i >= j whose column lies in this batch read the solved column j
// at row i and write (i, j) and (j, i) -- an entry of the anchor (row_unk / col_of < 0) keeps the zero the caller wrote
__global__ __launch_bounds__(256) void k_marg_gather(int ns, const int *__restrict__ row_unk, const int *__restrict__ col_of, int c0,
                                                     int nc, const double *__restrict__ Xb, int ldx, double *__restrict__ dst,
                                                     double *__restrict__ dst2) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)ns * ns) return;
  const int i = (int)(e / ns), j = (int)(e - (long long)i * ns);
  if (j > i) return;
  const int cj = col_of[j], ri = row_unk[i];
  if (cj < 0 || ri < 0) return;
  const int col = cj - c0;
  if (col < 0 || col >= nc) return;
  const double v = Xb[(size_t)ri * ldx + col];
  const long long lo = (long long)i * ns + j, up = (long long)j * ns + i;
  dst[lo] = v;
  dst[up] = v;
  if (dst2) {
    dst2[lo] = v;
    dst2[up] = v;
  }
}

// One lane per block (ko, lo), ko >= lo, of the relative covariance.  k_pairs_gate (pairs.hip) keeps a dense J and fills the
// register file for D = 3; here only the blocks of J that are neither zero nor the identity are held (marg_math.h: 2 x 27
// doubles for D = 3) and the output goes out entry by entry, so no scratch is needed.
template <int D>
__global__ __launch_bounds__(64) void k_marg_rel(int K, int b, const int *__restrict__ prow, const double *__restrict__ X,
                                                 const double *__restrict__ sig, double *__restrict__ C, double *__restrict__ C2) {
  typedef PairsDims<D> P;
  const int m = K - 1;
  const long long e = (long long)blockIdx.x * 64 + threadIdx.x;
  if (e >= (long long)m * m) return;
  const int ko = (int)(e / m), lo = (int)(e - (long long)ko * m);
  if (lo > ko) return;
  const int k = ko + (ko >= b ? 1 : 0), l = lo + (lo >= b ? 1 : 0);
  marg_rel_block<D>(X + (size_t)prow[b] * P::RS, X + (size_t)prow[k] * P::RS, X + (size_t)prow[l] * P::RS, sig,
                    (long long)P::DOF * K, b, k, l, ko, lo, C, C2, (long long)P::DOF * m);
}

__global__ __launch_bounds__(256) void k_marg_scatter(int n, const int *__restrict__ piv, const double *__restrict__ S,
                                                      double *__restrict__ info) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)n * n) return;
  const int a = (int)(e / n), c = (int)(e - (long long)a * n);
  info[(long long)piv[a] * n + piv[c]] = S[e];
}

// one workgroup: thread t sums log W_ii over i = t, t + 256, ... in ascending order, then a fixed tree over the 256 partial sums
__global__ __launch_bounds__(256) void k_marg_logdet(int n, const double *__restrict__ W, int ldw, double *__restrict__ out) {
  __shared__ double part[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += log(W[(size_t)i * ldw + i]);
  part[threadIdx.x] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = -2.0 * part[0];
}

}  // namespace

void launch_marg_gather(hipStream_t st, int ns, const int *row_unk, const int *col_of, int c0, int nc, const double *Xb, int ldx,
                        double *dst, double *dst2) {
  const long long total = (long long)ns * ns;
  if (total > 0 && nc > 0)
    hipLaunchKernelGGL(k_marg_gather, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, ns, row_unk, col_of, c0, nc, Xb, ldx, dst, dst2);
}

void launch_marg_rel(int d, hipStream_t st, int K, int b, const int *prow, const double *X, const double *sig, double *C, double *C2) {
  const long long total = (long long)(K - 1) * (K - 1);
  if (total <= 0) return;
  const dim3 grid((unsigned)((total + 63) / 64));
  if (d == 3) hipLaunchKernelGGL((k_marg_rel<3>), grid, dim3(64), 0, st, K, b, prow, X, sig, C, C2);
  else hipLaunchKernelGGL((k_marg_rel<2>), grid, dim3(64), 0, st, K, b, prow, X, sig, C, C2);
}

void launch_marg_scatter(hipStream_t st, int n, const int *piv, const double *S, double *info) {
  const long long total = (long long)n * n;
  if (total > 0) hipLaunchKernelGGL(k_marg_scatter, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, n, piv, S, info);
}

void launch_marg_logdet(hipStream_t st, int n, const double *W, int ldw, double *out) {
  hipLaunchKernelGGL(k_marg_logdet, dim3(1), dim3(256), 0, st, n, W, ldw, out);
}

}  // namespace dpgo
