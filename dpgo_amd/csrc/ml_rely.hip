// Kernels of the edge reliability and the candidate gate on the full information matrices for gfx950 (ml_rely.h): the
// covariance of every listed edge's predicted residual, and its record.  fp64, fixed order, no atomics, no LDS.
#include "ml_rely.h"
#include "ml_rely_math.h"

namespace dpgo {
namespace {

// One thread per (edge, entry of rel's lower triangle): a 12 x 12 Sigma_joint beside two Jacobians does not fit one lane's
// registers, and an entry needs nothing of its neighbours.  Entry (a, b), a >= b, is ml_rel_entry's one sum, written to (a, b)
// and (b, a): rel is symmetric bit for bit, and an edge's bits depend on nothing but its own J and joint.  idx (null: the
// identity) names the edge of J that listed edge k is; every offset is 64-bit.
template <int D>
__global__ __launch_bounds__(256) void k_ml_rel(int n, const int *__restrict__ idx, const double *__restrict__ J, long long ldj,
                                                const double *__restrict__ joint, double *__restrict__ rel) {
  constexpr int DOF = cov_dof(D), DD = DOF * DOF, NT = DOF * (DOF + 1) / 2;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)n * NT) return;
  const long long k = t / NT;
  const int e = (int)(t - k * NT);
  int a = 0;
#pragma unroll
  for (int i = 1; i < DOF; i++)
    if (e >= i * (i + 1) / 2) a = i;
  const int b = e - a * (a + 1) / 2;
  const long long src = idx ? (long long)idx[k] : k;
  const double *Jp = J + src * ldj;
  const double v = ml_rel_entry<D>(Jp, Jp + DD, joint + k * 3 * DD, a, b);
  rel[k * DD + a * DOF + b] = v;
  rel[k * DD + b * DOF + a] = v;
}

// One lane per edge: L, A, K and four vectors in registers (ml_rely_math.h); rel, Omega and r are read where they are used.
template <int D, int SIGN>
__global__ __launch_bounds__(64) void k_ml_rely_edge(int n, const int *__restrict__ idx, const double *__restrict__ rel,
                                                     const double *__restrict__ Om, const double *__restrict__ r,
                                                     double *__restrict__ rec) {
  constexpr int DOF = cov_dof(D), DD = DOF * DOF, W = SIGN > 0 ? MlGateDims<D>::WIDTH : RelyDims<D>::WIDTH;
  const long long k = (long long)blockIdx.x * 64 + threadIdx.x;
  if (k >= n) return;
  const long long src = idx ? (long long)idx[k] : k;
  ml_rely_one<D, SIGN>(rel + k * DD, Om + src * DD, r + src * DOF, rec + k * W);
}

}  // namespace

void launch_ml_rel(int d, hipStream_t st, int n, const int *idx, const double *J, long long ldj, const double *joint, double *rel) {
  if (n <= 0) return;
  const int dof = cov_dof(d);
  const long long total = (long long)n * (dof * (dof + 1) / 2);
  const dim3 grid((unsigned)((total + 255) / 256));
  if (d == 3) hipLaunchKernelGGL(k_ml_rel<3>, grid, dim3(256), 0, st, n, idx, J, ldj, joint, rel);
  else hipLaunchKernelGGL(k_ml_rel<2>, grid, dim3(256), 0, st, n, idx, J, ldj, joint, rel);
}

void launch_ml_rely_edge(int d, int sign, hipStream_t st, int n, const int *idx, const double *rel, const double *Om, const double *r,
                         double *rec) {
  if (n <= 0) return;
  const dim3 grid((unsigned)((n + 63) / 64));
  if (d == 3 && sign > 0) hipLaunchKernelGGL((k_ml_rely_edge<3, 1>), grid, dim3(64), 0, st, n, idx, rel, Om, r, rec);
  else if (d == 3) hipLaunchKernelGGL((k_ml_rely_edge<3, -1>), grid, dim3(64), 0, st, n, idx, rel, Om, r, rec);
  else if (sign > 0) hipLaunchKernelGGL((k_ml_rely_edge<2, 1>), grid, dim3(64), 0, st, n, idx, rel, Om, r, rec);
  else hipLaunchKernelGGL((k_ml_rely_edge<2, -1>), grid, dim3(64), 0, st, n, idx, rel, Om, r, rec);
}

}  // namespace dpgo
