// Kernels of the candidate sets for gfx950 (cand.h): the joint innovation covariance block by block, the residuals, the
// quadratic form of the joint test, and the two kernels of a selection step.  fp64, explicit fma, fixed order, no atomics,
// 64-bit offsets.
#include "cand.h"
#include "cand_math.h"

namespace dpgo {
namespace {

constexpr int UPDATE_THREADS = 192;   // a multiple of both dof = 3 and dof = 6: a candidate's rows never straddle two workgroups

// One lane per block (i, j), i >= j, as k_marg_rel (marg.hip): only the blocks of the two Jacobians that are neither zero nor
// the identity are held and the output goes out entry by entry, so no scratch is needed.
template <int D>
__global__ __launch_bounds__(64) void k_cand_innov(int m, int nK, const int *__restrict__ prow, const int *__restrict__ kpos,
                                                   const double *__restrict__ X, const double *__restrict__ sig,
                                                   const double *__restrict__ winv, double *__restrict__ cov, double *__restrict__ S,
                                                   double *__restrict__ S2) {
  typedef PairsDims<D> P;
  const long long e = (long long)blockIdx.x * 64 + threadIdx.x;
  if (e >= (long long)m * m) return;
  const int i = (int)(e / m), j = (int)(e - (long long)i * m);
  if (j > i) return;
  const int kpi = kpos[2 * i], kqi = kpos[2 * i + 1], kpj = kpos[2 * j], kqj = kpos[2 * j + 1];
  cand_innov_block<D>(X + (size_t)prow[kpi] * P::RS, X + (size_t)prow[kqi] * P::RS, X + (size_t)prow[kpj] * P::RS,
                      X + (size_t)prow[kqj] * P::RS, sig, (long long)P::DOF * nK, kpi, kqi, kpj, kqj, i, j, winv + 2 * (size_t)i, cov, S,
                      S2, (long long)P::DOF * m);
}

template <int D>
__global__ __launch_bounds__(64) void k_cand_resid(int m, const int *__restrict__ prow, const int *__restrict__ kpos,
                                                   const double *__restrict__ X, const double *__restrict__ cand,
                                                   double *__restrict__ r, double *__restrict__ winv) {
  typedef PairsDims<D> P;
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= m) return;
  const double *c = cand + (size_t)i * P::CAND;
  double ri[P::DOF], w[2];
  cand_residual<D>(X + (size_t)prow[kpos[2 * i]] * P::RS, X + (size_t)prow[kpos[2 * i + 1]] * P::RS, c, ri);
  cand_omega_inv(c[D * D + D], c[D * D + D + 1], w);
#pragma unroll
  for (int a = 0; a < P::DOF; a++) r[(size_t)i * P::DOF + a] = ri[a];
  winv[2 * (size_t)i] = w[0];
  winv[2 * (size_t)i + 1] = w[1];
}

// one workgroup: thread t takes the rows t, t + 256, ... in ascending order, each row's dot product in ascending columns; then a
// fixed tree over the 256 partial sums (k_marg_logdet's)
__global__ __launch_bounds__(256) void k_cand_quad(int n, const double *__restrict__ Sinv, const double *__restrict__ r,
                                                   double *__restrict__ out) {
  __shared__ double part[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    double row = 0.0;
    for (int j = 0; j < n; j++) row = fma(Sinv[(size_t)i * n + j], r[j], row);
    s = fma(r[i], row, s);
  }
  part[threadIdx.x] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = part[0];
}

template <int D>
__global__ __launch_bounds__(256) void k_cand_select_init(int m, const double *__restrict__ S, const double *__restrict__ r,
                                                          CandSelectBufs b) {
  constexpr int DOF = PairsDims<D>::DOF;
  const long long n = (long long)DOF * m, a = (long long)blockIdx.x * 256 + threadIdx.x;
  if (a == 0) {
    b.state[0] = -1;
    b.state[1] = 0;
    b.state[2] = 0;
    b.sums[0] = 0.0;
    b.sums[1] = 0.0;
  }
  if (a >= n) return;
  const int i = (int)(a / DOF), row = (int)(a - (long long)i * DOF);
#pragma unroll
  for (int c = 0; c < DOF; c++) b.C[a * DOF + c] = S[a * n + (long long)DOF * i + c];
  b.rho[a] = r[a];
  if (row == 0) b.taken[i] = 0;
}

// One workgroup.  Thread t scores the candidates t, t + 256, ... that are not taken; the argmax over the eligible ones is a tree
// over the 256 threads under cand_better's order (larger gain, then lower index), whose winner does not depend on the tree's
// shape.  Thread 0 then writes the step's record, the chosen index and the pivot (L_ss, z_s) that k_cand_update reads.
template <int D>
__global__ __launch_bounds__(256) void k_cand_score(int m, int t, double d2_max, const double *__restrict__ winv, CandSelectBufs b) {
  constexpr int DOF = PairsDims<D>::DOF;
  __shared__ double sg[256], sd[256];
  __shared__ int si[256], sn[256];
  if (b.state[1]) return;   // (uniform: written by thread 0 of an earlier launch only)
  double bg = 0.0, bd = 0.0;
  int bi = -1, cnt = 0;
  for (int i = threadIdx.x; i < m; i += 256) {
    if (b.taken[i]) continue;
    double g, d2;
    const bool pd = cand_score_one<D>(b.C + (size_t)i * DOF * DOF, b.rho + (size_t)i * DOF, winv + 2 * (size_t)i, &g, &d2);
    if (!pd || (d2_max > 0.0 && !(d2 <= d2_max))) continue;
    cnt++;
    if (cand_better(g, i, bg, bi)) {
      bg = g;
      bd = d2;
      bi = i;
    }
  }
  sg[threadIdx.x] = bg;
  sd[threadIdx.x] = bd;
  si[threadIdx.x] = bi;
  sn[threadIdx.x] = cnt;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) {
      const int o = threadIdx.x + h;
      if (cand_better(sg[o], si[o], sg[threadIdx.x], si[threadIdx.x])) {
        sg[threadIdx.x] = sg[o];
        sd[threadIdx.x] = sd[o];
        si[threadIdx.x] = si[o];
      }
      sn[threadIdx.x] += sn[o];
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const int s = si[0];
  b.state[0] = s;
  if (s < 0) {
    b.state[1] = 1;
    return;
  }
  b.state[2] = t + 1;
  b.taken[s] = 1;
  b.selected[t] = s;
  b.steps[4 * (size_t)t] = (double)s;
  b.steps[4 * (size_t)t + 1] = sg[0];
  b.steps[4 * (size_t)t + 2] = sd[0];
  b.steps[4 * (size_t)t + 3] = (double)sn[0];
  b.sums[0] += sg[0];
  b.sums[1] += sd[0];
  double L[DOF * DOF], z[DOF], lg, d2;
  (void)cand_chol<D>(b.C + (size_t)s * DOF * DOF, b.rho + (size_t)s * DOF, L, z, &lg, &d2);   // (positive definite: it was eligible)
#pragma unroll
  for (int a = 0; a < DOF; a++) {
#pragma unroll
    for (int c = 0; c < DOF; c++) b.piv[a * DOF + c] = c <= a ? L[a * DOF + c] : 0.0;
    b.piv[DOF * DOF + a] = z[a];
  }
}

// One thread per row of S.  The row of the new panel streams the earlier panels (rank dof per step: a handful of flops per
// double read, far under the fp64 ridge -- plain fma, no MFMA); the rows of one candidate then meet in LDS for
// C_i -= P_t[i] P_t[i]^T and rho_i -= P_t[i] z_s.  C_i's entries (r, c) and (c, r) are the same chain of fma's with the factors
// swapped: C_i stays symmetric bit for bit.
template <int D>
__global__ __launch_bounds__(UPDATE_THREADS) void k_cand_update(int m, int t, const double *__restrict__ S, CandSelectBufs b) {
  constexpr int DOF = PairsDims<D>::DOF;
  __shared__ double xs[UPDATE_THREADS * DOF];
  const int s = b.state[0];
  if (b.state[1] || s < 0) return;   // (uniform)
  const long long n = (long long)DOF * m, a = (long long)blockIdx.x * UPDATE_THREADS + threadIdx.x;
  double x[DOF];
  if (a < n) {
    cand_panel_row<D>(S, b.P, n, t, s, a, b.piv, x);
#pragma unroll
    for (int c = 0; c < DOF; c++) {
      b.P[((long long)DOF * t + c) * n + a] = x[c];
      xs[threadIdx.x * DOF + c] = x[c];
    }
  }
  __syncthreads();
  if (a >= n) return;
  const int row = (int)(a % DOF), t0 = (int)threadIdx.x - row;
#pragma unroll
  for (int c = 0; c < DOF; c++) {
    double v = b.C[a * DOF + c];
#pragma unroll
    for (int k = 0; k < DOF; k++) v = fma(-x[k], xs[(t0 + c) * DOF + k], v);
    b.C[a * DOF + c] = v;
  }
  double rh = b.rho[a];
#pragma unroll
  for (int k = 0; k < DOF; k++) rh = fma(-x[k], b.piv[DOF * DOF + k], rh);
  b.rho[a] = rh;
}

}  // namespace

void launch_cand_innov(int d, hipStream_t st, int m, int nK, const int *prow, const int *kpos, const double *X, const double *sig,
                       const double *winv, double *cov, double *S, double *S2) {
  const long long total = (long long)m * m;
  if (total <= 0) return;
  const dim3 grid((unsigned)((total + 63) / 64));
  if (d == 3) hipLaunchKernelGGL((k_cand_innov<3>), grid, dim3(64), 0, st, m, nK, prow, kpos, X, sig, winv, cov, S, S2);
  else hipLaunchKernelGGL((k_cand_innov<2>), grid, dim3(64), 0, st, m, nK, prow, kpos, X, sig, winv, cov, S, S2);
}

void launch_cand_resid(int d, hipStream_t st, int m, const int *prow, const int *kpos, const double *X, const double *cand, double *r,
                       double *winv) {
  if (m <= 0) return;
  const dim3 grid((unsigned)((m + 63) / 64));
  if (d == 3) hipLaunchKernelGGL((k_cand_resid<3>), grid, dim3(64), 0, st, m, prow, kpos, X, cand, r, winv);
  else hipLaunchKernelGGL((k_cand_resid<2>), grid, dim3(64), 0, st, m, prow, kpos, X, cand, r, winv);
}

void launch_cand_quad(hipStream_t st, int n, const double *Sinv, const double *r, double *out) {
  hipLaunchKernelGGL(k_cand_quad, dim3(1), dim3(256), 0, st, n, Sinv, r, out);
}

void launch_cand_select_init(int d, hipStream_t st, int m, const double *S, const double *r, CandSelectBufs b) {
  const long long n = (long long)(d == 3 ? 6 : 3) * m;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (d == 3) hipLaunchKernelGGL((k_cand_select_init<3>), grid, dim3(256), 0, st, m, S, r, b);
  else hipLaunchKernelGGL((k_cand_select_init<2>), grid, dim3(256), 0, st, m, S, r, b);
}

void launch_cand_score(int d, hipStream_t st, int m, int t, double d2_max, const double *winv, CandSelectBufs b) {
  if (d == 3) hipLaunchKernelGGL((k_cand_score<3>), dim3(1), dim3(256), 0, st, m, t, d2_max, winv, b);
  else hipLaunchKernelGGL((k_cand_score<2>), dim3(1), dim3(256), 0, st, m, t, d2_max, winv, b);
}

void launch_cand_update(int d, hipStream_t st, int m, int t, const double *S, CandSelectBufs b) {
  const long long n = (long long)(d == 3 ? 6 : 3) * m;
  const dim3 grid((unsigned)((n + UPDATE_THREADS - 1) / UPDATE_THREADS));
  if (d == 3) hipLaunchKernelGGL((k_cand_update<3>), grid, dim3(UPDATE_THREADS), 0, st, m, t, S, b);
  else hipLaunchKernelGGL((k_cand_update<2>), grid, dim3(UPDATE_THREADS), 0, st, m, t, S, b);
}

}  // namespace dpgo
