// The Riemannian Hessian in tangent coordinates for gfx950 (cov.h), written where the factorisation reads it.
//
// One wave per pose p, its lanes striding the pose's run of output values (nb_p blocks of dof x dof): an entry is a sum
// of at most 4 d products of entries of S_pq (read from M's values in the certificate's order, Lambda_p subtracted on the
// rotation part of the diagonal block) with entries of Y_p and Y_q (read from the pose records).  fp64, plain FMAs in a
// fixed order, no atomics: the same bits run to run.
#include "cov.h"

namespace dpgo {
namespace {

template <int D>
__global__ __launch_bounds__(256) void k_cov_hessian(int nposes, const int *__restrict__ bptr, const int *__restrict__ bcol,
                                                     const double *__restrict__ Mval, const double *__restrict__ Lam,
                                                     const double *__restrict__ X, int anchor, double *__restrict__ out) {
  constexpr int B = D + 1, RS = B * D, DOF = D + D * (D - 1) / 2;
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= nposes) return;
  const int b0 = bptr[p], nb = bptr[p + 1] - b0, rowlen = DOF * nb, len = DOF * rowlen;
  const size_t base_in = (size_t)B * B * b0, base_out = (size_t)DOF * DOF * b0;
  const double *Yp = X + (size_t)p * RS + D;
  for (int l = lane; l < len; l += 64) {
    const int a = l / rowlen, rem = l - a * rowlen, j = rem / DOF, b = rem - j * DOF;
    const int q = bcol[b0 + j];
    if (p == anchor || q == anchor) {   // the gauge: the anchor's row and column are those of the identity
      out[base_out + l] = (p == q && a == b) ? 1.0 : 0.0;
      continue;
    }
    const double *Yq = X + (size_t)q * RS + D;
    // S_pq[r][c]
    auto S = [&](int r, int c) -> double {
      double v = Mval[base_in + (size_t)r * B * nb + (size_t)j * B + c];
      if (p == q && r >= 1 && c >= 1) v -= Lam[(size_t)p * D * D + (r - 1) * D + (c - 1)];
      return v;
    };
    double h;
    if (a < D && b < D) {
      h = a == b ? S(0, 0) : 0.0;
    } else if (a < D) {                 // translation a, rotation b - D of q:  sum_r S[0, 1 + r] B_l(q)[r, a]
      int s1, s2;
      cov_rot_rows<D>(b - D, s1, s2);
      h = fma(S(0, 1 + s1), Yq[s2 * D + a], -(S(0, 1 + s2) * Yq[s1 * D + a]));
    } else if (b < D) {                 // rotation a - D of p, translation b:  sum_r B_k(p)[r, b] S[1 + r, 0]
      int r1, r2;
      cov_rot_rows<D>(a - D, r1, r2);
      h = fma(Yp[r2 * D + b], S(1 + r1, 0), -(Yp[r1 * D + b] * S(1 + r2, 0)));
    } else {                            // tr(B_k(p)^T S[1:, 1:] B_l(q))
      int r1, r2, s1, s2;
      cov_rot_rows<D>(a - D, r1, r2);
      cov_rot_rows<D>(b - D, s1, s2);
      const double S11 = S(1 + r1, 1 + s1), S12 = S(1 + r1, 1 + s2), S21 = S(1 + r2, 1 + s1), S22 = S(1 + r2, 1 + s2);
      h = 0.0;
#pragma unroll
      for (int c = 0; c < D; c++) {
        const double bp1 = Yp[r2 * D + c], bp2 = -Yp[r1 * D + c], bq1 = Yq[s2 * D + c], bq2 = -Yq[s1 * D + c];
        h = fma(bp1, fma(S11, bq1, S12 * bq2), h);
        h = fma(bp2, fma(S21, bq1, S22 * bq2), h);
      }
    }
    out[base_out + l] = h;
  }
}

}  // namespace

void launch_cov_hessian(int d, hipStream_t st, int nposes, const int *bptr, const int *bcol, const double *Mval, const double *Lam,
                        const double *X, int anchor, double *out) {
  if (nposes == 0) return;
  if (d == 3)
    hipLaunchKernelGGL((k_cov_hessian<3>), dim3((nposes + 3) / 4), dim3(256), 0, st, nposes, bptr, bcol, Mval, Lam, X, anchor, out);
  else
    hipLaunchKernelGGL((k_cov_hessian<2>), dim3((nposes + 3) / 4), dim3(256), 0, st, nposes, bptr, bcol, Mval, Lam, X, anchor, out);
}

}  // namespace dpgo
