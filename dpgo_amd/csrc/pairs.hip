// Kernels of the joint pair covariances for gfx950 (pairs.h): the unit right-hand sides of a batch, the gather of the blocks out
// of the solved batch, and the relative covariance and gate of every pair.  fp64, fixed order, no atomics.
#include "pairs.h"
#include "pairs_math.h"

namespace dpgo {
namespace {

__global__ __launch_bounds__(64) void k_pairs_rhs(const int *__restrict__ col_unknown, int c0, int nc, double *__restrict__ Xb, int ldx) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j < nc) Xb[(size_t)col_unknown[c0 + j] * ldx + j] = 1.0;
}

// one thread per entry of the 3 dof^2 doubles of a pair: block 0 = S_pp (row of p, column of p), 1 = S_pq (row of p, column of
// q), 2 = S_qq; an entry whose column is not in this batch is left for the batch that holds it
__global__ __launch_bounds__(256) void k_pairs_gather(int dof, int npairs, const int *__restrict__ prow, const int *__restrict__ pcol,
                                                      int c0, int nc, const double *__restrict__ Xb, int ldx, double *__restrict__ joint) {
  const int DD = dof * dof;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)npairs * 3 * DD) return;
  const int k = (int)(e / (3 * DD)), rem = (int)(e - (long long)k * 3 * DD), blk = rem / DD, a = (rem % DD) / dof, b = rem % dof;
  const int cp = pcol[2 * k], cq = pcol[2 * k + 1];
  if ((blk != 2 && cp < 0) || (blk != 0 && cq < 0)) return;   // (the anchor: the zeros the caller wrote)
  const int col = (blk == 0 ? cp : cq) + b - c0;
  if (col < 0 || col >= nc) return;
  const int row = dof * prow[2 * k + (blk == 2 ? 1 : 0)] + a;
  joint[e] = Xb[(size_t)row * ldx + col];
}

// One lane per pair keeps J (dof x 2 dof), a row of J Sigma and the dof x dof factor in registers: for D = 3 that is the whole
// register file of a wave (256 VGPRs, the rest parked in AGPRs, no scratch), which a launch of one wave per 64 pairs can
// afford.  A formulation on J's sparsity (J_q is [[Y_p, 0], [0, I]]) would be leaner, should a compiler ever spill this one.
template <int D>
__global__ __launch_bounds__(64) void k_pairs_gate(int npairs, const int *__restrict__ prow, const double *__restrict__ joint,
                                                   const double *__restrict__ X, const double *__restrict__ cand,
                                                   double *__restrict__ rel, double *__restrict__ gate) {
  typedef PairsDims<D> P;
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= npairs) return;
  const double *S = joint + (size_t)k * 3 * P::DD;
  pairs_one<D>(X + (size_t)prow[2 * k] * P::RS, X + (size_t)prow[2 * k + 1] * P::RS, S, S + P::DD, S + 2 * P::DD,
               cand ? cand + (size_t)k * P::CAND : nullptr, rel + (size_t)k * P::DD, gate ? gate + (size_t)k * (2 + P::DOF) : nullptr);
}

}  // namespace

void launch_pairs_rhs(hipStream_t st, const int *col_unknown, int c0, int nc, double *Xb, int ldx) {
  if (nc > 0) hipLaunchKernelGGL(k_pairs_rhs, dim3((nc + 63) / 64), dim3(64), 0, st, col_unknown, c0, nc, Xb, ldx);
}

void launch_pairs_gather(hipStream_t st, int dof, int npairs, const int *prow, const int *pcol, int c0, int nc, const double *Xb,
                         int ldx, double *joint) {
  const long long total = (long long)npairs * 3 * dof * dof;
  if (total > 0)
    hipLaunchKernelGGL(k_pairs_gather, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, dof, npairs, prow, pcol, c0, nc, Xb, ldx, joint);
}

void launch_pairs_gate(int d, hipStream_t st, int npairs, const int *prow, const double *joint, const double *X, const double *cand,
                       double *rel, double *gate) {
  if (npairs == 0) return;
  if (d == 3)
    hipLaunchKernelGGL((k_pairs_gate<3>), dim3((npairs + 63) / 64), dim3(64), 0, st, npairs, prow, joint, X, cand, rel, gate);
  else
    hipLaunchKernelGGL((k_pairs_gate<2>), dim3((npairs + 63) / 64), dim3(64), 0, st, npairs, prow, joint, X, cand, rel, gate);
}

}  // namespace dpgo
