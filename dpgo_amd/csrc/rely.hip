// Kernels of the per-edge reliability for gfx950 (rely.h): the gather of every listed edge's three blocks out of the selected
// inversion, and the record of every edge.  fp64, fixed order, no atomics.
#include "rely.h"
#include "rely_math.h"

namespace dpgo {
namespace {

// one thread per entry of the 3 dof^2 doubles of an edge, pairs.h's layout: block 0 = S_pp, 1 = S_pq (rows of p, columns of q),
// 2 = S_qq.  Every S_front is symmetric bit for bit, so S_pq[a][b] is read at (p's a, q's b) of the front that holds both,
// whichever of the two it eliminates.  A block that involves the anchor (off < 0) is zero.  Offsets are 64-bit.
__global__ __launch_bounds__(256) void k_rely_gather(int dof, int nedges, const int64_t *__restrict__ off, const int *__restrict__ loc,
                                                     const double *__restrict__ Sig, double *__restrict__ joint) {
  const int DD = dof * dof, NL = rely_map_ints(dof);
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)nedges * 3 * DD) return;
  const int k = (int)(e / (3 * DD)), rem = (int)(e - (long long)k * 3 * DD), blk = rem / DD, a = (rem % DD) / dof, b = rem % dof;
  const int64_t o = off[(size_t)3 * k + blk];
  double v = 0.0;
  if (o >= 0) {
    const int *l = loc + (size_t)k * NL;
    const int m = l[blk];
    const int *rows = l + 3 + (blk == 0 ? 0 : blk == 1 ? 2 * dof : dof), *cols = l + 3 + (blk == 0 ? 0 : blk == 1 ? 3 * dof : dof);
    v = Sig[o + (int64_t)rows[a] * m + cols[b]];
  }
  joint[e] = v;
}

// One lane per edge: the dof x dof factor and two vectors in registers (rely_math.h); rel is read where it is used.
template <int D>
__global__ __launch_bounds__(64) void k_rely_edge(int nedges, const double *__restrict__ rel, const double *__restrict__ r, int ldr,
                                                  const double *__restrict__ kt, int ldkt, double *__restrict__ rec) {
  typedef RelyDims<D> Q;
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= nedges) return;
  double rl[Q::DOF * Q::DOF], rr[Q::DOF], out[Q::WIDTH];
#pragma unroll
  for (int i = 0; i < Q::DOF * Q::DOF; i++) rl[i] = rel[(size_t)k * Q::DOF * Q::DOF + i];
#pragma unroll
  for (int i = 0; i < Q::DOF; i++) rr[i] = r[(size_t)k * ldr + i];
  rely_one<D>(rl, rr, kt[(size_t)k * ldkt], kt[(size_t)k * ldkt + 1], out);
#pragma unroll
  for (int i = 0; i < Q::WIDTH; i++) rec[(size_t)k * Q::WIDTH + i] = out[i];
}

}  // namespace

void launch_rely_gather(hipStream_t st, int dof, int nedges, const int64_t *off, const int *loc, const double *Sig, double *joint) {
  const long long total = (long long)nedges * 3 * dof * dof;
  if (total > 0)
    hipLaunchKernelGGL(k_rely_gather, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, dof, nedges, off, loc, Sig, joint);
}

void launch_rely_edge(int d, hipStream_t st, int nedges, const double *rel, const double *r, int ldr, const double *kt, int ldkt,
                      double *rec) {
  if (nedges == 0) return;
  if (d == 3)
    hipLaunchKernelGGL((k_rely_edge<3>), dim3((nedges + 63) / 64), dim3(64), 0, st, nedges, rel, r, ldr, kt, ldkt, rec);
  else
    hipLaunchKernelGGL((k_rely_edge<2>), dim3((nedges + 63) / 64), dim3(64), 0, st, nedges, rel, r, ldr, kt, ldkt, rec);
}

}  // namespace dpgo
