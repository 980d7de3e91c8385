// Certificate-matrix kernels for gfx950 (cert.h): the row-local passes of the LOBPCG search on S = M - Lambda(X)
// (C++/SESync/src/SESyncProblem.cpp:375-395, :444-447; C++/Optimization/include/Optimization/LinearAlgebra/LOBPCG.h:131-337).
//
// One wave per own segment of the group's SegTable, lane = pose, records moved as 16-byte loads and stores.  fp64
// throughout, no fast-math.  Every sum is a fixed tree -- lanes of a wave, then the segments in order (k_cert_reduce):
// the same bits run to run, no floating-point atomics.  The products with M themselves are k_bsr's (kernels.hip).
#include "cert.h"

#include <cstdio>

#include "wave_reduce.h"

namespace dpgo {
namespace {

template <int N>
__device__ __forceinline__ void load_rec(const double *p, double (&r)[N]) {
  static_assert(N % 2 == 0, "records are multiples of 16 bytes");
  const double2 *q = reinterpret_cast<const double2 *>(p);
#pragma unroll
  for (int k = 0; k < N / 2; k++) {
    const double2 v = q[k];
    r[2 * k] = v.x;
    r[2 * k + 1] = v.y;
  }
}
template <int N>
__device__ __forceinline__ void store_rec(double *p, const double (&r)[N]) {
  static_assert(N % 2 == 0, "records are multiples of 16 bytes");
  double2 *q = reinterpret_cast<double2 *>(p);
#pragma unroll
  for (int k = 0; k < N / 2; k++) q[k] = make_double2(r[2 * k], r[2 * k + 1]);
}
__device__ __forceinline__ bool node_on(const NodeMask &m, int node) { return ((m.p ? (m.v & *m.p) : m.v) >> node) & 1ull; }

// Sums of N = 3 * 2^k values per lane over the 64 lanes of a wave with N + O(1) shuffles instead of 6 N: while the count
// is even, the lanes of a pair (l, l ^ OFF) split it -- the lower lane keeps the first half of the sums, the upper lane
// the second, each adds what the other held of its half -- and once three are left the remaining strides add in full.
// Afterwards the lanes with (lane & dup) == 0 hold the complete sums base .. base + 2.  A fixed tree.
template <int N, int OFF>
__device__ __forceinline__ void reduce_scatter(double *v, int lane, int &base, int &dup) {
  if constexpr (OFF >= 1) {
    if constexpr (N % 2 == 0) {
      const bool up = (lane & OFF) != 0;
#pragma unroll
      for (int i = 0; i < N / 2; i++) {
        const double keep = up ? v[i + N / 2] : v[i], send = up ? v[i] : v[i + N / 2];
        v[i] = keep + __shfl_xor(send, OFF, 64);
      }
      base += up ? N / 2 : 0;
      reduce_scatter<N / 2, OFF / 2>(v, lane, base, dup);
    } else {
#pragma unroll
      for (int i = 0; i < N; i++) v[i] += __shfl_xor(v[i], OFF, 64);
      dup |= OFF;
      reduce_scatter<N, OFF / 2>(v, lane, base, dup);
    }
  }
}
// the NS sums (padded to NP = 3 * 2^k) of a wave to dst[s * stride]
template <int NS, int NP>
__device__ __forceinline__ void wave_store_sums(double (&v)[NP], double *dst, int stride) {
  static_assert(NP >= NS && (NP == 48 || NP == 24), "3 * 2^k");
  const int lane = threadIdx.x & 63;
  int base = 0, dup = 0;
  reduce_scatter<NP, 32>(v, lane, base, dup);
  if ((lane & dup) == 0) {
#pragma unroll
    for (int i = 0; i < 3; i++)
      if (base + i < NS) dst[(size_t)(base + i) * stride] = v[i];
  }
}

// Lambda_p = 1/2 (P + P^T), P = (M X).Y (X.Y)^T   (SESyncProblem.cpp:375-395); L: d x d row-major
template <int D>
__device__ __forceinline__ void lambda_block(const double *x, const double *mx, double *L) {
  double P[D * D];
#pragma unroll
  for (int r = 0; r < D; r++)
#pragma unroll
    for (int s = 0; s < D; s++) {
      double a = 0;
#pragma unroll
      for (int c = 0; c < D; c++) a = fma(mx[D + r * D + c], x[D + s * D + c], a);
      P[r * D + s] = a;
    }
#pragma unroll
  for (int r = 0; r < D; r++)
#pragma unroll
    for (int s = 0; s < D; s++) L[r * D + s] = 0.5 * (P[r * D + s] + P[s * D + r]);
}
// out.Y = mv.Y - L v.Y (rotation rows); out.x = mv.x.  The d products are summed first and subtracted once: the error is
// d u |L| |v| + u |out|.  Subtracting them from mv one fma at a time rounds every partial result, d u |out| + 2 (d - 1) u |L| |v|,
// which is up to d times more where |mv| is large against |L| |v| (tests/test_gpu_cert_search.py: test_gram_finishes_S_W).
template <int D>
__device__ __forceinline__ void sub_lambda(const double *L, const double *v, const double *mv, double *out) {
#pragma unroll
  for (int c = 0; c < D; c++) out[c] = mv[c];
#pragma unroll
  for (int r = 0; r < D; r++)
#pragma unroll
    for (int c = 0; c < D; c++) {
      double t = L[r * D] * v[D + c];
#pragma unroll
      for (int k = 1; k < D; k++) t = fma(L[r * D + k], v[D + k * D + c], t);
      out[D + r * D + c] = mv[D + r * D + c] - t;
    }
}

template <int D>
__global__ __launch_bounds__(SEG_ROWS) void k_cert_lambda(const Seg *segs, NodeMask mask, const double *__restrict__ X,
                                                          const double *__restrict__ MX, double *__restrict__ Lam,
                                                          double *__restrict__ SX, double *partial, int nseg) {
  constexpr int RS = (D + 1) * D;
  const Seg s = segs[blockIdx.x];
  if (!node_on(mask, s.node)) return;
  const int row = s.begin + threadIdx.x;
  double p = 0;
  if (row < s.end) {
    double x[RS], mx[RS], sx[RS], L[D * D];
    load_rec<RS>(X + (size_t)row * RS, x);
    load_rec<RS>(MX + (size_t)row * RS, mx);
    lambda_block<D>(x, mx, L);
#pragma unroll
    for (int k = 0; k < D * D; k++) Lam[(size_t)row * D * D + k] = L[k];
    sub_lambda<D>(L, x, mx, sx);
    if (SX) store_rec<RS>(SX + (size_t)row * RS, sx);
#pragma unroll
    for (int k = 0; k < RS; k++) p = fma(sx[k], sx[k], p);
  }
  p = wave_sum(p);
  if (threadIdx.x == 0) partial[blockIdx.x] = p;
  (void)nseg;
}

template <int D>
__global__ __launch_bounds__(SEG_ROWS) void k_cert_apply(const Seg *segs, NodeMask mask, const double *__restrict__ Lam,
                                                         const double *__restrict__ V, const double *MV, double *out) {
  constexpr int RS = (D + 1) * D;
  const Seg s = segs[blockIdx.x];
  if (!node_on(mask, s.node)) return;
  const int row = s.begin + threadIdx.x;
  if (row >= s.end) return;
  double v[RS], mv[RS], o[RS], L[D * D];
  load_rec<RS>(V + (size_t)row * RS, v);
  load_rec<RS>(MV + (size_t)row * RS, mv);
#pragma unroll
  for (int k = 0; k < D * D; k++) L[k] = Lam[(size_t)row * D * D + k];
  sub_lambda<D>(L, v, mv, o);
  store_rec<RS>(out + (size_t)row * RS, o);
}

// entry (r, blk * D + j) of the basis [V W P] of one pose
#define CERT_B(arr, r, a) arr[(a) / D][(r) * D + (a) % D]

template <int D>
__global__ __launch_bounds__(SEG_ROWS) void k_cert_gram(const Seg *segs, NodeMask mask, const double *__restrict__ Lam,
                                                        const double *__restrict__ V, const double *__restrict__ W,
                                                        const double *__restrict__ P, const double *__restrict__ SV, double *SW,
                                                        const double *__restrict__ SP, double *partial, int nseg) {
  constexpr int RS = (D + 1) * D, N3 = 3 * D, NT = cert_ntri(D), NP = D == 3 ? 48 : 24;
  const Seg s = segs[blockIdx.x];
  if (!node_on(mask, s.node)) return;   // (uniform over the workgroup)
  const int row = s.begin + threadIdx.x;
  const bool live = row < s.end;
  const size_t off = (size_t)(live ? row : s.begin) * RS;
  double b[3][RS];
  load_rec<RS>(V + off, b[0]);
  load_rec<RS>(W + off, b[1]);
  load_rec<RS>(P + off, b[2]);
  if (!live) {
#pragma unroll
    for (int q = 0; q < 3; q++)
#pragma unroll
      for (int k = 0; k < RS; k++) b[q][k] = 0.0;
  }
  double g[NP];
#pragma unroll
  for (int k = NT; k < NP; k++) g[k] = 0.0;
  // B^T B
#pragma unroll
  for (int a = 0; a < N3; a++)
#pragma unroll
    for (int c = a; c < N3; c++) {
      double t = 0;
#pragma unroll
      for (int r = 0; r <= D; r++) t = fma(CERT_B(b, r, a), CERT_B(b, r, c), t);
      g[cert_tri(N3, a, c)] = t;
    }
  wave_store_sums<NT, NP>(g, partial + blockIdx.x, nseg);
  // S W = M W - [0 ; Lambda W.Y], then B^T (S B)
  double sb[3][RS];
  load_rec<RS>(SV + off, sb[0]);
  load_rec<RS>(SP + off, sb[2]);
  {
    double mw[RS], L[D * D];
    load_rec<RS>(SW + off, mw);
#pragma unroll
    for (int k = 0; k < D * D; k++) L[k] = Lam[(size_t)(live ? row : s.begin) * D * D + k];
    sub_lambda<D>(L, b[1], mw, sb[1]);
    if (live) store_rec<RS>(SW + off, sb[1]);
  }
#pragma unroll
  for (int k = NT; k < NP; k++) g[k] = 0.0;
#pragma unroll
  for (int a = 0; a < N3; a++)
#pragma unroll
    for (int c = a; c < N3; c++) {
      double t = 0;
#pragma unroll
      for (int r = 0; r <= D; r++) t = fma(CERT_B(b, r, a), CERT_B(sb, r, c), t);
      g[cert_tri(N3, a, c)] = t;
    }
  wave_store_sums<NT, NP>(g, partial + (size_t)NT * nseg + blockIdx.x, nseg);
}

struct CoefArg {
  CertCoef c;
};

template <int D>
__global__ __launch_bounds__(SEG_ROWS) void k_cert_update(const Seg *segs, NodeMask mask, CoefArg K, const double *__restrict__ Tp,
                                                          double *V, double *W, double *P, double *SV,
                                                          const double *__restrict__ SW, double *SP, double *partial, int nseg) {
  constexpr int RS = (D + 1) * D, B = D + 1;
  const Seg s = segs[blockIdx.x];
  if (!node_on(mask, s.node)) return;
  const int row = s.begin + threadIdx.x;
  double rr[D], vv[D];
#pragma unroll
  for (int j = 0; j < D; j++) rr[j] = vv[j] = 0.0;
  if (row < s.end) {
    const size_t off = (size_t)row * RS;
    double nv[RS], np[RS], nsv[RS], nsp[RS];
    {
      double v[RS], w[RS], p[RS];
      load_rec<RS>(V + off, v);
      load_rec<RS>(W + off, w);
      load_rec<RS>(P + off, p);
#pragma unroll
      for (int r = 0; r <= D; r++)
#pragma unroll
        for (int j = 0; j < D; j++) {
          double a = 0, c = 0;
#pragma unroll
          for (int i = 0; i < D; i++) {
            a = fma(w[r * D + i], K.c.C[(D + i) * D + j], a);
            a = fma(p[r * D + i], K.c.C[(2 * D + i) * D + j], a);
            c = fma(v[r * D + i], K.c.C[i * D + j], c);
          }
          np[r * D + j] = a;
          nv[r * D + j] = c + a;
        }
    }
    {
      double v[RS], w[RS], p[RS];
      load_rec<RS>(SV + off, v);
      load_rec<RS>(SW + off, w);
      load_rec<RS>(SP + off, p);
#pragma unroll
      for (int r = 0; r <= D; r++)
#pragma unroll
        for (int j = 0; j < D; j++) {
          double a = 0, c = 0;
#pragma unroll
          for (int i = 0; i < D; i++) {
            a = fma(w[r * D + i], K.c.C[(D + i) * D + j], a);
            a = fma(p[r * D + i], K.c.C[(2 * D + i) * D + j], a);
            c = fma(v[r * D + i], K.c.C[i * D + j], c);
          }
          nsp[r * D + j] = a;
          nsv[r * D + j] = c + a;
        }
    }
    store_rec<RS>(V + off, nv);
    store_rec<RS>(P + off, np);
    store_rec<RS>(SV + off, nsv);
    store_rec<RS>(SP + off, nsp);
    double res[RS];
#pragma unroll
    for (int r = 0; r <= D; r++)
#pragma unroll
      for (int j = 0; j < D; j++) {
        const double e = fma(-K.c.theta[j], nv[r * D + j], nsv[r * D + j]);
        res[r * D + j] = e;
        rr[j] = fma(e, e, rr[j]);
        vv[j] = fma(nv[r * D + j], nv[r * D + j], vv[j]);
      }
    if (Tp) {   // W' = T_p R'
      double nw[RS];
      const double *t = Tp + (size_t)row * B * B;
#pragma unroll
      for (int r = 0; r < B; r++)
#pragma unroll
        for (int j = 0; j < D; j++) {
          double a = 0;
#pragma unroll
          for (int k = 0; k < B; k++) a = fma(t[r * B + k], res[k * D + j], a);
          nw[r * D + j] = a;
        }
      store_rec<RS>(W + off, nw);
    } else {
      store_rec<RS>(W + off, res);
    }
  }
  constexpr int NT2 = 2 * cert_ntri(D);
#pragma unroll
  for (int j = 0; j < D; j++) {
    const double a = wave_sum(rr[j]), c = wave_sum(vv[j]);
    if (threadIdx.x == 0) {
      partial[(size_t)(NT2 + j) * nseg + blockIdx.x] = a;
      partial[(size_t)(NT2 + D + j) * nseg + blockIdx.x] = c;
    }
  }
}

// The matrix STEP 1 factors, written where the factorisation reads it: one wave per pose, its lanes striding the pose's
// run of values -- a coalesced copy of M with Lambda_p and eta applied to the diagonal block.
template <int D>
__global__ __launch_bounds__(256) void k_cert_matrix(int nposes, const int *__restrict__ bptr, const int *__restrict__ diag_pose,
                                                     const double *__restrict__ Mval, const double *__restrict__ Lam, double eta,
                                                     double *__restrict__ out) {
  constexpr int B = D + 1;
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= nposes) return;
  const int b0 = bptr[p], nb = bptr[p + 1] - b0, rowlen = B * nb, len = B * rowlen;
  const size_t base = (size_t)B * B * b0;
  for (int l = lane; l < len; l += 64) {
    const int r = l / rowlen, rem = l - r * rowlen, j = rem / B, c = rem - j * B;
    double v = Mval[base + l];
    if (diag_pose[b0 + j] >= 0) {
      if (r >= 1 && c >= 1) v -= Lam[(size_t)p * D * D + (r - 1) * D + (c - 1)];
      if (r == c) v += eta;
    }
    out[base + l] = v;
  }
}

// One wave per sum: the segments' partials in a fixed order, the result straight into pinned host memory; the last wave
// to arrive raises the group's read-back flag (the protocol of k_reduce, kernels.hip).
__global__ __launch_bounds__(64) void k_cert_reduce(int nseg, const double *partials, double *host, unsigned *arrived,
                                                    unsigned long long *host_flag, unsigned long long seq,
                                                    unsigned long long *dev_seq) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const double *p = partials + (size_t)s * nseg;
  double v = 0;
  for (int k = lane; k < nseg; k += 64) v += p[k];
  v = wave_sum(v);
  if (lane == 0) {
    __hip_atomic_store(host + s, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __atomic_thread_fence(__ATOMIC_RELEASE);
    const unsigned done = __hip_atomic_fetch_add(arrived, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_SYSTEM);
    if (done == gridDim.x - 1) {
      __hip_atomic_store(arrived, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (seq == 0) seq = *dev_seq + 1;
      *dev_seq = seq;
      __hip_atomic_store(host_flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

}  // namespace

#define CERT_DISPATCH_D(d, ...)        \
  do {                                 \
    if ((d) == 3) {                    \
      constexpr int D = 3;             \
      __VA_ARGS__;                     \
    } else {                           \
      constexpr int D = 2;             \
      __VA_ARGS__;                     \
    }                                  \
  } while (0)

void launch_cert_lambda(const LaunchCtx &lc, const double *X, const double *MX, double *Lam, double *SX, double *partials) {
  const auto &[d, st, T, mask] = lc;
  if (T.nseg_own == 0) return;
  CERT_DISPATCH_D(d, hipLaunchKernelGGL((k_cert_lambda<D>), dim3(T.nseg_own), dim3(SEG_ROWS), 0, st, T.segs, mask, X, MX, Lam, SX,
                                        partials, T.nseg_own));
}

void launch_cert_apply(const LaunchCtx &lc, const double *Lam, const double *V, const double *MV, double *out) {
  const auto &[d, st, T, mask] = lc;
  if (T.nseg_own == 0) return;
  CERT_DISPATCH_D(d, hipLaunchKernelGGL((k_cert_apply<D>), dim3(T.nseg_own), dim3(SEG_ROWS), 0, st, T.segs, mask, Lam, V, MV, out));
}

void launch_cert_gram(const LaunchCtx &lc, const double *Lam, const double *V, const double *W,
                      const double *P, const double *SV, double *SW, const double *SP, double *partials) {
  const auto &[d, st, T, mask] = lc;
  if (T.nseg_own == 0) return;
  CERT_DISPATCH_D(d, hipLaunchKernelGGL((k_cert_gram<D>), dim3(T.nseg_own), dim3(SEG_ROWS), 0, st, T.segs, mask, Lam, V, W, P, SV, SW,
                                        SP, partials, T.nseg_own));
}

void launch_cert_update(const LaunchCtx &lc, const CertCoef &c, const double *Tp, double *V,
                        double *W, double *P, double *SV, const double *SW, double *SP, double *partials) {
  const auto &[d, st, T, mask] = lc;
  if (T.nseg_own == 0) return;
  CoefArg K{c};
  CERT_DISPATCH_D(d, hipLaunchKernelGGL((k_cert_update<D>), dim3(T.nseg_own), dim3(SEG_ROWS), 0, st, T.segs, mask, K, Tp, V, W, P, SV,
                                        SW, SP, partials, T.nseg_own));
}

void launch_cert_matrix(int d, hipStream_t st, int nposes, const int *bptr, const int *diag_pose, const double *Mval,
                        const double *Lam, double eta, double *out) {
  if (nposes == 0) return;
  CERT_DISPATCH_D(d, hipLaunchKernelGGL((k_cert_matrix<D>), dim3((nposes + 3) / 4), dim3(256), 0, st, nposes, bptr, diag_pose, Mval, Lam,
                                        eta, out));
}

void launch_cert_reduce(hipStream_t st, const SegTable &T, int nsums, const double *partials, double *host, ReadbackFlag flag) {
  hipLaunchKernelGGL(k_cert_reduce, dim3(nsums), dim3(64), 0, st, T.nseg_own, partials, host, flag.arrived, flag.host, flag.seq,
                     flag.dev_seq);
}

}  // namespace dpgo
