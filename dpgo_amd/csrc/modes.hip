// The kernels of the Hessian modes for gfx950 (modes.h): the start block, the two Gram matrices of a tall block pair, the
// Ritz update with its residuals, and the reduction of the workgroups' partial sums.
//
// fp64 throughout, no fast-math.  The products run on v_mfma_f64_16x16x4_f64, laid out as k_ms_forward (spd_dev.hip) lays it
// out: lane l hands in A[l & 15][l >> 4] and B[l >> 4][l & 15], and register r of lane l is C[(l >> 4) + 4 r][l & 15].  A
// workgroup owns MODES_ROWS consecutive rows whatever b is, every entry is one chain of instructions over those rows in
// ascending order, and k_modes_reduce adds the workgroups in order: the same bits on every call, no atomics, and an entry's
// bits depend neither on b nor on the other columns.
#include "modes.h"

#include <cstdint>

namespace dpgo {
namespace {

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int MG_SLAB = 32;   // rows of W and V staged in LDS at a time
constexpr int MG_LD = 80;     // their row length in LDS: the four depths one instruction reads lie 32 banks apart

__global__ __launch_bounds__(256) void k_modes_init(long long n, int b, int ld, int a0, int dof, unsigned long long seed,
                                                    const int *__restrict__ gid, int row_dof, double *__restrict__ V) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n * b) return;
  const long long i = e / b;
  const int j = (int)(e % b);
  const long long u = gid ? (long long)row_dof * gid[i / row_dof] + i % row_dof : i;
  const bool anch = a0 >= 0 && i >= a0 && i < a0 + dof;
  V[i * ld + j] = anch ? 0.0 : modes_start_entry(seed, (unsigned long long)u, (unsigned)j);
}

// G = W'W and T = W'V, the tiles on or below the diagonal, over the workgroup's rows.  Job q = ti (ti + 1) / 2 + tj is the tile
// (ti, tj) of BOTH matrices -- they share the A operand, the columns ti of W -- and wave w takes the jobs w, w + 4, w + 8.  W
// and V go through LDS MG_SLAB rows at a time, each read from memory once, the next slab's loads in flight behind the
// products; a slab's tail is padded with zero rows to a multiple of four.
template <int NT>
__global__ __launch_bounds__(256) void k_modes_gram(long long n, int ld, int vec, const double *__restrict__ W,
                                                    const double *__restrict__ V, double *__restrict__ partials) {
  constexpr int B = 16 * NT, NJ = NT * (NT + 1) / 2, Q = (NJ + 3) / 4, PER = MG_SLAB * B / 256;
  __shared__ double Ws[MG_SLAB][MG_LD], Vs[MG_SLAB][MG_LD];
  const int t = threadIdx.x, wv = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const long long r0 = (long long)blockIdx.x * MODES_ROWS, r1 = min(n, r0 + MODES_ROWS);
  int ti[Q], tj[Q];
  v4d accG[Q], accT[Q];
#pragma unroll
  for (int q = 0; q < Q; q++) {
    const int job = wv + 4 * q;
    int i = 0;
    while ((i + 1) * (i + 2) / 2 <= job) i++;
    ti[q] = i;
    tj[q] = job - i * (i + 1) / 2;
    accG[q] = v4d{0.0, 0.0, 0.0, 0.0};
    accT[q] = v4d{0.0, 0.0, 0.0, 0.0};
  }
  double pw[PER], pv[PER];
  auto fetch = [&](long long k0) {
    if (vec) {
#pragma unroll
      for (int j = 0; j < PER / 2; j++) {
        const int idx = t + 256 * j, c = 2 * (idx % (B / 2));
        const long long row = k0 + idx / (B / 2);
        double2 w = {0.0, 0.0}, v = {0.0, 0.0};
        if (row < r1) {
          w = *reinterpret_cast<const double2 *>(W + row * ld + c);
          v = *reinterpret_cast<const double2 *>(V + row * ld + c);
        }
        pw[2 * j] = w.x; pw[2 * j + 1] = w.y;
        pv[2 * j] = v.x; pv[2 * j + 1] = v.y;
      }
    } else {
#pragma unroll
      for (int j = 0; j < PER; j++) {
        const int idx = t + 256 * j, c = idx % B;
        const long long row = k0 + idx / B;
        pw[j] = row < r1 ? W[row * ld + c] : 0.0;
        pv[j] = row < r1 ? V[row * ld + c] : 0.0;
      }
    }
  };
  fetch(r0);
  for (long long k0 = r0; k0 < r1; k0 += MG_SLAB) {
    const int kn4 = ((int)min((long long)MG_SLAB, r1 - k0) + 3) & ~3;
    __syncthreads();
    if (vec) {
#pragma unroll
      for (int j = 0; j < PER / 2; j++) {
        const int idx = t + 256 * j, r = idx / (B / 2), c = 2 * (idx % (B / 2));
        Ws[r][c] = pw[2 * j]; Ws[r][c + 1] = pw[2 * j + 1];
        Vs[r][c] = pv[2 * j]; Vs[r][c + 1] = pv[2 * j + 1];
      }
    } else {
#pragma unroll
      for (int j = 0; j < PER; j++) {
        const int idx = t + 256 * j;
        Ws[idx / B][idx % B] = pw[j];
        Vs[idx / B][idx % B] = pv[j];
      }
    }
    __syncthreads();
    if (k0 + MG_SLAB < r1) fetch(k0 + MG_SLAB);
#pragma unroll
    for (int kk = 0; kk < MG_SLAB; kk += 4) {
      if (kk >= kn4) break;
      const int kq = kk + (lane >> 4), rr = lane & 15;
#pragma unroll
      for (int q = 0; q < Q; q++) {
        if (wv + 4 * q >= NJ) continue;
        const double a = Ws[kq][ti[q] * 16 + rr];
        accG[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Ws[kq][tj[q] * 16 + rr], accG[q], 0, 0, 0);
        accT[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Vs[kq][tj[q] * 16 + rr], accT[q], 0, 0, 0);
      }
    }
  }
  double *out = partials + (size_t)blockIdx.x * 2 * B * B;
#pragma unroll
  for (int q = 0; q < Q; q++) {
    if (wv + 4 * q >= NJ) continue;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int i = ti[q] * 16 + (lane >> 4) + 4 * r, j = tj[q] * 16 + (lane & 15);
      out[i * B + j] = accG[q][r];
      out[B * B + i * B + j] = accT[q][r];
    }
  }
}

// V <- W C and the residual columns V_old C - (W C) Theta, 16 rows per wave at a time, C and Theta staged in LDS once per
// workgroup.  A wave reads every entry of its 16 rows of V before it writes one (a row depends only on itself); the tiles
// t of a workgroup's rows go to wave t mod 4 whatever b is, a lane's sums run over its tiles in order, then lanes l, l ^ 16,
// l ^ 32 and the four waves in order: a fixed tree.
template <int NT>
__global__ __launch_bounds__(256) void k_modes_update(long long n, int ld, int a0, int dof, const double *__restrict__ W, double *V,
                                                      const double *__restrict__ C, const double *__restrict__ theta,
                                                      double *__restrict__ partials) {
  constexpr int B = 16 * NT, LDC = B + 16;
  __shared__ double Cs[B][LDC], Th[B], red[4][2 * B];
  const int t = threadIdx.x, wv = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  for (int idx = t; idx < B * B; idx += 256) Cs[idx / B][idx % B] = C[idx];
  if (t < B) Th[t] = theta[t];
  __syncthreads();
  const long long r0 = (long long)blockIdx.x * MODES_ROWS, r1 = min(n, r0 + MODES_ROWS);
  double rr[NT], vv[NT];
#pragma unroll
  for (int ct = 0; ct < NT; ct++) rr[ct] = vv[ct] = 0.0;
  for (long long tr = r0 + 16 * wv; tr < r1; tr += 64) {
    const long long ra = tr + (lane & 15);
    const bool in = ra < r1;
    v4d aw[NT], av[NT];
#pragma unroll
    for (int ct = 0; ct < NT; ct++) aw[ct] = av[ct] = v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int kk = 0; kk < B; kk += 4) {
      const int kq = kk + (lane >> 4);
      const double w = in ? W[ra * ld + kq] : 0.0, v = in ? V[ra * ld + kq] : 0.0;
#pragma unroll
      for (int ct = 0; ct < NT; ct++) {
        const double c = Cs[kq][ct * 16 + (lane & 15)];
        aw[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(w, c, aw[ct], 0, 0, 0);
        av[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(v, c, av[ct], 0, 0, 0);
      }
    }
#pragma unroll
    for (int ct = 0; ct < NT; ct++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const long long row = tr + (lane >> 4) + 4 * r;
        const int col = ct * 16 + (lane & 15);
        if (row >= r1) continue;
        const bool anch = a0 >= 0 && row >= a0 && row < a0 + dof;
        const double wc = anch ? 0.0 : aw[ct][r], res = anch ? 0.0 : fma(-wc, Th[col], av[ct][r]);
        V[row * ld + col] = wc;
        rr[ct] = fma(res, res, rr[ct]);
        vv[ct] = fma(wc, wc, vv[ct]);
      }
  }
#pragma unroll
  for (int ct = 0; ct < NT; ct++) {
    rr[ct] += __shfl_xor(rr[ct], 16, 64);
    rr[ct] += __shfl_xor(rr[ct], 32, 64);
    vv[ct] += __shfl_xor(vv[ct], 16, 64);
    vv[ct] += __shfl_xor(vv[ct], 32, 64);
    if (lane < 16) {
      red[wv][ct * 16 + lane] = rr[ct];
      red[wv][B + ct * 16 + lane] = vv[ct];
    }
  }
  __syncthreads();
  if (t < 2 * B) partials[(size_t)blockIdx.x * 2 * B + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
}

// out[dst(e)] = the workgroups' partials of entry e in order.  tri_b > 0: e runs over two tri_b x tri_b matrices and only
// j <= i is handed out, packed by rows, one triangle behind the other.  The last workgroup to arrive raises the flag (the
// protocol of k_polish_reduce, polish.hip); host_flag null: none.
__global__ __launch_bounds__(256) void k_modes_reduce(int nwg, int stride, int nent, int tri_b, const double *__restrict__ partials,
                                                      double *out, unsigned *arrived, unsigned long long *host_flag,
                                                      unsigned long long seq, unsigned long long *dev_seq) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < nent) {
    int dst = e;
    bool on = true;
    if (tri_b > 0) {
      const int bb = tri_b * tri_b, m = e / bb, i = (e % bb) / tri_b, j = e % tri_b;
      on = j <= i;
      dst = m * (tri_b * (tri_b + 1) / 2) + i * (i + 1) / 2 + j;
    }
    if (on) {
      double v = 0.0;
      for (int w = 0; w < nwg; w++) v += partials[(size_t)w * stride + e];
      __hip_atomic_store(out + dst, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
  if (!host_flag) return;
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) {
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

__global__ __launch_bounds__(256) void k_modes_column(long long n, int ld, int col, double coef, const double *__restrict__ V,
                                                      double *__restrict__ sol) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) sol[i] = coef * V[i * ld + col];
}

}  // namespace

#define MODES_DISPATCH_NT(b, ...)                      \
  do {                                                 \
    switch ((b) / 16) {                                \
      case 1: { constexpr int NT = 1; __VA_ARGS__; } break; \
      case 2: { constexpr int NT = 2; __VA_ARGS__; } break; \
      case 3: { constexpr int NT = 3; __VA_ARGS__; } break; \
      default: { constexpr int NT = 4; __VA_ARGS__; } break; \
    }                                                  \
  } while (0)

void launch_modes_init(hipStream_t st, long long n, int b, int ld, int a0, int dof, unsigned long long seed, const int *gid,
                       int row_dof, double *V) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_modes_init, dim3((unsigned)((n * b + 255) / 256)), dim3(256), 0, st, n, b, ld, a0, dof, seed, gid, row_dof, V);
}

void launch_modes_gram(hipStream_t st, long long n, int b, int ld, const double *W, const double *V, double *partials) {
  if (n <= 0) return;
  const int vec = (ld & 1) == 0 && (((uintptr_t)W | (uintptr_t)V) & 15) == 0;
  MODES_DISPATCH_NT(b, hipLaunchKernelGGL((k_modes_gram<NT>), dim3(modes_workgroups(n)), dim3(256), 0, st, n, ld, vec, W, V, partials));
}

void launch_modes_update(hipStream_t st, long long n, int b, int ld, int a0, int dof, const double *W, double *V, const double *C,
                         const double *theta, double *partials) {
  if (n <= 0) return;
  MODES_DISPATCH_NT(b, hipLaunchKernelGGL((k_modes_update<NT>), dim3(modes_workgroups(n)), dim3(256), 0, st, n, ld, a0, dof, W, V, C, theta,
                                          partials));
}

void launch_modes_reduce_gram(hipStream_t st, int nwg, int b, const double *partials, double *out, ReadbackFlag flag) {
  hipLaunchKernelGGL(k_modes_reduce, dim3((2 * b * b + 255) / 256), dim3(256), 0, st, nwg, 2 * b * b, 2 * b * b, b, partials, out,
                     flag.arrived, flag.host, flag.seq, flag.dev_seq);
}

void launch_modes_reduce(hipStream_t st, int nwg, int stride, int nent, const double *partials, double *out, ReadbackFlag flag) {
  hipLaunchKernelGGL(k_modes_reduce, dim3((nent + 255) / 256), dim3(256), 0, st, nwg, stride, nent, 0, partials, out, flag.arrived,
                     flag.host, flag.seq, flag.dev_seq);
}

void launch_modes_column(hipStream_t st, long long n, int ld, int col, double coef, const double *V, double *sol) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_modes_column, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, ld, col, coef, V, sol);
}

}  // namespace dpgo
