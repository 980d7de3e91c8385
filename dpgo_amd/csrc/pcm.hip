// PCM pairwise consistency (C++/DPGO/src/PCM.cpp:194-230) on gfx950: the O(m^2) part of PCM::update.
//
// One wave per (64-column chunk, tile of PCM_TR rows); a block is PCM_WAVES waves that share the column chunk.  The
// records of the chunk's columns and of the block's rows are staged in LDS.  Lane c of the wave evaluates the entry
// (r, c) as the reference's pair (p, q) = (min(r, c), max(r, c)) -- p in its first role, q in its second -- so both
// triangles come out of the same formula and the bit matrix is symmetric without a transpose (2x the FLOPs of the
// triangle; the kernel is far from any bound that would make that matter at the sizes PCM sees).  __ballot(err <= tol)
// gives the row's 64-bit word, which lane 0 stores.  Lanes past m vote false (cleared tail bits), the diagonal votes
// true.  fp64 throughout, no fast-math; no atomics.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "pcm.h"

namespace dpgo {

constexpr int PCM_TR = 8;      // rows per wave
constexpr int PCM_WAVES = 4;   // waves per block
constexpr int PCM_ROWS = PCM_TR * PCM_WAVES;

// The reference's pair error for measurement p (first role) and q (second role), composed in its own order:
// Rii = Ri1' Ri0, tii = Ri1' (ti0 - ti1), Rjj = Rj0' Rj1, tjj = Rj0' (tj1 - tj0),
// Raj1 = Rij Rjj, taj1 = tij + Rij tjj, Rai1 = Raj1 Rji, tai1 = taj1 + Raj1 tji, Rai0 = Rai1 Rii, tai0 = tai1 + Rai1 tii,
// error = sqrt(kappa |Rai0 - I|_F^2 + tau |tai0|^2).
template <int D>
__device__ __forceinline__ double pair_error(const double *P, const double *Q, bool weighted) {
  constexpr int RT = D * D + D;
  const double *Ri0 = P, *ti0 = P + D * D, *Rj0 = P + RT, *tj0 = P + RT + D * D, *Rij = P + 2 * RT, *tij = P + 2 * RT + D * D;
  const double *Ri1 = Q, *ti1 = Q + D * D, *Rj1 = Q + RT, *tj1 = Q + RT + D * D, *Rji = Q + 3 * RT, *tji = Q + 3 * RT + D * D;
  double Rii[D * D], tii[D], Rjj[D * D], tjj[D], dti[D], dtj[D];
#pragma unroll
  for (int k = 0; k < D; k++) {
    dti[k] = ti0[k] - ti1[k];
    dtj[k] = tj1[k] - tj0[k];
  }
#pragma unroll
  for (int a = 0; a < D; a++) {
#pragma unroll
    for (int b = 0; b < D; b++) {
      double si = 0, sj = 0;
#pragma unroll
      for (int k = 0; k < D; k++) {
        si += Ri1[k * D + a] * Ri0[k * D + b];
        sj += Rj0[k * D + a] * Rj1[k * D + b];
      }
      Rii[a * D + b] = si;
      Rjj[a * D + b] = sj;
    }
    double ui = 0, uj = 0;
#pragma unroll
    for (int k = 0; k < D; k++) {
      ui += Ri1[k * D + a] * dti[k];
      uj += Rj0[k * D + a] * dtj[k];
    }
    tii[a] = ui;
    tjj[a] = uj;
  }
  // Raj1 = Rij Rjj, taj1 = tij + Rij tjj
  double Ra[D * D], ta[D], Rb[D * D], tb[D];
#pragma unroll
  for (int a = 0; a < D; a++) {
    double s = 0;
#pragma unroll
    for (int k = 0; k < D; k++) s += Rij[a * D + k] * tjj[k];
    ta[a] = tij[a] + s;
#pragma unroll
    for (int b = 0; b < D; b++) {
      double r = 0;
#pragma unroll
      for (int k = 0; k < D; k++) r += Rij[a * D + k] * Rjj[k * D + b];
      Ra[a * D + b] = r;
    }
  }
  // Rai1 = Raj1 Rji, tai1 = taj1 + Raj1 tji
#pragma unroll
  for (int a = 0; a < D; a++) {
    double s = 0;
#pragma unroll
    for (int k = 0; k < D; k++) s += Ra[a * D + k] * tji[k];
    tb[a] = ta[a] + s;
#pragma unroll
    for (int b = 0; b < D; b++) {
      double r = 0;
#pragma unroll
      for (int k = 0; k < D; k++) r += Ra[a * D + k] * Rji[k * D + b];
      Rb[a * D + b] = r;
    }
  }
  // Rai0 = Rai1 Rii, tai0 = tai1 + Rai1 tii
  double eR = 0, eT = 0;
#pragma unroll
  for (int a = 0; a < D; a++) {
    double s = 0;
#pragma unroll
    for (int k = 0; k < D; k++) s += Rb[a * D + k] * tii[k];
    const double t = tb[a] + s;
    eT += t * t;
#pragma unroll
    for (int b = 0; b < D; b++) {
      double r = 0;
#pragma unroll
      for (int k = 0; k < D; k++) r += Rb[a * D + k] * Rii[k * D + b];
      const double e = r - (a == b ? 1.0 : 0.0);
      eR += e * e;
    }
  }
  constexpr int KAP = 4 * RT;
  const double kappa = weighted ? 0.5 * (P[KAP] + Q[KAP]) : 1.0;
  const double tau = weighted ? 0.5 * (P[KAP + 1] + Q[KAP + 1]) : 1.0;
  return sqrt(kappa * eR + tau * eT);
}

template <int D, bool ERR>
__global__ __launch_bounds__(64 * PCM_WAVES) void k_pcm_pairs(int m, int W, const double *__restrict__ rec, double tol,
                                                             int weighted, unsigned long long *__restrict__ bits,
                                                             double *__restrict__ err) {
  constexpr int L = pcm_rec_len(D);
  __shared__ double s_col[64 * L];
  __shared__ double s_row[PCM_ROWS * L];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c0 = blockIdx.x * 64, r0 = blockIdx.y * PCM_ROWS;
  const int ncol = min(64, m - c0), nrow = min(PCM_ROWS, m - r0);
  for (int k = threadIdx.x; k < ncol * L; k += blockDim.x) s_col[k] = rec[(size_t)c0 * L + k];
  for (int k = threadIdx.x; k < nrow * L; k += blockDim.x) s_row[k] = rec[(size_t)r0 * L + k];
  __syncthreads();
  const int c = c0 + lane;
  for (int i = 0; i < PCM_TR; i++) {
    const int rl = wave * PCM_TR + i, r = r0 + rl;
    if (r >= m) break;   // uniform across the wave
    bool ok = false;
    double e = 0;
    if (c < m) {
      if (c == r) {
        ok = true;
      } else {
        const double *lo = c < r ? s_col + lane * L : s_row + rl * L;
        const double *hi = c < r ? s_row + rl * L : s_col + lane * L;
        e = pair_error<D>(lo, hi, weighted != 0);
        ok = e <= tol;
      }
    }
    const unsigned long long word = __ballot(ok);
    if (lane == 0) bits[(size_t)r * W + blockIdx.x] = word;
    if (ERR && c < m) err[(size_t)r * m + c] = e;
  }
}

int pcm_pairs_launch(int d, int m, const double *rec, double tol, bool weighted, uint64_t *bits, double *err,
                     void *stream) {
  if (m <= 0) return 0;
  if (m > PCM_MAX_M || (err && m > PCM_MAX_M_ERRORS) || (d != 2 && d != 3)) return -1;
  const int W = (m + 63) / 64;
  const dim3 grid(W, (m + PCM_ROWS - 1) / PCM_ROWS), block(64 * PCM_WAVES);
  hipStream_t st = (hipStream_t)stream;
  auto *b = (unsigned long long *)bits;
  const int w = weighted ? 1 : 0;
  if (d == 2) {
    if (err) hipLaunchKernelGGL((k_pcm_pairs<2, true>), grid, block, 0, st, m, W, rec, tol, w, b, err);
    else hipLaunchKernelGGL((k_pcm_pairs<2, false>), grid, block, 0, st, m, W, rec, tol, w, b, nullptr);
  } else {
    if (err) hipLaunchKernelGGL((k_pcm_pairs<3, true>), grid, block, 0, st, m, W, rec, tol, w, b, err);
    else hipLaunchKernelGGL((k_pcm_pairs<3, false>), grid, block, 0, st, m, W, rec, tol, w, b, nullptr);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    fprintf(stderr, "[dpgo_amd] ERROR: k_pcm_pairs launch: %s\n", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

}  // namespace dpgo
