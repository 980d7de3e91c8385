// The kernels of graduated non-convexity for gfx950 (gnc.h): the edge pass with weights from the surrogate or from an array,
// and its final wave.  fp64 throughout, no fast-math; every sum runs in a fixed order (the lanes of a wave by shuffle, the
// workgroups' partials strided in one final wave; wave_reduce.h): the same bits run to run, no atomics, no LDS, no inline
// assembly.
#include "gnc.h"

#include <cmath>

#include "gnc_math.h"
#include "gnc_partials.h"
#include "robust_math.h"

namespace dpgo {
namespace {

template <int D>
__global__ __launch_bounds__(EDGE_BLOCK) void k_gnc_edge(int m, const double2 *__restrict__ rec, const double2 *__restrict__ poses,
                                                         int kind, double mu, double c2, int weigh, double *__restrict__ warr,
                                                         double *__restrict__ s_out, double *__restrict__ rows,
                                                         double *__restrict__ partials, long long *__restrict__ counts) {
  constexpr int EU = edge_rec_doubles(D) / 2, PU = pose_rec_doubles(D) / 2, RS = pose_rec_doubles(D);
  static_assert(edge_rec_doubles(D) % 2 == 0 && pose_rec_doubles(D) % 2 == 0, "records are whole 16-byte units");
  const int e = blockIdx.x * EDGE_BLOCK + threadIdx.x;
  double f_out = 0, f_ws = 0, f_rho = 0, smax = 0, wmin = INFINITY;
  bool zero = false, one = false, between = false;
  if (e < m) {
    double q[2 * EU];
#pragma unroll
    for (int k = 0; k < EU; k++) {
      const double2 u = rec[(size_t)e * EU + k];
      q[2 * k] = u.x;
      q[2 * k + 1] = u.y;
    }
    int i, j;
    bool in_R;
    edge_head(q, i, j, in_R);
    double a[RS], b[RS];
#pragma unroll
    for (int k = 0; k < PU; k++) {
      const double2 u = poses[(size_t)i * PU + k], v = poses[(size_t)j * PU + k];
      a[2 * k] = u.x;
      a[2 * k + 1] = u.y;
      b[2 * k] = v.x;
      b[2 * k + 1] = v.y;
    }
    double v[4];
    edge_lane<D>(q, a, b, in_R, 0, 0.0, v);
    const double s = v[2];   // (loss 0: the rounded sum of the two rounded parts)
    s_out[e] = v[0];
    s_out[(size_t)m + e] = v[1];
    if (rows) {
      double ri[RS], rj[RS];
      robust_rows<D>(q, a, b, ri, rj);
      double2 *dst = (double2 *)rows + (size_t)e * 2 * PU;
#pragma unroll
      for (int k = 0; k < PU; k++) {
        dst[k] = make_double2(ri[2 * k], ri[2 * k + 1]);
        dst[PU + k] = make_double2(rj[2 * k], rj[2 * k + 1]);
      }
    }
    if (in_R) {
      double w, rho;
      gnc_weight_rho(kind, mu, c2, s, w, rho);
      if (weigh) warr[e] = w;
      else w = warr[e];
      {
#pragma clang fp contract(off)
        f_ws = w * s;
      }
      f_rho = rho;
      smax = s;
      wmin = w;
      zero = w == 0.0;
      one = w == 1.0;
      between = w > 0.0 && w < 1.0;
    } else {
      f_out = s;
    }
  }
  gnc_store_partials(f_out, f_ws, f_rho, smax, wmin, partials, counts, zero, one, between);
}

// NC counts per workgroup; the NC - 3 past num_between follow the struct (MlGncSummaryDev and its static_asserts, ml_gnc.h)
template <int NC>
__global__ __launch_bounds__(64) void k_gnc_final(int nb, const double *__restrict__ partials, const long long *__restrict__ counts,
                                                  GncSummaryDev *__restrict__ sum, double *__restrict__ fslot, int nslot) {
  static_assert(NC >= GNC_COUNT_SLOTS, "the three counts of GncSummaryDev come first");
  const int lane = threadIdx.x;
  double fo = 0, fw = 0, fr = 0, smax = 0, wmin = INFINITY;
  long long n[NC] = {};
  for (int k = lane; k < nb; k += 64) {
    fo += partials[k];
    fw += partials[(size_t)nb + k];
    fr += partials[2 * (size_t)nb + k];
    smax = fmax(smax, partials[3 * (size_t)nb + k]);
    wmin = fmin(wmin, partials[4 * (size_t)nb + k]);
#pragma unroll
    for (int c = 0; c < NC; c++) n[c] += counts[c * (size_t)nb + k];
  }
  fo = wave_sum(fo);
  fw = wave_sum(fw);
  fr = wave_sum(fr);
  smax = wave_max(smax);
  wmin = wave_min(wmin);
#pragma unroll
  for (int c = 0; c < NC; c++) n[c] = wave_sum(n[c]);
  if (fslot)
    for (int k = lane == 0 ? 64 : lane; k < nslot; k += 64) fslot[k] = 0.0;
  if (lane == 0) {
    sum->sum_out = fo;
    sum->sum_ws = fw;
    sum->sum_rho = fr;
    sum->s_max = smax;
    sum->w_min = wmin;
    sum->num_zero = n[0];
    sum->num_one = n[1];
    sum->num_between = n[2];
    long long *more = reinterpret_cast<long long *>(sum + 1);
#pragma unroll
    for (int c = GNC_COUNT_SLOTS; c < NC; c++) more[c - GNC_COUNT_SLOTS] = n[c];
    if (fslot) fslot[0] = 0.5 * fo + 0.5 * fw;
  }
}

}  // namespace

void launch_gnc_edge(int d, hipStream_t st, int m, const double *rec, const double *X, int kind, double mu, double c2, bool weigh,
                     double *w, double *s_out, double *rows, double *partials, long long *counts, GncSummaryDev *sum, double *fslot,
                     int nslot) {
  if (m <= 0) return;
  const int nb = (m + EDGE_BLOCK - 1) / EDGE_BLOCK;
  if (d == 3)
    hipLaunchKernelGGL(k_gnc_edge<3>, dim3(nb), dim3(EDGE_BLOCK), 0, st, m, (const double2 *)rec, (const double2 *)X, kind, mu, c2,
                       weigh ? 1 : 0, w, s_out, rows, partials, counts);
  else
    hipLaunchKernelGGL(k_gnc_edge<2>, dim3(nb), dim3(EDGE_BLOCK), 0, st, m, (const double2 *)rec, (const double2 *)X, kind, mu, c2,
                       weigh ? 1 : 0, w, s_out, rows, partials, counts);
  launch_gnc_final(st, nb, GNC_COUNT_SLOTS, partials, counts, sum, fslot, nslot);
}

void launch_gnc_final(hipStream_t st, int nb, int ncounts, const double *partials, const long long *counts, GncSummaryDev *sum,
                      double *fslot, int nslot) {
  if (ncounts == GNC_COUNT_SLOTS)
    hipLaunchKernelGGL(k_gnc_final<GNC_COUNT_SLOTS>, dim3(1), dim3(64), 0, st, nb, partials, counts, sum, fslot, nslot);
  else
    hipLaunchKernelGGL(k_gnc_final<ML_GNC_COUNT_SLOTS>, dim3(1), dim3(64), 0, st, nb, partials, counts, sum, fslot, nslot);
}

}  // namespace dpgo
