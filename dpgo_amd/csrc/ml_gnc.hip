// The kernels of graduated non-convexity on the maximum-likelihood objective for gfx950 (ml_gnc.h): the weighted edge pass,
// with weights from the surrogate or from an array; its tail is gnc_partials.h's and its final wave gnc.hip's.  fp64 throughout,
// no fast-math; every sum runs in a fixed order (the lanes of a wave by shuffle, wave_reduce.h; the workgroups' partials
// strided in one final wave): the same bits run to run, no floating-point atomics, no LDS, no inline assembly.
#include "ml_gnc.h"

#include <cmath>

#include "cov.h"
#include "edge_math.h"
#include "gnc_math.h"
#include "gnc_partials.h"
#include "ml_gnc_math.h"

namespace dpgo {
namespace {

// FULL: r, chi2, w (Omega r), the weighted gradient terms and the record [J_i | J_j | w Omega J_i | w Omega J_j] are written;
// otherwise the sums alone (the trial point)
template <int D, bool FULL>
__global__ __launch_bounds__(EDGE_BLOCK) void k_ml_gnc_edge(int m, const double2 *__restrict__ rec, const double *__restrict__ omega,
                                                            const double2 *__restrict__ poses, const int *__restrict__ in_R, int kind,
                                                            double mu, double c2, int weigh, double *__restrict__ warr, MlEdgeOut out,
                                                            double *__restrict__ partials, long long *__restrict__ counts) {
  constexpr int EU = edge_rec_doubles(D) / 2, PU = pose_rec_doubles(D) / 2, RS = pose_rec_doubles(D), DOF = cov_dof(D), DD = DOF * DOF;
  static_assert(edge_rec_doubles(D) % 2 == 0 && pose_rec_doubles(D) % 2 == 0, "records are whole 16-byte units");
  const int e = blockIdx.x * EDGE_BLOCK + threadIdx.x;
  double f_out = 0, f_ws = 0, f_rho = 0, smax = 0, wmin = INFINITY;
  bool zero = false, one = false, between = false, near_w = false, near_all = false;
  if (e < m) {
    double q[2 * EU];
#pragma unroll
    for (int k = 0; k < EU; k++) {
      const double2 u = rec[(size_t)e * EU + k];
      q[2 * k] = u.x;
      q[2 * k + 1] = u.y;
    }
    int i, j;
    bool inter;
    edge_head(q, i, j, inter);
    double a[RS], b[RS];
#pragma unroll
    for (int k = 0; k < PU; k++) {
      const double2 u = poses[(size_t)i * PU + k], v = poses[(size_t)j * PU + k];
      a[2 * k] = u.x;
      a[2 * k + 1] = u.y;
      b[2 * k] = v.x;
      b[2 * k + 1] = v.y;
    }
    double Om[DD], r[DOF], orr[DOF], Ji[DD], Jj[DD];
#pragma unroll
    for (int k = 0; k < DD; k++) Om[k] = omega[(size_t)e * DD + k];
    near_all = ml_residual<D>(q, a, b, r, Ji, Jj);
    const double chi2 = ml_weigh<D>(Om, r, orr);
    double w = 1.0;
    if (in_R[e] != 0) {
      double rho;
      gnc_weight_rho(kind, mu, c2, chi2, w, rho);
      if (weigh) warr[e] = w;
      else w = warr[e];
      f_ws = ml_gnc_wchi2(w, chi2);
      f_rho = rho;
      smax = chi2;
      wmin = w;
      zero = w == 0.0;
      one = w == 1.0;
      between = w > 0.0 && w < 1.0;
    } else {
      f_out = chi2;
    }
    near_w = near_all && w > 0.0;
    if (FULL) {
      out.chi2[e] = chi2;
#pragma unroll
      for (int k = 0; k < DOF; k++) out.r[(size_t)e * DOF + k] = r[k];
      ml_gnc_edge_out<D>(w, Om, Ji, Jj, orr, out.wr + (size_t)e * DOF, out.g + (size_t)2 * e * DOF,
                         out.g + ((size_t)2 * e + 1) * DOF, out.jw + (size_t)e * 4 * DD);
    }
  }
  gnc_store_partials(f_out, f_ws, f_rho, smax, wmin, partials, counts, zero, one, between, near_w, near_all);
}

template <int D, bool FULL>
void launch_edge(hipStream_t st, int nb, int m, const double *rec, const double *omega, const double *X, const int *in_R, int kind,
                 double mu, double c2, bool weigh, double *w, const MlEdgeOut &out, double *partials, long long *counts) {
  hipLaunchKernelGGL((k_ml_gnc_edge<D, FULL>), dim3(nb), dim3(EDGE_BLOCK), 0, st, m, (const double2 *)rec, omega, (const double2 *)X, in_R,
                     kind, mu, c2, weigh ? 1 : 0, w, out, partials, counts);
}

}  // namespace

void launch_ml_gnc_edge(int d, hipStream_t st, int m, const double *rec, const double *omega, const double *X, const int *in_R,
                        int kind, double mu, double c2, bool weigh, double *w, const MlEdgeOut &out, double *partials,
                        long long *counts, MlGncSummaryDev *sum, double *fslot, int nslot) {
  if (m <= 0) return;
  const int nb = (m + EDGE_BLOCK - 1) / EDGE_BLOCK;
  if (d == 3) {
    if (out.r) launch_edge<3, true>(st, nb, m, rec, omega, X, in_R, kind, mu, c2, weigh, w, out, partials, counts);
    else launch_edge<3, false>(st, nb, m, rec, omega, X, in_R, kind, mu, c2, weigh, w, out, partials, counts);
  } else {
    if (out.r) launch_edge<2, true>(st, nb, m, rec, omega, X, in_R, kind, mu, c2, weigh, w, out, partials, counts);
    else launch_edge<2, false>(st, nb, m, rec, omega, X, in_R, kind, mu, c2, weigh, w, out, partials, counts);
  }
  launch_gnc_final(st, nb, ML_GNC_COUNT_SLOTS, partials, counts, &sum->gnc, fslot, nslot);
}

}  // namespace dpgo
