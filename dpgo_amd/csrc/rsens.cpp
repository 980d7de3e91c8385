// Host side of the sensitivities of the robust objective (rsens.h): sens.cpp's check of the upstream and its batch loop
// (sens_begin, sens_batches) on the TRUE robust Hessian, with this file's edge step.  The lists, the point and the Hessian are
// the robust objective's (robust.cpp: robust_begin, robust_point, robust_hessian_launch), the refusal is the block solves'
// (pairs.cpp: pairs_setup) with the robust buffers in its own part.  The optimiser's state is not touched.
#include "rsens.h"

#include <algorithm>
#include <chrono>
#include <cmath>

#include "cert_state.h"
#include "cov_state.h"
#include "edges.h"
#include "group.h"
#include "robust_math.h"
#include "robust_state.h"
#include "rsens_math.h"
#include "sens_math.h"

namespace dpgo {

int Group::robust_sensitivity(const Graph &g, const double *X, int ld, int loss, double loss_reg, int anchor, long long max_bytes,
                              const double *upstream, int ldu, int k, double *adjoint, double *sens, double *dloss_reg,
                              SensResult &out) {
  out = SensResult();
  if (!upstream || !sens || !dloss_reg || k < 1) {
    fprintf(stderr, "[dpgo_amd] ERROR: robust sensitivity: missing upstream or output arrays, or no column.\n");
    return -1;
  }
  if (robust_begin(g, X, ld, loss, loss_reg, 1, anchor, "robust sensitivity") != 0) return -1;
  const int kb = sens_begin("robust sensitivity", upstream, ldu, k, out);
  if (kb < 0) return -1;
  const int d = d_, dof = cov_dof(d), N = P0_, NO = 3 + dof, m = rob_->plan.m, ncmax = std::min(k, SENS_BATCH);
  const long long n = (long long)dof * N;
  out.edges = m;
  // this call's buffers: the batch, one batch of upstream, one batch of per-edge output, the preparation array, the two row
  // lists; behind them the robust objective's, which an earlier call may have left on the device
  const long long own = 8ll * (n * kb + n * ncmax + (long long)ncmax * m * NO + (long long)m * NO) + 4ll * 2 * N;
  const int ready = pairs_setup(max_bytes, {own + rob_->bytes, own + robust_remain()}, kb, out);
  if (ready < 0) return -1;
  if (ready != 0) return 0;   // SKIPPED: nothing allocated, nothing written, the stationarity not computed
  robust_alloc();
  CertState &c = *cert_;
  RobustState &r = *rob_;
  robust_point(X, ld, loss, loss_reg, &out.stationarity);
  std::fill(sens, sens + (size_t)k * m * NO, 0.0);
  std::fill(dloss_reg, dloss_reg + k, 0.0);
  if (adjoint) std::fill(adjoint, adjoint + (size_t)k * n, 0.0);
  const int rc = hess_factor("robust sensitivity", [&] { robust_hessian_launch(own_row(anchor), 1); }, out);
  if (rc < 0) return -1;
  if (rc != 0) {
    out.outcome = SENS_NOT_PD;
    return 0;
  }
  DevBuf<double> d_prep, d_out;
  d_prep.alloc((size_t)m * NO, false);
  d_out.alloc((size_t)ncmax * m * NO, false);
  return sens_batches("robust sensitivity", anchor, upstream, ldu, k, adjoint, [&](const SensBatch &b) {
    if (b.b == 0) launch_rsens_prep(d, st_, m, r.rec.p, c.X.p, r.out.p, loss, loss_reg, d_prep.p);   // once: every batch reads it
    launch_rsens_edge(d, st_, m, r.rec.p, c.X.p, r.out.p, d_prep.p, b.Xb, b.kb, b.nc, d_out.p);
    HIP_CHECK(hipGetLastError());
    double *dst = sens + (size_t)b.c0 * m * NO;
    HIP_CHECK(hipMemcpyAsync(dst, d_out.p, sizeof(double) * (size_t)b.nc * m * NO, hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
    // dL/ddelta: the edges' terms in ascending order, one column per thread (a column's sum is one thread's, in order)
#pragma omp parallel for schedule(static) if ((long long)b.nc * m > 65536)
    for (int j = 0; j < b.nc; j++) {
      double sum = 0;
      for (int e = 0; e < m; e++) sum += dst[((size_t)j * m + e) * NO + NO - 1];
      dloss_reg[b.c0 + j] = sum;
    }
  }, out);
}

// ---- host only: the per-edge arithmetic of k_rsens_prep and k_rsens_edge through rsens_math.h ----
template <int D>
static void rsens_edge_one(const double *q, const double *a, const double *b, bool inter, int loss, double dl, const double *li,
                           const double *lj, double *o, double *ph) {
  constexpr int NO = 2 + D + D * (D - 1) / 2;
  double v[4], ds[NO], so[NO], phi;
  edge_lane<D>(q, a, b, inter, loss, dl, v);
  const double s = v[0] + v[1], w = v[3];
  rsens_ds<D>(q, a, b, ds);
  sens_one<D>(q, a, b, li, lj, so, &phi);
  rsens_combine<D>(w, robust_curv(loss, dl, s, w, inter), phi, ds, rsens_dw(loss, dl, s, w, inter), so, o);
  if (ph) *ph = phi;
}

int robust_sens_edge_host(const Graph &g, const double *X, int ld, int loss, double loss_reg, const double *lambda, double *sens,
                          double *phi) {
  const int d = g.d, N = g.num_poses, m = (int)g.all.size();
  if ((d != 2 && d != 3) || N <= 0 || m == 0 || !X || ld < (d + 1) * N || !lambda || !sens) return -1;
  if (loss < 0 || loss > 3 || (loss != 0 && !(std::isfinite(loss_reg) && loss_reg > 0))) return -1;
  for (const Measurement &mm : g.all)
    if (mm.ipose < 0 || mm.ipose >= N || mm.jpose < 0 || mm.jpose >= N) return -1;
  std::vector<double> rec, pose((size_t)N * pose_rec_doubles(d));
  edge_records(g, rec);
  pose_records(d, N, X, ld, pose.data());
  const int L = edge_rec_doubles(d), RS = pose_rec_doubles(d), dof = cov_dof(d), NO = 3 + dof;
  for (int e = 0; e < m; e++) {
    const double *q = rec.data() + (size_t)e * L;
    int i, j;
    bool inter;
    edge_head(q, i, j, inter);
    const double *a = pose.data() + (size_t)i * RS, *b = pose.data() + (size_t)j * RS;
    const double *li = lambda + (size_t)dof * i, *lj = lambda + (size_t)dof * j;
    double *o = sens + (size_t)e * NO, *ph = phi ? phi + e : nullptr;
    if (d == 2) rsens_edge_one<2>(q, a, b, inter, loss, loss_reg, li, lj, o, ph);
    else rsens_edge_one<3>(q, a, b, inter, loss, loss_reg, li, lj, o, ph);
  }
  return 0;
}

}  // namespace dpgo
