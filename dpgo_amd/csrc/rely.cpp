// Host side of the per-edge reliability (rely.h): the graph against the group, the listed edges, the two predictions and the
// refusal, and the call -- H written on the device (k_cov_hessian) and factored (hess.cpp: hess_factor), the three blocks of every
// listed edge gathered out of the selected inversion (spd_selinv_device, k_rely_gather) or solved for batch by batch
// (pairs.cpp: pairs_solve_joint), the relative covariance and the residual of every edge (k_pairs_gate), its record
// (k_rely_edge).  The matrix, its symbolic analysis and its numeric context are the covariance's (cov.cpp), the edge records
// the robust objective's (robust.cpp: graph_records_own).  The optimiser's state is not touched (cert_begin).
#include "rely.h"

#include <algorithm>
#include <chrono>
#include <cmath>

#include "cert_state.h"
#include "cov_state.h"
#include "edge_math.h"
#include "edges.h"
#include "group.h"
#include "rely_math.h"

namespace dpgo {

// The three blocks S_pp, S_pq, S_qq of nu listed edges behind a factorisation that succeeded, into d_joint (device, nu x 3 dof^2,
// zeroed by the caller: the anchor's blocks under SOLVE): gathered out of the selected inversion (RELY_SELINV) or solved for
// batch by batch (pairs_solve_joint).  prow: the unified own rows of every edge's two poses, d_prow the same on the device.
// Returns behind a synchronise.  edge_reliability and ml_edge_reliability (ml_rely.cpp) share it.
int Group::rely_joint(int use, const PairsPlan &pl, int nu, const std::vector<int> &prow, int arow, const int *d_prow, double *d_joint,
                      const char *who) {
  if (use != RELY_SELINV) return pairs_solve_joint(pl, nu, d_prow, d_joint, who);
  CertState &c = *cert_;
  CovState &s = *cov_;
  const int dof = cov_dof(d_), NL = rely_map_ints(dof);
  if (spd_selinv_device(s.F, st_) != 0) {
    fprintf(stderr, "[dpgo_amd] ERROR: %s: the selected inversion failed on the device.\n", who);
    return -1;
  }
  // the map: a pose's dof unknowns are pivots of one front, whose S_pp holds its marginal; the block of an edge lies in the
  // front of whichever pose is eliminated first, whose update rows hold the other (cov.cpp: cov_finish)
  const SpdFactor &F = s.F;
  const std::vector<int64_t> foff = spd_selinv_offsets(F);
  std::vector<int64_t> off((size_t)3 * nu, -1);
  std::vector<int> loc((size_t)NL * nu, 0);
  for (int k = 0; k < nu; k++) {
    const int p = prow[2 * k], q = prow[2 * k + 1];
    int *l = &loc[(size_t)NL * k];
    const int fp = s.piv_front[dof * p], fq = s.piv_front[dof * q], fx = std::min(fp, fq);
    for (int a = 0; a < dof; a++) {
      if (s.piv_front[dof * p + a] != fp || s.piv_front[dof * q + a] != fq) {
        fprintf(stderr, "[dpgo_amd] ERROR: %s: the unknowns of a pose are spread over two fronts.\n", who);
        return -1;
      }
      l[3 + a] = s.piv_loc[dof * p + a];
      l[3 + dof + a] = s.piv_loc[dof * q + a];
    }
    l[0] = F.w[fp] + F.u[fp];
    l[1] = F.w[fx] + F.u[fx];
    l[2] = F.w[fq] + F.u[fq];
    if (p != arow) off[(size_t)3 * k] = foff[fp];
    if (q != arow) off[(size_t)3 * k + 2] = foff[fq];
    if (p == arow || q == arow) continue;
    const int w = F.w[fx], u = F.u[fx];
    const int *up = u ? &F.upd_idx[F.upd_ptr[fx]] : nullptr;
    for (int side = 0; side < 2; side++) {
      const int pose = side == 0 ? p : q;
      for (int a = 0; a < dof; a++) {
        const int v = dof * pose + a;
        int lv = -1;
        if (s.piv_front[v] == fx) lv = s.piv_loc[v];
        else {
          const int *it = std::lower_bound(up, up + u, v);
          if (it != up + u && *it == v) lv = w + (int)(it - up);
          else
            for (int t = 0; t < u && lv < 0; t++)   // (update rows that are not ascending)
              if (up[t] == v) lv = w + t;
        }
        if (lv < 0 || lv >= w + u) {
          fprintf(stderr, "[dpgo_amd] ERROR: %s: edge (%d, %d) lies outside the factor's pattern.\n", who, c.gid[p], c.gid[q]);
          return -1;
        }
        l[3 + (2 + side) * dof + a] = lv;
      }
    }
    off[(size_t)3 * k + 1] = foff[fx];
  }
  DevBuf<int64_t> d_off;
  DevBuf<int> d_loc;
  d_off.upload(off);
  d_loc.upload(loc);
  launch_rely_gather(st_, dof, nu, d_off.p, d_loc.p, spd_selinv_values(s.F), d_joint);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(st_));
  return 0;
}

int Group::edge_reliability(const Graph &g, const double *X, int ld, int anchor, long long max_bytes, int method, const int *edges,
                            int nedges, double *rec_out, double *rel, double *joint, RelyResult &out) {
  out = RelyResult();
  if (!rec_out || (edges && nedges < 0)) {
    fprintf(stderr, "[dpgo_amd] ERROR: edge_reliability: missing output array, or a negative number of edges.\n");
    return -1;
  }
  if (method != RELY_AUTO && method != RELY_SELINV && method != RELY_SOLVE) {
    fprintf(stderr, "[dpgo_amd] ERROR: edge_reliability: method %d is none of AUTO, SELINV, SOLVE.\n", method);
    return -1;
  }
  if (cov_begin(X, ld, anchor) != 0) return -1;
  std::vector<double> rec;
  if (graph_records_own(g, "edge_reliability", rec) != 0) return -1;
  CertState &c = *cert_;
  const int d = d_, dof = cov_dof(d), DD = dof * dof, N = P0_, m = (int)g.all.size(), L = edge_rec_doubles(d);
  const int NC = d * d + d + 2, NG = 2 + dof, W = rely_width(d), NL = rely_map_ints(dof);
  const int nl = edges ? nedges : m;
  for (int k = 0; k < nl; k++)
    if (edges && (edges[k] < 0 || edges[k] >= m)) {
      fprintf(stderr, "[dpgo_amd] ERROR: edge_reliability: entry %d of the list names edge %d of %d.\n", k, edges[k], m);
      return -1;
    }
  out.edges = nl;
  // the listed edges with weights: what is uploaded (live[i]: its position in the list); the others are flag-2 records
  std::vector<int> live, prow, pairs;
  std::vector<double> cand;
  for (int k = 0; k < nl; k++) {
    const double *q = &rec[(size_t)(edges ? edges[k] : k) * L];
    const double kappa = q[2 + d * d + d], tau = q[2 + d * d + d + 1];
    if (!(kappa > 0) || !(tau > 0)) {
      out.unweighted++;
      continue;
    }
    int i, j;
    bool inter;
    edge_head(q, i, j, inter);
    live.push_back(k);
    prow.push_back(i);
    prow.push_back(j);
    pairs.push_back(c.gid[i]);
    pairs.push_back(c.gid[j]);
    cand.insert(cand.end(), q + 2, q + 2 + NC);
  }
  const int nu = (int)live.size();
  // ---- the two predictions and the refusal: either method's parts, with this call's buffers ----
  if (cov_analyse(out) != 0) return -1;
  CovState &s = *cov_;
  const PairsPlan pl = pairs_plan(dof, anchor, pairs.data(), nu);
  const long long n = (long long)dof * N;
  const long long selinv = s.selinv_bytes, solve = (long long)spd_msolve_bytes(s.F, pl.kb);
  const long long common = 8ll * nu * (4 * DD + NC + NG + W) + 4ll * 2 * nu;
  const long long own_selinv = common + 8ll * 3 * nu + 4ll * NL * nu;
  const long long own_solve = common + 8ll * n * pl.kb + 4ll * (2ll * nu + pl.columns);
  out.columns = pl.columns;
  out.batches = pl.batches;
  out.device_bytes_selinv = s.numeric_bytes + selinv + own_selinv;
  out.device_bytes_solve = s.numeric_bytes + solve + own_solve;
  // SELINV: the blocks of the selected inversion are still to allocate where no earlier call has left them; SOLVE: the block
  // solve's buffers whether an earlier call has left them or not (pairs_setup)
  auto reserve = [&](int meth) {
    if (meth == RELY_SELINV)
      return hess_reserve(max_bytes, "edge_reliability",
                          {s.numeric_part(), {selinv, spd_selinv_values(s.F) ? 0 : selinv}, {own_selinv, own_selinv}}, out);
    return hess_reserve(max_bytes, "edge_reliability", {s.numeric_part(), {solve, solve}, {own_solve, own_solve}}, out);
  };
  // AUTO: SELINV where it is not refused, SOLVE where that is not; both refused: the smaller prediction is reported
  int use = method == RELY_AUTO ? RELY_SELINV : method, ready = reserve(use);
  if (method == RELY_AUTO && ready == 1) {
    use = RELY_SOLVE;
    ready = reserve(use);
    if (ready == 1) use = out.device_bytes_selinv <= out.device_bytes_solve ? RELY_SELINV : RELY_SOLVE;
  }
  if (ready < 0) return -1;
  out.method_used = ready != 0 ? method : use;
  out.device_bytes = use == RELY_SELINV ? out.device_bytes_selinv : out.device_bytes_solve;
  cert_prepare(X, ld, &out.stationarity);
  if (ready != 0) return 0;   // SKIPPED, with what the analysis and the sizes predict
  std::fill(rec_out, rec_out + (size_t)nl * W, 0.0);
  if (rel) std::fill(rel, rel + (size_t)nl * DD, 0.0);
  if (joint) std::fill(joint, joint + (size_t)nl * 3 * DD, 0.0);
  const int arow = own_row(anchor);
  typedef std::chrono::steady_clock Clock;
  auto ms_since = [](Clock::time_point t) { return 1e3 * std::chrono::duration<double>(Clock::now() - t).count(); };
  const int rc = hess_factor("edge_reliability", [&] { launch_cov_hessian_at(arow); }, out);
  if (rc < 0) return -1;
  if (rc != 0) {
    out.outcome = RELY_NOT_PD;
    return 0;
  }
  for (int k = 0, i = 0; k < nl; k++) {   // the records that never reach the device
    if (i < nu && live[i] == k) i++;
    else rec_out[(size_t)k * W + 1] = (double)RELY_FLAG_UNWEIGHTED;
  }
  if (nu > 0) {
    auto t0 = Clock::now();
    DevBuf<int> d_prow;
    DevBuf<double> d_joint, d_rel, d_gate, d_cand, d_rec;
    d_prow.upload(prow);
    d_cand.upload(cand);
    d_joint.alloc((size_t)nu * 3 * DD);   // (zeroed: the anchor's blocks under SOLVE)
    d_rel.alloc((size_t)nu * DD, false);
    d_gate.alloc((size_t)nu * NG, false);
    d_rec.alloc((size_t)nu * W, false);
    if (rely_joint(use, pl, nu, prow, arow, d_prow.p, d_joint.p, "edge_reliability") != 0) return -1;
    out.inverse_ms = ms_since(t0);
    t0 = Clock::now();
    launch_pairs_gate(d, st_, nu, d_prow.p, d_joint.p, c.X.p, d_cand.p, d_rel.p, d_gate.p);
    launch_rely_edge(d, st_, nu, d_rel.p, d_gate.p + 2, NG, d_cand.p + d * d + d, NC, d_rec.p);
    HIP_CHECK(hipGetLastError());
    std::vector<double> h_rec((size_t)nu * W), h_rel(rel ? (size_t)nu * DD : 0), h_joint(joint ? (size_t)nu * 3 * DD : 0);
    HIP_CHECK(hipMemcpyAsync(h_rec.data(), d_rec.p, sizeof(double) * h_rec.size(), hipMemcpyDeviceToHost, st_));
    if (rel) HIP_CHECK(hipMemcpyAsync(h_rel.data(), d_rel.p, sizeof(double) * h_rel.size(), hipMemcpyDeviceToHost, st_));
    if (joint) HIP_CHECK(hipMemcpyAsync(h_joint.data(), d_joint.p, sizeof(double) * h_joint.size(), hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
    for (int i = 0; i < nu; i++) {
      const size_t k = (size_t)live[i];
      std::copy(h_rec.begin() + (size_t)i * W, h_rec.begin() + (size_t)(i + 1) * W, rec_out + k * W);
      if (rel) std::copy(h_rel.begin() + (size_t)i * DD, h_rel.begin() + (size_t)(i + 1) * DD, rel + k * DD);
      if (joint) std::copy(h_joint.begin() + (size_t)i * 3 * DD, h_joint.begin() + (size_t)(i + 1) * 3 * DD, joint + k * 3 * DD);
    }
    out.edge_ms = ms_since(t0);
  }
  for (int k = 0; k < nl; k++) {   // list order, flag-2 edges left out
    const double flag = rec_out[(size_t)k * W + 1];
    if (flag == (double)RELY_FLAG_UNWEIGHTED) continue;
    if (flag == (double)RELY_FLAG_NOT_PD) out.flagged++;
    out.redundancy_sum += rec_out[(size_t)k * W + 2];
  }
  out.outcome = RELY_OK;
  return 0;
}

// ---- host only: rely_one of n edges through rely_math.h ----
int rely_edge_host(int d, int n, const double *rel, const double *r, const double *kappa, const double *tau, double *rec) {
  if ((d != 2 && d != 3) || n < 0 || (n > 0 && (!rel || !r || !kappa || !tau || !rec))) return -1;
  const int dof = cov_dof(d), DD = dof * dof, W = rely_width(d);
  for (int k = 0; k < n; k++) {
    if (d == 3) rely_one<3>(rel + (size_t)k * DD, r + (size_t)k * dof, kappa[k], tau[k], rec + (size_t)k * W);
    else rely_one<2>(rel + (size_t)k * DD, r + (size_t)k * dof, kappa[k], tau[k], rec + (size_t)k * W);
  }
  return 0;
}

// ---- k_rely_edge alone on the caller's arrays (host pointers), on the current device's null stream ----
int rely_edge_device(int d, int n, const double *rel, const double *r, const double *kappa, const double *tau, double *rec) {
  if ((d != 2 && d != 3) || n < 1 || !rel || !r || !kappa || !tau || !rec) return -1;
  const int dof = cov_dof(d), DD = dof * dof, W = rely_width(d);
  std::vector<double> kt((size_t)2 * n);
  for (int k = 0; k < n; k++) {
    kt[(size_t)2 * k] = kappa[k];
    kt[(size_t)2 * k + 1] = tau[k];
  }
  DevBuf<double> d_rel, d_r, d_kt, d_rec;
  d_rel.upload(std::vector<double>(rel, rel + (size_t)n * DD));
  d_r.upload(std::vector<double>(r, r + (size_t)n * dof));
  d_kt.upload(kt);
  d_rec.alloc((size_t)n * W);
  launch_rely_edge(d, nullptr, n, d_rel.p, d_r.p, dof, d_kt.p, 2, d_rec.p);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpy(rec, d_rec.p, sizeof(double) * (size_t)n * W, hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace dpgo
