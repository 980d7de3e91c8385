// Host side of the edge reliability and the candidate gate on the full information matrices (ml_rely.h): ml_begin and the ML
// edge pass, the two predictions and the refusal with the ML buffers as a part of their own, H written by k_ml_hessian and
// factored (hess.cpp: hess_factor), the three blocks of every listed edge (rely.cpp: rely_joint) or pair (pairs.cpp:
// pairs_solve_joint), then k_ml_rel and k_ml_rely_edge.  The optimiser's state is not touched (cert_begin).
#include "ml_rely.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

#include "cert_state.h"
#include "cov_state.h"
#include "edge_math.h"
#include "edges.h"
#include "group.h"
#include "ml_rely_math.h"
#include "ml_state.h"

namespace dpgo {

// |g_ml| at X: the full edge pass at CertState's X (which stays there: r and the stored records of every edge) and the gather
double Group::ml_stationarity(const double *X, int ld, int arow) {
  CertState &c = *cert_;
  cert_upload(X, ld, d_, c.X.p);
  ml_point(arow, ml_->grad.p, 0, -1);
  launch_polish_reduce(st_, T_, 1, 0u, c.partials.p, c.h_sums, sched_.flag());
  wait_flag(sched_.last_seq());
  return std::sqrt(c.h_sums[0]);
}

int Group::ml_edge_reliability(const Graph &g, const double *X, int ld, int anchor, long long max_bytes, int method, const int *edges,
                               int nedges, double *rec_out, double *rel, double *joint, RelyResult &out) {
  const char *who = "ml_edge_reliability";
  out = RelyResult();
  if (!rec_out || (edges && nedges < 0)) {
    fprintf(stderr, "[dpgo_amd] ERROR: %s: missing output array, or a negative number of edges.\n", who);
    return -1;
  }
  if (method != RELY_AUTO && method != RELY_SELINV && method != RELY_SOLVE) {
    fprintf(stderr, "[dpgo_amd] ERROR: %s: method %d is none of AUTO, SELINV, SOLVE.\n", who, method);
    return -1;
  }
  if (ml_begin(g, X, ld, anchor, who) != 0) return -1;
  CertState &c = *cert_;
  const int d = d_, dof = cov_dof(d), DD = dof * dof, N = P0_, m = (int)g.all.size(), L = edge_rec_doubles(d);
  const int W = rely_width(d), NL = rely_map_ints(dof);
  const int nl = edges ? nedges : m;
  // the listed edges: their index in the graph, the unified own rows of their poses, the poses
  std::vector<int> idx((size_t)nl), prow, pairs;
  for (int k = 0; k < nl; k++) {
    const int e = edges ? edges[k] : k;
    if (e < 0 || e >= m) {
      fprintf(stderr, "[dpgo_amd] ERROR: %s: entry %d of the list names edge %d of %d.\n", who, k, e, m);
      return -1;
    }
    int i, j;
    bool inter;
    edge_head(&ml_->plan.rec[(size_t)e * L], i, j, inter);
    idx[k] = e;
    prow.push_back(i);
    prow.push_back(j);
    pairs.push_back(c.gid[i]);
    pairs.push_back(c.gid[j]);
  }
  out.edges = nl;
  // ---- the two predictions and the refusal: either method's parts, this call's buffers, the ML buffers ----
  if (cov_analyse(out) != 0) return -1;
  CovState &s = *cov_;
  const PairsPlan pl = pairs_plan(dof, anchor, pairs.data(), nl);
  const long long n = (long long)dof * N;
  const long long selinv = s.selinv_bytes, solve = (long long)spd_msolve_bytes(s.F, pl.kb);
  const long long common = 8ll * nl * (4 * DD + W) + 4ll * 3 * nl;   // joint, rel, the records; the rows and the indices
  const long long own_selinv = common + 8ll * 3 * nl + 4ll * NL * nl;
  const long long own_solve = common + 8ll * n * pl.kb + 4ll * (2ll * nl + pl.columns);
  out.columns = pl.columns;
  out.batches = pl.batches;
  out.device_bytes_selinv = s.numeric_bytes + selinv + own_selinv + ml_->bytes;
  out.device_bytes_solve = s.numeric_bytes + solve + own_solve + ml_->bytes;
  auto reserve = [&](int meth) {
    const HessPart ml{ml_->bytes, ml_remain()};
    if (meth == RELY_SELINV)
      return hess_reserve(max_bytes, who, {s.numeric_part(), {selinv, spd_selinv_values(s.F) ? 0 : selinv}, {own_selinv, own_selinv}, ml},
                          out);
    return hess_reserve(max_bytes, who, {s.numeric_part(), {solve, solve}, {own_solve, own_solve}, ml}, out);
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
  if (ready != 0) return 0;   // SKIPPED: nothing allocated, the stationarity not computed
  ml_alloc();
  MlState &ml = *ml_;
  const int arow = own_row(anchor);
  out.stationarity = ml_stationarity(X, ld, arow);
  std::fill(rec_out, rec_out + (size_t)nl * W, 0.0);
  if (rel) std::fill(rel, rel + (size_t)nl * DD, 0.0);
  if (joint) std::fill(joint, joint + (size_t)nl * 3 * DD, 0.0);
  typedef std::chrono::steady_clock Clock;
  auto ms_since = [](Clock::time_point t) { return 1e3 * std::chrono::duration<double>(Clock::now() - t).count(); };
  const int rc = hess_factor(who, [&] { ml_hessian_launch(arow); }, out);
  if (rc < 0) return -1;
  if (rc != 0) {
    out.outcome = RELY_NOT_PD;
    return 0;
  }
  if (nl > 0) {
    auto t0 = Clock::now();
    DevBuf<int> d_prow, d_idx;
    DevBuf<double> d_joint, d_rel, d_rec;
    d_prow.upload(prow);
    d_idx.upload(idx);
    d_joint.alloc((size_t)nl * 3 * DD);   // (zeroed: the anchor's blocks under SOLVE)
    d_rel.alloc((size_t)nl * DD, false);
    d_rec.alloc((size_t)nl * W, false);
    if (rely_joint(use, pl, nl, prow, arow, d_prow.p, d_joint.p, who) != 0) return -1;
    out.inverse_ms = ms_since(t0);
    t0 = Clock::now();
    launch_ml_rel(d, st_, nl, d_idx.p, ml.jw.p, ml_jw_doubles(d), d_joint.p, d_rel.p);
    launch_ml_rely_edge(d, -1, st_, nl, d_idx.p, d_rel.p, ml.om.p, ml.r.p, d_rec.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(rec_out, d_rec.p, sizeof(double) * (size_t)nl * W, hipMemcpyDeviceToHost, st_));
    if (rel) HIP_CHECK(hipMemcpyAsync(rel, d_rel.p, sizeof(double) * (size_t)nl * DD, hipMemcpyDeviceToHost, st_));
    if (joint) HIP_CHECK(hipMemcpyAsync(joint, d_joint.p, sizeof(double) * (size_t)nl * 3 * DD, hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
    out.edge_ms = ms_since(t0);
  }
  for (int k = 0; k < nl; k++) {   // list order
    if (rec_out[(size_t)k * W + 1] == (double)RELY_FLAG_NOT_PD) out.flagged++;
    out.redundancy_sum += rec_out[(size_t)k * W + 2];
  }
  out.outcome = RELY_OK;
  return 0;
}

int Group::ml_pair_gate(const Graph &g, const double *X, int ld, int anchor, long long max_bytes, const int *pairs, int npairs,
                        const double *cand_R, const double *cand_t, const double *cand_info, double *joint, double *rel, double *gate,
                        PairsResult &out) {
  const char *who = "ml_pair_gate";
  out = PairsResult();
  if (npairs < 0 || (npairs > 0 && (!pairs || !cand_R || !cand_t || !cand_info || !joint || !rel || !gate))) {
    fprintf(stderr, "[dpgo_amd] ERROR: %s: missing pair, candidate or output arrays.\n", who);
    return -1;
  }
  if (ml_begin(g, X, ld, anchor, who) != 0) return -1;
  CertState &c = *cert_;
  CovState &s = *cov_;
  const int d = d_, dof = cov_dof(d), DD = dof * dof, N = P0_, L = edge_rec_doubles(d), NG = 2 + dof, JW = ml_jw_doubles(d);
  if (!pairs_args_ok(who, pairs, npairs)) return -1;
  for (int k = 0; k < npairs; k++) {
    bool finite = true;
    for (int a = 0; a < d * d; a++) finite = finite && std::isfinite(cand_R[(size_t)k * d * d + a]);
    for (int a = 0; a < d; a++) finite = finite && std::isfinite(cand_t[(size_t)k * d + a]);
    const std::vector<double> one(cand_info + (size_t)k * DD, cand_info + (size_t)(k + 1) * DD);
    if (!finite || ml_check_information(d, one, who) != 0) {
      fprintf(stderr, "[dpgo_amd] ERROR: %s: candidate %d has a measurement that is not finite, or an information matrix that is not "
                      "symmetric positive definite.\n", who, k);
      return -1;
    }
  }
  const PairsPlan pl = pairs_plan(dof, anchor, pairs, npairs);
  out.columns = pl.columns;
  out.batches = pl.batches;
  const long long n = (long long)dof * N, nb = (npairs + EDGE_BLOCK - 1) / EDGE_BLOCK;
  // the batch, joint, rel, the gate; the candidates' records, Omega and what the edge pass writes of them; the plan's lists
  const long long own = 8ll * (n * pl.kb + (long long)npairs * (4 * DD + NG + L + DD + 2 * dof + 1 + 2 * dof + JW)) +
                        8ll * 2 * nb + (long long)sizeof(MlSummaryDev) + 4ll * (4ll * npairs + pl.columns);
  if (cov_analyse(out) != 0) return -1;
  const long long solve = (long long)spd_msolve_bytes(s.F, pl.kb);
  const int ready = hess_reserve(max_bytes, who, {s.numeric_part(), {solve, solve}, {own, own}, {ml_->bytes, ml_remain()}}, out);
  if (ready < 0) return -1;
  for (int b = 0; b < pl.batches; b++) {
    const int nc = std::min(PAIRS_BATCH, pl.columns - b * PAIRS_BATCH);
    out.solve_flops += 4.0 * (double)s.F.entries * (16 * ((nc + 15) / 16));
    out.factor_bytes += 16.0 * (double)s.F.entries;
  }
  if (ready != 0) return 0;   // SKIPPED: nothing allocated, the stationarity not computed
  ml_alloc();
  const int arow = own_row(anchor);
  out.stationarity = ml_stationarity(X, ld, arow);
  std::fill(joint, joint + (size_t)npairs * 3 * DD, 0.0);
  std::fill(rel, rel + (size_t)npairs * DD, 0.0);
  std::fill(gate, gate + (size_t)npairs * NG, 0.0);
  typedef std::chrono::steady_clock Clock;
  auto ms_since = [](Clock::time_point t) { return 1e3 * std::chrono::duration<double>(Clock::now() - t).count(); };
  const int rc = hess_factor(who, [&] { ml_hessian_launch(arow); }, out);
  if (rc < 0) return -1;
  out.outcome = rc != 0 ? PAIRS_NOT_PD : PAIRS_OK;
  if (rc != 0 || npairs == 0) return 0;
  auto t0 = Clock::now();
  // the candidates as edge records of their own, heads on unified own rows: k_ml_edge<FULL> computes their r and J as it
  // computes an edge's, so a candidate that copies an edge of the graph has that edge's bits
  std::vector<int> prow((size_t)2 * npairs);
  std::vector<double> crec((size_t)npairs * L, 0.0);
  for (int k = 0; k < npairs; k++) {
    prow[2 * k] = own_row(pairs[2 * k]);
    prow[2 * k + 1] = own_row(pairs[2 * k + 1]);
    double *q = &crec[(size_t)k * L];
    const int head[4] = {prow[2 * k], prow[2 * k + 1], 0, 0};
    std::memcpy(q, head, sizeof(head));
    std::copy(cand_R + (size_t)k * d * d, cand_R + (size_t)(k + 1) * d * d, q + 2);
    std::copy(cand_t + (size_t)k * d, cand_t + (size_t)(k + 1) * d, q + 2 + d * d);
    q[2 + d * d + d] = q[2 + d * d + d + 1] = 1.0;   // (kappa, tau: not read by the ML edge pass)
  }
  DevBuf<int> d_prow;
  DevBuf<double> d_joint, d_rel, d_gate, d_crec, d_om, d_r, d_wr, d_chi2, d_ge, d_jw, d_part, d_sum;
  DevBuf<int64_t> d_cnt;
  d_prow.upload(prow);
  d_crec.upload(crec);
  d_om.upload(std::vector<double>(cand_info, cand_info + (size_t)npairs * DD));
  d_joint.alloc((size_t)npairs * 3 * DD);   // (zeroed: the anchor's blocks)
  d_rel.alloc((size_t)npairs * DD);
  d_gate.alloc((size_t)npairs * NG);
  d_r.alloc((size_t)npairs * dof);
  d_wr.alloc((size_t)npairs * dof);
  d_chi2.alloc((size_t)npairs);
  d_ge.alloc((size_t)2 * npairs * dof);
  d_jw.alloc((size_t)npairs * JW);
  d_part.alloc((size_t)nb);
  d_cnt.alloc((size_t)nb);
  d_sum.alloc(sizeof(MlSummaryDev) / sizeof(double));
  if (pairs_solve_joint(pl, npairs, d_prow.p, d_joint.p, who) != 0) return -1;
  out.solve_ms = ms_since(t0);
  t0 = Clock::now();
  launch_ml_edge(d, st_, npairs, d_crec.p, d_om.p, c.X.p, MlEdgeOut{d_r.p, d_wr.p, d_chi2.p, d_ge.p, d_jw.p}, d_part.p,
                 reinterpret_cast<long long *>(d_cnt.p), reinterpret_cast<MlSummaryDev *>(d_sum.p), nullptr, 0);
  launch_ml_rel(d, st_, npairs, nullptr, d_jw.p, JW, d_joint.p, d_rel.p);
  launch_ml_rely_edge(d, 1, st_, npairs, nullptr, d_rel.p, d_om.p, d_r.p, d_gate.p);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(joint, d_joint.p, sizeof(double) * (size_t)npairs * 3 * DD, hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipMemcpyAsync(rel, d_rel.p, sizeof(double) * (size_t)npairs * DD, hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipMemcpyAsync(gate, d_gate.p, sizeof(double) * (size_t)npairs * NG, hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
  out.gate_ms = ms_since(t0);
  return 0;
}

// ---- host only: ml_rel_entry and ml_rely_one of n edges through ml_rely_math.h ----
static bool ml_rely_args_ok(int d, int n, int sign, const double *J, const double *joint, const double *Om, const double *r,
                            const double *rel, const double *rec) {
  if ((d != 2 && d != 3) || (sign != 1 && sign != -1) || n < 0) return false;
  if (n > 0 && (!J || !joint || !Om || !r || !rel || !rec)) return false;
  const int DD = cov_dof(d) * cov_dof(d);
  return n == 0 || ml_check_information(d, std::vector<double>(Om, Om + (size_t)n * DD), "ml_rely_edge debug") == 0;
}

template <int D>
static void ml_rely_host_d(int n, int sign, const double *J, const double *joint, const double *Om, const double *r, double *rel,
                           double *rec) {
  constexpr int DOF = cov_dof(D), DD = DOF * DOF;
  const int W = sign < 0 ? RelyDims<D>::WIDTH : MlGateDims<D>::WIDTH;
  for (int k = 0; k < n; k++) {
    const double *Jp = J + (size_t)k * 2 * DD;
    double *rl = rel + (size_t)k * DD;
    for (int a = 0; a < DOF; a++)
      for (int b = 0; b <= a; b++) rl[a * DOF + b] = rl[b * DOF + a] = ml_rel_entry<D>(Jp, Jp + DD, joint + (size_t)k * 3 * DD, a, b);
    if (sign < 0) ml_rely_one<D, -1>(rl, Om + (size_t)k * DD, r + (size_t)k * DOF, rec + (size_t)k * W);
    else ml_rely_one<D, 1>(rl, Om + (size_t)k * DD, r + (size_t)k * DOF, rec + (size_t)k * W);
  }
}

int ml_rely_edge_host(int d, int n, int sign, const double *J, const double *joint, const double *Om, const double *r, double *rel,
                      double *rec) {
  if (!ml_rely_args_ok(d, n, sign, J, joint, Om, r, rel, rec)) return -1;
  if (d == 3) ml_rely_host_d<3>(n, sign, J, joint, Om, r, rel, rec);
  else ml_rely_host_d<2>(n, sign, J, joint, Om, r, rel, rec);
  return 0;
}

// ---- k_ml_rel and k_ml_rely_edge alone on the caller's arrays (host pointers), on the current device's null stream ----
int ml_rely_edge_device(int d, int n, int sign, const double *J, const double *joint, const double *Om, const double *r, double *rel,
                        double *rec) {
  if (n < 1 || !ml_rely_args_ok(d, n, sign, J, joint, Om, r, rel, rec)) return -1;
  const int dof = cov_dof(d), DD = dof * dof, W = sign < 0 ? rely_width(d) : 2 + dof;
  DevBuf<double> d_J, d_joint, d_om, d_r, d_rel, d_rec;
  d_J.upload(std::vector<double>(J, J + (size_t)n * 2 * DD));
  d_joint.upload(std::vector<double>(joint, joint + (size_t)n * 3 * DD));
  d_om.upload(std::vector<double>(Om, Om + (size_t)n * DD));
  d_r.upload(std::vector<double>(r, r + (size_t)n * dof));
  d_rel.alloc((size_t)n * DD);
  d_rec.alloc((size_t)n * W);
  launch_ml_rel(d, nullptr, n, nullptr, d_J.p, 2 * DD, d_joint.p, d_rel.p);
  launch_ml_rely_edge(d, sign, nullptr, n, nullptr, d_rel.p, d_om.p, d_r.p, d_rec.p);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpy(rel, d_rel.p, sizeof(double) * (size_t)n * DD, hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(rec, d_rec.p, sizeof(double) * (size_t)n * W, hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace dpgo
