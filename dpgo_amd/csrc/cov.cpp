// Host side of the marginal pose covariances (cov.h): the pattern of the tangent-space Hessian from the certificate's walk,
// its multifrontal analysis, the parts of its refusal, and the calls that write H on the device (k_cov_hessian), factor it
// (hess.cpp: hess_factor) and invert it inside the factor's pattern (spd_selinv_device).  The optimiser's state is not
// touched: own factor, own buffers, behind finish_update() / join_exchange() (cert_begin), released in the group's teardown.
#include "cov.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <numeric>

#include "cert_state.h"
#include "cov_state.h"
#include "group.h"

namespace dpgo {

void Group::cov_release() {
  delete cov_;
  cov_ = nullptr;
}

int Group::cov_begin(const double *X, int ld, int anchor) {
  if (cert_begin(X, ld) != 0) return -1;   // (the arguments, the trivial loss, every node hosted; the optimiser's pending work taken)
  if (anchor < 0 || anchor >= num_poses_global_) {
    fprintf(stderr, "[dpgo_amd] ERROR: covariance: the anchor %d is no pose of the graph.\n", anchor);
    return -1;
  }
  if (!cov_) cov_ = new CovState();
  return 0;
}

// The analysis (first call) and its numbers: the pattern of H from the certificate's, its multifrontal analysis.  device_bytes is
// the caller's refusal's to fill (hess_reserve).
int Group::cov_analyse(HessAnalysis &out) {
  CertState &c = *cert_;
  CovState &s = *cov_;
  cert_build_pattern();
  const int B = B_, BB = B * B, dof = cov_dof(d_), DD = dof * dof, N = P0_;
  if (!s.have_symbolic) {
    const auto t0 = std::chrono::steady_clock::now();
    const size_t nblk = c.bptr_h[N], nnz = nblk * DD;
    if (nnz > (size_t)0x7fffffff) throw DeviceError("covariance: the matrix has more than 2^31 entries");
    s.bcol_h.resize(nblk);
    s.A.n = dof * N;
    s.A.ptr.assign((size_t)dof * N + 1, 0);
    s.A.col.resize(nnz);
    for (int p = 0; p < N; p++) {
      const int b0 = c.bptr_h[p], nb = c.bptr_h[p + 1] - b0;
      const size_t base = (size_t)DD * b0;
      for (int j = 0; j < nb; j++) s.bcol_h[b0 + j] = c.A.col[(size_t)BB * b0 + (size_t)j * B] / B;
      for (int r = 0; r < dof; r++) {
        s.A.ptr[(size_t)dof * p + r + 1] = (int)(base + (size_t)(r + 1) * dof * nb);
        for (int j = 0; j < nb; j++)
          for (int cc = 0; cc < dof; cc++) s.A.col[base + (size_t)r * dof * nb + (size_t)j * dof + cc] = dof * s.bcol_h[b0 + j] + cc;
      }
    }
    // collapse = 1 and leaves of 16 poses, as the certificate's factor (more where that many leaves would not fit the
    // 65535 fronts a level's launch can index)
    const long long n = s.A.n;
    const int leaf = (int)std::max<long long>(16 * dof, dof * ((2 * n / dof + 59999) / 60000));
    s.F.quiet = true;   // a non-positive pivot is a verdict here
    if (spd_symbolic(s.A, s.F, leaf, 1, dof) != 0) {
      fprintf(stderr, "[dpgo_amd] ERROR: covariance: the symbolic analysis of the Hessian failed.\n");
      return -1;
    }
    s.piv_front.assign(s.A.n, -1);
    s.piv_loc.assign(s.A.n, -1);
    for (int f = 0; f < s.F.nfronts; f++)
      for (int k = 0; k < s.F.w[f]; k++) {
        s.piv_front[s.F.piv_idx[s.F.piv_ptr[f] + k]] = f;
        s.piv_loc[s.F.piv_idx[s.F.piv_ptr[f] + k]] = k;
      }
    s.numeric_bytes = (long long)spd_numeric_bytes(s.F, (long long)s.A.col.size()) + 4ll * (long long)nblk;
    s.selinv_bytes = (long long)spd_selinv_bytes(s.F);
    s.symbolic_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    out.symbolic_s = s.symbolic_s;
    s.have_symbolic = true;
  }
  out.unknowns = s.A.n;
  out.fronts = s.F.nfronts;
  out.levels = (int)s.F.by_height.size();
  out.max_front = s.F.max_front;
  return 0;
}

// The analysis and the refusal of covariance, robust_covariance and the two read-backs: the numeric phase, the blocks of the
// selected inversion -- still to allocate only where the numeric phase is, whether an earlier call has left them or not -- and the
// caller's extra bytes (robust.cpp).
int Group::cov_setup(long long max_bytes, CovResult &out, HessPart extra) {
  if (cov_analyse(out) != 0) return -1;
  CovState &s = *cov_;
  for (int f = 0; f < s.F.nfronts; f++) {
    const double w = s.F.w[f], u = s.F.u[f];
    out.selinv_flops += 2 * u * u * w + 2 * u * w * w + w * w * w;
  }
  return hess_reserve(max_bytes, "covariance", {s.numeric_part(), {s.selinv_bytes, s.F.numeric ? 0 : s.selinv_bytes}, extra}, out);
}

bool Group::pairs_args_ok(const char *who, const int *pairs, int npairs) const {
  for (int k = 0; k < 2 * npairs; k++)
    if (pairs[k] < 0 || pairs[k] >= P0_) {
      fprintf(stderr, "[dpgo_amd] ERROR: %s: pair %d names a pose that is not in the graph.\n", who, k / 2);
      return false;
    }
  return true;
}

// edges lie inside the selected pattern; anything else does not
bool Group::pairs_are_edges(const char *who, const int *pairs, int npairs) const {
  for (int k = 0; k < npairs; k++)
    if (cert_block_of(own_row(pairs[2 * k]), own_row(pairs[2 * k + 1])) < 0) {
      fprintf(stderr, "[dpgo_amd] ERROR: %s: pair %d (%d, %d) is not an edge of the graph.\n", who, k, pairs[2 * k], pairs[2 * k + 1]);
      return false;
    }
  return true;
}

int Group::covariance(const double *X, int ld, int anchor, long long max_bytes, const int *pairs, int npairs, double *marginals,
                      double *cross, CovResult &out) {
  out = CovResult();
  if (!marginals || npairs < 0 || (npairs > 0 && (!pairs || !cross))) {
    fprintf(stderr, "[dpgo_amd] ERROR: covariance: missing output or pair arrays.\n");
    return -1;
  }
  if (cov_begin(X, ld, anchor) != 0) return -1;
  if (!pairs_args_ok("covariance", pairs, npairs)) return -1;
  const int ready = cov_setup(max_bytes, out);
  if (ready < 0 || !pairs_are_edges("covariance", pairs, npairs)) return -1;
  cert_prepare(X, ld, &out.stationarity);
  if (ready != 0) return 0;   // SKIPPED, with what the analysis predicts
  return cov_finish([&] { launch_cov_hessian_at(own_row(anchor)); }, own_row(anchor), pairs, npairs, marginals, cross, out);
}

// k_cov_hessian on the certificate's M, Lambda and X into the factorisation's values
void Group::launch_cov_hessian_at(int arow) {
  CertState &c = *cert_;
  CovState &s = *cov_;
  launch_cov_hessian(d_, st_, P0_, c.bptr.p, s.bcol.p, c.Mval.p, c.Lam.p, c.X.p, arow, spd_numeric_values(s.F));
}

int Group::cov_finish(const std::function<void()> &write_H, int arow, const int *pairs, int npairs, double *marginals, double *cross,
                      CovResult &out) {
  CertState &c = *cert_;
  CovState &s = *cov_;
  const int dof = cov_dof(d_), DD = dof * dof, N = P0_;
  const std::vector<int> &row_of = c.row_of;
  std::fill(marginals, marginals + (size_t)N * DD, 0.0);
  if (npairs) std::fill(cross, cross + (size_t)npairs * DD, 0.0);
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = hess_factor("covariance", write_H, out);
  if (rc < 0) return -1;
  if (rc != 0) {
    out.numeric_ms = 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    out.outcome = COV_NOT_PD;
    return 0;
  }
  if (spd_selinv_device(s.F, st_) != 0) {
    fprintf(stderr, "[dpgo_amd] ERROR: covariance: the selected inversion failed on the device.\n");
    return -1;
  }
  HIP_CHECK(hipStreamSynchronize(st_));
  out.numeric_ms = 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  out.selinv_ms = out.numeric_ms - out.factor_ms;
  // the blocks to the host, then read out: a pose's dof unknowns are pivots of one front (the ordering is computed on the
  // quotient graph), so its marginal is a block of that front's S_pp; the block of an edge lies in the front of whichever
  // pose is eliminated first, whose update rows hold the other
  const std::vector<int64_t> off = spd_selinv_offsets(s.F);
  std::vector<double> Sig(off.back());
  if (!Sig.empty()) HIP_CHECK(hipMemcpy(Sig.data(), spd_selinv_values(s.F), sizeof(double) * Sig.size(), hipMemcpyDeviceToHost));
  const SpdFactor &F = s.F;
  for (int p = 0; p < N; p++) {
    if (p == arow) continue;
    const int f = s.piv_front[dof * p], m = F.w[f] + F.u[f];
    double *out_b = marginals + (size_t)c.gid[p] * DD;
    for (int a = 0; a < dof; a++)
      for (int b = 0; b < dof; b++) {
        if (s.piv_front[dof * p + a] != f || s.piv_front[dof * p + b] != f) {
          fprintf(stderr, "[dpgo_amd] ERROR: covariance: the unknowns of a pose are spread over two fronts.\n");
          return -1;
        }
        out_b[a * dof + b] = Sig[off[f] + (int64_t)s.piv_loc[dof * p + a] * m + s.piv_loc[dof * p + b]];
      }
  }
  // pairs by the front that holds them (one map of its update rows per front)
  std::vector<int> order(npairs), loc(s.A.n, -1);
  std::iota(order.begin(), order.end(), 0);
  auto first_front = [&](int k) {
    return std::min(s.piv_front[dof * row_of[pairs[2 * k]]], s.piv_front[dof * row_of[pairs[2 * k + 1]]]);
  };
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return first_front(x) < first_front(y); });
  for (size_t i = 0; i < order.size();) {
    const int f = first_front(order[i]), w = F.w[f], u = F.u[f], m = w + u;
    const int *up = u ? &F.upd_idx[F.upd_ptr[f]] : nullptr;
    for (int k = 0; k < u; k++) loc[up[k]] = w + k;
    for (; i < order.size() && first_front(order[i]) == f; i++) {
      const int k = order[i];
      int p = row_of[pairs[2 * k]], q = row_of[pairs[2 * k + 1]];
      if (p == arow || q == arow) continue;
      const bool swapped = s.piv_front[dof * p] != f;   // q is the one this front eliminates: read S_qp, hand out its transpose
      if (swapped) std::swap(p, q);
      for (int a = 0; a < dof; a++)
        for (int b = 0; b < dof; b++) {
          const int vq = dof * q + b;
          const int lq = s.piv_front[vq] == f ? s.piv_loc[vq] : loc[vq];
          if (lq < 0) {
            fprintf(stderr, "[dpgo_amd] ERROR: covariance: pair %d lies outside the factor's pattern.\n", k);
            return -1;
          }
          const double v = Sig[off[f] + (int64_t)s.piv_loc[dof * p + a] * m + lq];
          cross[(size_t)k * DD + (swapped ? b * dof + a : a * dof + b)] = v;
        }
    }
    for (int k = 0; k < u; k++) loc[up[k]] = -1;
  }
  out.outcome = COV_OK;
  return 0;
}

int Group::cov_hessian(const double *X, int ld, int anchor, int *ptr, int *col, double *val, long long cap, long long *nnz) {
  if (!nnz || cov_begin(X, ld, anchor) != 0) return -1;
  CovState &s = *cov_;
  CovResult r;
  const int ready = cov_setup(0, r);
  if (ready < 0) return -1;
  *nnz = (long long)s.A.col.size();
  if (!ptr && !col && !val) return 0;   // (the size alone)
  if (!ptr || !col || !val || cap < *nnz) {
    fprintf(stderr, "[dpgo_amd] ERROR: covariance: cov_hessian needs room for %lld entries.\n", *nnz);
    return -1;
  }
  if (ready != 0) {
    fprintf(stderr, "[dpgo_amd] ERROR: covariance: the value array of the factorisation does not fit the device.\n");
    return -1;
  }
  cert_prepare(X, ld, nullptr);
  launch_cov_hessian_at(own_row(anchor));
  std::vector<double> v(s.A.col.size());
  HIP_CHECK(hipMemcpyAsync(v.data(), spd_numeric_values(s.F), sizeof(double) * v.size(), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
  cov_csr_out(v, ptr, col, val);
  return 0;
}

// handed out on GLOBAL poses -- unknown dof g + a, g = gid[p] -- rows in that order, a row's blocks by ascending pose
void Group::cov_csr_out(const std::vector<double> &v, int *ptr, int *col, double *val) {
  CertState &c = *cert_;
  CovState &s = *cov_;
  const int dof = cov_dof(d_), DD = dof * dof, N = P0_;
  std::vector<int> order;
  size_t e = 0;
  ptr[0] = 0;
  for (int g = 0; g < N; g++) {
    const int p = own_row(g), b0 = c.bptr_h[p], nb = c.bptr_h[p + 1] - b0;
    const size_t base = (size_t)DD * b0;
    auto pose_of = [&](int j) { return c.gid[s.bcol_h[b0 + j]]; };
    order.resize(nb);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int x, int y) { return pose_of(x) < pose_of(y); });
    for (int r = 0; r < dof; r++) {
      for (int j : order)
        for (int cc = 0; cc < dof; cc++, e++) {
          col[e] = dof * pose_of(j) + cc;
          val[e] = v[base + (size_t)r * dof * nb + (size_t)j * dof + cc];
        }
      ptr[(size_t)dof * g + r + 1] = (int)e;
    }
  }
}

}  // namespace dpgo
