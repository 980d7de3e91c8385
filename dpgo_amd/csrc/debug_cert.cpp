// Test hooks for the certificate's LOBPCG search (group.h: debug_cert_gram, debug_cert_update, debug_cert_precon,
// debug_cert_trace).  Nothing here computes: each entry copies reference-layout inputs into CertState's buffers with
// cert_upload, makes the launch cert_search makes through the search's own launch_cert_* functions and launch_cert_reduce,
// and reads the results back with cert_download.
#include <cstring>

#include "cert_state.h"
#include "group.h"

namespace dpgo {

int Group::debug_cert_gram(const double *X, const double *V, const double *W, const double *P, const double *SV, const double *SP,
                           const double *MW, int ld, double *sums, double *SW) {
  if (!V || !W || !P || !SV || !SP || !sums || !SW || cert_begin(X, ld) != 0) return -1;
  CertState &c = *cert_;
  const NodeMask all{all_bits(), nullptr};
  const int nsums = cert_nsums(d_);
  cert_prepare(X, ld, nullptr);
  cert_upload(V, ld, d_, c.V.p);
  cert_upload(W, ld, d_, c.W.p);
  cert_upload(P, ld, d_, c.P.p);
  cert_upload(SV, ld, d_, c.SV.p, false);
  cert_upload(SP, ld, d_, c.SP.p, false);
  if (MW) cert_upload(MW, ld, d_, c.SW.p, false);
  else cert_apply_M(c.W.p, c.SW.p);
  launch_cert_gram(lc(all), c.Lam.p, c.V.p, c.W.p, c.P.p, c.SV.p, c.SW.p, c.SP.p, c.partials.p);
  launch_cert_reduce(st_, T_, nsums, c.partials.p, c.h_sums, sched_.flag());
  wait_flag(sched_.last_seq());
  std::copy(c.h_sums, c.h_sums + nsums, sums);
  cert_download(c.SW.p, SW, ld, d_);
  return 0;
}

int Group::debug_cert_update(const CertUpdateDebug &q) {
  const int d = d_, rows = (d + 1) * num_poses_global_;
  if (!q.C || !q.theta || !q.V || !q.W || !q.P || !q.SV || !q.SW || !q.SP || !q.sums || q.ld < rows) return -1;
  for (double *o : q.out)
    if (!o) return -1;
  if (P1_ > 0 && !q.nbr) return -1;
  if (cert_ready() != 0) return -1;
  CertState &c = *cert_;
  const NodeMask all{all_bits(), nullptr};
  const int nsums = cert_nsums(d);
  if (q.precondition) cert_build_precon();
  cert_upload(q.V, q.ld, d, c.V.p);
  cert_upload(q.W, q.ld, d, c.W.p);
  cert_upload(q.P, q.ld, d, c.P.p);
  cert_upload(q.SV, q.ld, d, c.SV.p, false);
  cert_upload(q.SW, q.ld, d, c.SW.p, false);
  cert_upload(q.SP, q.ld, d, c.SP.p, false);
  const size_t nnbr = (size_t)P1_ * RS_;
  double *const with_nbr[3] = {c.V.p, c.W.p, c.P.p};
  if (nnbr) {
    const std::vector<double> fill(nnbr, q.nbr_fill);
    for (double *b : with_nbr) HIP_CHECK(hipMemcpyAsync(b + (size_t)P0_ * RS_, fill.data(), sizeof(double) * nnbr, hipMemcpyHostToDevice, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
  }
  CertCoef K;
  std::memset(&K, 0, sizeof(K));
  std::copy(q.C, q.C + 3 * d * d, K.C);
  std::copy(q.theta, q.theta + d, K.theta);
  launch_cert_update(lc(all), K, q.precondition ? c.Tp.p : nullptr, c.V.p, c.W.p, c.P.p, c.SV.p, c.SW.p, c.SP.p, c.partials.p);
  launch_cert_reduce(st_, T_, nsums, c.partials.p, c.h_sums, sched_.flag());
  wait_flag(sched_.last_seq());
  std::copy(c.h_sums, c.h_sums + nsums, q.sums);
  const double *const res[6] = {c.V.p, c.W.p, c.P.p, c.SV.p, c.SW.p, c.SP.p};
  for (int k = 0; k < 6; k++) cert_download(res[k], q.out[k], q.ld, d);
  for (int k = 0; k < 3 && nnbr; k++)
    HIP_CHECK(hipMemcpy(q.nbr + k * nnbr, with_nbr[k] + (size_t)P0_ * RS_, sizeof(double) * nnbr, hipMemcpyDeviceToHost));
  return 0;
}

int Group::debug_cert_precon(double *T) {
  if (!T || cert_ready() != 0) return -1;
  CertState &c = *cert_;
  cert_build_precon();
  const int BB = B_ * B_;
  std::vector<double> Tp((size_t)P0_ * BB);
  HIP_CHECK(hipMemcpy(Tp.data(), c.Tp.p, sizeof(double) * Tp.size(), hipMemcpyDeviceToHost));
  for (int row = 0; row < P0_; row++) std::copy(&Tp[(size_t)row * BB], &Tp[(size_t)(row + 1) * BB], T + (size_t)c.gid[row] * BB);
  return 0;
}

// sums | nblk | used | theta[d] | C (3d x d row-major) | 1 where a refresh followed (set by cert_search)
void Group::cert_trace_pass(const double *sums, int nblk, int used, const CertCoef &K) {
  std::vector<double> &t = cert_trace_;
  t.insert(t.end(), sums, sums + cert_nsums(d_));
  t.push_back(nblk);
  t.push_back(used);
  t.insert(t.end(), K.theta, K.theta + d_);
  t.insert(t.end(), K.C, K.C + 3 * d_ * d_);
  t.push_back(0.0);
}

}  // namespace dpgo
