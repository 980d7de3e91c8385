// Centralised chordal initialisation (host, set-up only, untimed in the driver).
//
// Same least-squares problems as the reference's --dist_init false branch
// (C++/examples/dist_pgo.cpp:416-444 -> C++/SESync/src/SESync_utils.cpp:573-652):
//   rotations   : min sum kappa |R_ij^T Y_i - Y_j|_F^2  with Y_0 = I, then per-block SO(d) projection
//   translations: min sum tau |x_i - x_j + t_ij^T Y_i|^2 with x_0 = 0
// The reference solves them with SPQR; here the normal equations are solved
// matrix-free by Jacobi-preconditioned CG to 1e-13 (same minimiser), the operators applied pose by pose on all host
// threads with reductions in a fixed order (the result does not depend on the number of threads).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <omp.h>

#include "graph.h"
#include "settings.h"

namespace dpgo {

namespace {

// nearest rotation of a d x d block (host; Jacobi eigen-decomposition of M^T M, as the device kernel)
void project_block(int d, double *M) {
  if (d == 2) {
    double c = M[0] + M[3], s = M[2] - M[1], n2 = c * c + s * s;
    if (n2 < 1e-32) { c = 1; s = 0; n2 = 1; }
    const double inv = 1.0 / std::sqrt(n2);
    M[0] = c * inv; M[1] = -s * inv; M[2] = s * inv; M[3] = c * inv;
    return;
  }
  double S[9], V[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) {
      double a = 0;
      for (int k = 0; k < 3; k++) a += M[k * 3 + r] * M[k * 3 + c];
      S[r * 3 + c] = a;
    }
  for (int sweep = 0; sweep < 30; sweep++) {
    double off = std::fabs(S[1]) + std::fabs(S[2]) + std::fabs(S[5]);
    if (off < 1e-300) break;
    for (int p = 0; p < 2; p++)
      for (int q = p + 1; q < 3; q++) {
        if (std::fabs(S[p * 3 + q]) < 1e-300) continue;
        double th = (S[q * 3 + q] - S[p * 3 + p]) / (2 * S[p * 3 + q]);
        double t = (th >= 0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1));
        double c = 1 / std::sqrt(t * t + 1), s = t * c;
        for (int k = 0; k < 3; k++) {  // S <- S J
          double a = S[k * 3 + p], b = S[k * 3 + q];
          S[k * 3 + p] = c * a - s * b; S[k * 3 + q] = s * a + c * b;
        }
        for (int k = 0; k < 3; k++) {  // S <- J^T S
          double a = S[p * 3 + k], b = S[q * 3 + k];
          S[p * 3 + k] = c * a - s * b; S[q * 3 + k] = s * a + c * b;
        }
        for (int k = 0; k < 3; k++) {
          double a = V[k * 3 + p], b = V[k * 3 + q];
          V[k * 3 + p] = c * a - s * b; V[k * 3 + q] = s * a + c * b;
        }
      }
  }
  double Bm[9], nrm[3];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) Bm[r * 3 + c] = M[r * 3] * V[c] + M[r * 3 + 1] * V[3 + c] + M[r * 3 + 2] * V[6 + c];
  for (int c = 0; c < 3; c++) nrm[c] = Bm[c] * Bm[c] + Bm[3 + c] * Bm[3 + c] + Bm[6 + c] * Bm[6 + c];
  int o[3] = {0, 1, 2};
  std::sort(o, o + 3, [&](int a, int b) { return nrm[a] > nrm[b]; });
  double u1[3], u2[3], u3[3], v[3][3];
  for (int k = 0; k < 3; k++) { u1[k] = Bm[k * 3 + o[0]]; u2[k] = Bm[k * 3 + o[1]]; for (int j = 0; j < 3; j++) v[j][k] = V[k * 3 + o[j]]; }
  double n1 = std::sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
  if (n1 < 1e-150) { for (int k = 0; k < 9; k++) M[k] = (k % 4 == 0); return; }
  for (double &x : u1) x /= n1;
  double pr = u1[0] * u2[0] + u1[1] * u2[1] + u1[2] * u2[2];
  for (int k = 0; k < 3; k++) u2[k] -= pr * u1[k];
  double n2 = std::sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
  if (n2 < 1e-14 * n1) {
    double e[3] = {0, 0, 0};
    int mi = 0;
    for (int k = 1; k < 3; k++) if (std::fabs(u1[k]) < std::fabs(u1[mi])) mi = k;
    e[mi] = 1;
    u2[0] = u1[1] * e[2] - u1[2] * e[1]; u2[1] = u1[2] * e[0] - u1[0] * e[2]; u2[2] = u1[0] * e[1] - u1[1] * e[0];
    n2 = std::sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
  }
  for (double &x : u2) x /= n2;
  u3[0] = u1[1] * u2[2] - u1[2] * u2[1]; u3[1] = u1[2] * u2[0] - u1[0] * u2[2]; u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
  // v3 must complete a right-handed frame with v1, v2 so that det V = +1
  double v3[3] = {v[0][1] * v[1][2] - v[0][2] * v[1][1], v[0][2] * v[1][0] - v[0][0] * v[1][2], v[0][0] * v[1][1] - v[0][1] * v[1][0]};
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) M[r * 3 + c] = u1[r] * v[0][c] + u2[r] * v[1][c] + u3[r] * v3[c];
}

// Sums of K x nc per-row terms, in an order that does not depend on the number of threads: rows are cut into fixed
// chunks, each chunk is summed by one thread, the chunk sums are added in order.
template <class F>
void chunk_sums(int n, int len, std::vector<double> &out, const F &f) {
  constexpr int CH = 4096;
  const int nch = (n + CH - 1) / CH;
  std::vector<double> part((size_t)nch * len, 0.0);
#pragma omp parallel for schedule(static)
  for (int ch = 0; ch < nch; ch++) {
    double *acc = &part[(size_t)ch * len];
    const int i1 = std::min(n, (ch + 1) * CH);
    for (int i = ch * CH; i < i1; i++) f(i, acc);
  }
  out.assign(len, 0.0);
  for (int ch = 0; ch < nch; ch++)
    for (int k = 0; k < len; k++) out[k] += part[(size_t)ch * len + k];
}

template <class Apply>
int pcg(int n, int nc, const Apply &A, const std::vector<double> &diag, const std::vector<double> &b,
        std::vector<double> &x, double tol, int maxit) {
  // all nc right-hand sides share the iteration (block of independent CGs)
  std::vector<double> r = b, z(r.size()), p(r.size()), Ap(r.size());
  x.assign(b.size(), 0.0);
  std::vector<double> s0;
  chunk_sums(n, 2 * nc, s0, [&](int i, double *acc) {
    for (int c = 0; c < nc; c++) {
      z[(size_t)i * nc + c] = r[(size_t)i * nc + c] / diag[i];
      acc[c] += r[(size_t)i * nc + c] * z[(size_t)i * nc + c];
      acc[nc + c] += b[(size_t)i * nc + c] * b[(size_t)i * nc + c];
    }
  });
  std::vector<double> rz(s0.begin(), s0.begin() + nc), b2(s0.begin() + nc, s0.end());
  p = z;
  int it = 0;
  std::vector<double> pAp, r2, rz_new, al(nc), be(nc);
  for (; it < maxit; it++) {
    A(p, Ap);
    chunk_sums(n, nc, pAp, [&](int i, double *acc) {
      for (int c = 0; c < nc; c++) acc[c] += p[(size_t)i * nc + c] * Ap[(size_t)i * nc + c];
    });
    for (int c = 0; c < nc; c++) al[c] = pAp[c] > 0 ? rz[c] / pAp[c] : 0.0;
    chunk_sums(n, nc, r2, [&](int i, double *acc) {
      for (int c = 0; c < nc; c++) {
        x[(size_t)i * nc + c] += al[c] * p[(size_t)i * nc + c];
        r[(size_t)i * nc + c] -= al[c] * Ap[(size_t)i * nc + c];
        acc[c] += r[(size_t)i * nc + c] * r[(size_t)i * nc + c];
      }
    });
    bool done = true;
    for (int c = 0; c < nc; c++) done = done && (r2[c] <= tol * tol * std::max(b2[c], 1e-300));
    if (done) break;
    chunk_sums(n, nc, rz_new, [&](int i, double *acc) {
      for (int c = 0; c < nc; c++) {
        z[(size_t)i * nc + c] = r[(size_t)i * nc + c] / diag[i];
        acc[c] += r[(size_t)i * nc + c] * z[(size_t)i * nc + c];
      }
    });
    for (int c = 0; c < nc; c++) be[c] = rz[c] > 0 ? rz_new[c] / rz[c] : 0.0;
#pragma omp parallel for schedule(static)
    for (int i = 0; i < n; i++)
      for (int c = 0; c < nc; c++) p[(size_t)i * nc + c] = z[(size_t)i * nc + c] + be[c] * p[(size_t)i * nc + c];
    rz = rz_new;
  }
  return it;
}

}  // namespace

void project_to_SOd_host(int d, double *M) { project_block(d, M); }

int chordal_initialization(const Graph &g, double *X, int ld) {
  const int d = g.d, N = g.num_poses;
  const auto &E = g.all;
  if (ld < (d + 1) * N) return -1;
  // ---- rotations: unknown Y (d N x d row-major), rows of pose 0 fixed to I
  const int nr = d * N;
  // incidence lists: the operators below are applied pose by pose (gather form: every pose adds the terms of its
  // incident edges in list order), so the products run on all host threads and do not depend on their number
  omp_set_num_threads(host_threads());
  std::vector<int> inc_ptr(N + 1, 0), inc;
  for (const auto &m : E) { inc_ptr[m.ipose + 1]++; inc_ptr[m.jpose + 1]++; }
  for (int i = 0; i < N; i++) inc_ptr[i + 1] += inc_ptr[i];
  inc.resize(inc_ptr[N]);
  {
    std::vector<int> pos(inc_ptr.begin(), inc_ptr.end() - 1);
    for (int e = 0; e < (int)E.size(); e++) {
      inc[pos[E[e].ipose]++] = 2 * e;        // tail
      inc[pos[E[e].jpose]++] = 2 * e + 1;    // head
    }
  }
  // pin0: the rows of pose 0 count as zero (the pinned pose's column is dropped)
  auto applyR = [&](const std::vector<double> &v, std::vector<double> &out, bool pin0 = false) {
#pragma omp parallel for schedule(dynamic, 256)
    for (int p = 0; p < N; p++) {
      double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      for (int q = inc_ptr[p]; q < inc_ptr[p + 1]; q++) {
        const auto &m = E[inc[q] >> 1];
        const int i = m.ipose, j = m.jpose;
        double W[9];
        for (int r = 0; r < d; r++)
          for (int c = 0; c < d; c++) {
            double a = (pin0 && j == 0) ? 0.0 : -v[((size_t)j * d + r) * d + c];
            if (!(pin0 && i == 0))
              for (int k = 0; k < d; k++) a += m.R[k * d + r] * v[((size_t)i * d + k) * d + c];
            W[r * d + c] = m.kappa * a;
          }
        if (inc[q] & 1) {
          for (int k = 0; k < d * d; k++) acc[k] -= W[k];
        } else {
          for (int r = 0; r < d; r++)
            for (int c = 0; c < d; c++) {
              double a = 0;
              for (int k = 0; k < d; k++) a += m.R[r * d + k] * W[k * d + c];
              acc[r * d + c] += a;
            }
        }
      }
      for (int k = 0; k < d * d; k++) out[(size_t)p * d * d + k] = acc[k];
    }
  };
  std::vector<double> Y0((size_t)nr * d, 0.0), LY0(Y0.size()), b(Y0.size()), Ysol, diag(nr, 0.0);
  for (int k = 0; k < d; k++) Y0[k * d + k] = 1.0;
  applyR(Y0, LY0);
  for (size_t k = 0; k < b.size(); k++) b[k] = -LY0[k];
  for (const auto &m : E)
    for (int r = 0; r < d; r++) {
      double rr = 0;
      for (int k = 0; k < d; k++) rr += m.R[r * d + k] * m.R[r * d + k];
      diag[m.ipose * d + r] += m.kappa * rr;
      diag[m.jpose * d + r] += m.kappa;
    }
  // pin pose 0: identity rows in the operator
  auto applyRp = [&](const std::vector<double> &v, std::vector<double> &out) {
    applyR(v, out, true);
    for (int k = 0; k < d * d; k++) out[k] = v[k];
  };
  for (int k = 0; k < d * d; k++) b[k] = 0.0;
  for (int r = 0; r < d; r++) diag[r] = 1.0;
  int it1 = pcg(nr, d, applyRp, diag, b, Ysol, 1e-13, 50000);
  for (int k = 0; k < d; k++)
    for (int c = 0; c < d; c++) Ysol[k * d + c] = (k == c);
  for (int i = 1; i < N; i++) {
    // the reference projects R_i (= Y_i^T); projection commutes with transposition
    project_block(d, &Ysol[(size_t)i * d * d]);
  }
  // ---- translations
  std::vector<double> bt((size_t)N * d, 0.0), xsol, dg(N, 0.0);
  for (const auto &m : E) {
    const int i = m.ipose, j = m.jpose;
    for (int c = 0; c < d; c++) {
      double a = 0;
      for (int k = 0; k < d; k++) a += m.t[k] * Ysol[((size_t)i * d + k) * d + c];
      bt[i * d + c] -= m.tau * a;
      bt[j * d + c] += m.tau * a;
    }
    dg[i] += m.tau;
    dg[j] += m.tau;
  }
  auto applyT = [&](const std::vector<double> &v, std::vector<double> &out) {
#pragma omp parallel for schedule(dynamic, 256)
    for (int p = 1; p < N; p++) {
      double acc[3] = {0, 0, 0};
      for (int q = inc_ptr[p]; q < inc_ptr[p + 1]; q++) {
        const auto &m = E[inc[q] >> 1];
        const int o = (inc[q] & 1) ? m.ipose : m.jpose;   // the other end; pose 0 is pinned (its column is dropped)
        for (int c = 0; c < d; c++) acc[c] += m.tau * (v[(size_t)p * d + c] - (o == 0 ? 0.0 : v[(size_t)o * d + c]));
      }
      for (int c = 0; c < d; c++) out[(size_t)p * d + c] = acc[c];
    }
    for (int c = 0; c < d; c++) out[c] = v[c];
  };
  for (int c = 0; c < d; c++) bt[c] = 0.0;
  dg[0] = 1.0;
  int it2 = pcg(N, d, applyT, dg, bt, xsol, 1e-13, 50000);
  // the reference solves both least-squares problems directly (SPQR); an iteration that ran into its cap has
  // not reached the 1e-13 residual target, and the caller must know (disconnected or badly scaled graph)
  if (settings().setup_timing)
    fprintf(stderr, "[setup] chordal initialisation: %d PCG iterations for the rotations, %d for the translations\n", it1, it2);
  if (it1 >= 50000 || it2 >= 50000) {
    fprintf(stderr, "[dpgo_amd] ERROR: chordal initialisation: PCG did not converge (rotations %d, translations %d of 50000 "
                    "iterations); is the graph connected?\n", it1, it2);
    return -1;
  }
  for (int i = 0; i < N; i++)
    for (int c = 0; c < d; c++) {
      X[(size_t)c * ld + i] = i == 0 ? 0.0 : xsol[i * d + c];
      for (int r = 0; r < d; r++) X[(size_t)c * ld + N + i * d + r] = Ysol[((size_t)i * d + r) * d + c];
    }
  return 0;
}

}  // namespace dpgo
