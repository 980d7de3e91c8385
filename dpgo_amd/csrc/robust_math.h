// The per-edge arithmetic of the robust Hessian (robust.h), as functions the device kernels (robust.hip) and the host's debug
// hook (robust_edge_host, robust.cpp; no GPU needed) both compile: the curvature of the loss, the rows of M_e X, the tangent
// gradient of one edge, an entry of M_e.  Plain fp64 with explicit FMAs in a fixed order, no memory but the caller's arrays.
//
// Records as in edge_math.h: an edge record q (ints i, j, inter; R row-major, t, kappa, tau), a pose record [t | rows of Y].
// M_e is the edge's block of the data matrix as the assembly writes it (assemble.cpp; DPGO_utils.cpp:1541-1641), with R_e R_e^T
// taken as the identity in the rotation block of pose i -- so that sum_e M_e is the certificate's M to the bit of its terms:
//   (i, i) = [ tau, tau t^T ; tau t, tau t t^T + kappa I ]   (i, j) = [ -tau, 0 ; -tau t, -kappa R ]   (j, j) = [ tau, 0 ; 0, kappa I ]
// With dt = t_j - t_i - t_e^T Y_i (a row) and dr = Y_j - R_e^T Y_i (d rows), s_e = tau |dt|^2 + kappa |dr|_F^2 = tr(X^T M_e X) and
//   (M_e X)_j = [ tau dt ; kappa dr ],     (M_e X)_i = [ -tau dt ; -t_e (tau dt) + kappa (Y_i - R_e Y_j) ].
// (A symmetric change of a pose's rotation block, such as kappa (R R^T - I) of a measured R that is orthogonal to six digits
// only, is absorbed by Lambda and drops out of every tangent trace: g and H do not see it.)
#pragma once
#include "cov.h"
#include "edge_math.h"

namespace dpgo {

// c_e = 2 rho''(s_e): 0 on intra edges, under the trivial loss, and exactly 0 where the weight is exactly 0
__host__ __device__ inline double robust_curv(int loss, double dl, double s, double w, bool inter) {
  if (!inter || loss == 0 || w == 0.0) return 0.0;
  if (loss == 1) return s > dl ? -w / s : 0.0;   // Huber: linear in s below the kink
  if (loss == 2) return -4.0 * w / (s + dl);     // Geman-McClure
  return -2.0 * w / dl;                          // Welsch
}

// ri, rj: the records of (M_e X)_i and (M_e X)_j, unweighted
template <int D>
__host__ __device__ inline void robust_rows(const double *q, const double *a, const double *b, double *ri, double *rj) {
  const double *R = q + 2, *t = q + 2 + D * D;
  const double kappa = q[2 + D * D + D], tau = q[2 + D * D + D + 1];
  const double *Yi = a + D, *Yj = b + D;
#pragma unroll
  for (int c = 0; c < D; c++) {
    double p = 0;
#pragma unroll
    for (int k = 0; k < D; k++) p = fma(t[k], Yi[k * D + c], p);
    rj[c] = tau * ((b[c] - a[c]) - p);
    ri[c] = -rj[c];
#pragma unroll
    for (int r = 0; r < D; r++) {
      double g = 0;
#pragma unroll
      for (int k = 0; k < D; k++) g = fma(R[k * D + r], Yi[k * D + c], g);
      rj[D + r * D + c] = kappa * (Yj[r * D + c] - g);
    }
  }
#pragma unroll
  for (int k = 0; k < D; k++)
#pragma unroll
    for (int c = 0; c < D; c++) {
      double h = 0;
#pragma unroll
      for (int r = 0; r < D; r++) h = fma(R[k * D + r], Yj[r * D + c], h);
      ri[D + k * D + c] = fma(kappa, Yi[k * D + c] - h, -(t[k] * rj[c]));
    }
}

// tr(E_a(p)^T mx): entry a of the tangent gradient of a pose whose record is x and whose rows of M X are mx (k_polish_grad's sum)
template <int D>
__host__ __device__ inline double robust_ghat_entry(const double *x, const double *mx, int a) {
  if (a < D) return mx[a];
  int r1, r2;
  cov_rot_rows<D>(a - D, r1, r2);
  double v = 0;
#pragma unroll
  for (int c = 0; c < D; c++) v = fma(x[D + r2 * D + c], mx[D + r1 * D + c], fma(-x[D + r1 * D + c], mx[D + r2 * D + c], v));
  return v;
}

// Entry (r, c) of the (d+1) x (d+1) block of M_e between the edge's pose of role rr (0: i, 1: j; the rows) and that of role
// rc (the columns); index 0 is the translation, 1 + k row k of Y.  The (j, i) block is the (i, j) block transposed and the
// (i, i) block is evaluated on r <= c, so the entries of a symmetric pair have the same bits.
template <int D>
__host__ __device__ inline double robust_m_entry(const double *q, int rr, int rc, int r, int c) {
  const double *R = q + 2, *t = q + 2 + D * D;
  const double kappa = q[2 + D * D + D], tau = q[2 + D * D + D + 1];
  if (rr == 1 && rc == 0) {
    rr = 0;
    rc = 1;
    const int s = r;
    r = c;
    c = s;
  }
  if (rr == 1) return r != c ? 0.0 : (r == 0 ? tau : kappa);
  if (rc == 1) {
    if (r == 0) return c == 0 ? -tau : 0.0;
    return c == 0 ? -(tau * t[r - 1]) : -(kappa * R[(r - 1) * D + (c - 1)]);
  }
  if (r > c) {
    const int s = r;
    r = c;
    c = s;
  }
  if (r == 0) return c == 0 ? tau : tau * t[c - 1];
  return r == c ? fma(tau, t[r - 1] * t[c - 1], kappa) : tau * (t[r - 1] * t[c - 1]);
}

}  // namespace dpgo
