// The per-edge arithmetic of the measurement sensitivities (sens.h): the mixed second derivative of one edge's own term in the
// direction of an adjoint and in the edge's parameters.  Plain fp64 with explicit FMAs in a fixed order, no memory but the
// caller's arrays: k_sens_edge (sens.hip) runs it with one lane per (edge, column), sens_edge_host (sens.cpp) on the host.
//
// Records as in edge_math.h: an edge record q (ints i, j, inter; R~ row-major, t~, kappa, tau), a pose record [t | rows of Y],
// Y = R^T.  With a = t_j - t_i - R_i t~ and B = R_j - R_i R~ the edge's term is 1/2 s_e = 1/2 tau |a|^2 + 1/2 kappa |B|_F^2.  In the
// tangent coordinates of cov.h an adjoint lambda = (dt_i, omega_i, dt_j, omega_j) moves the poses by t + dt, R <- R Exp(hat(omega)):
//     da = dt_j - dt_i - R_i hat(omega_i) t~,      dB = R_j hat(omega_j) - R_i hat(omega_i) R~,
//     phi_e = D_lambda (1/2 s_e) = tau a^T da + kappa <B, dB>   ( = lambda_i^T ghat_e(i) + lambda_j^T ghat_e(j), robust_math.h ).
// The parameters move by kappa + dkappa, tau + dtau, t~ + dt~ (raw entries) and R~ <- R~ Exp(hat(eta)), and
//     d phi / d tau   = a^T da                      d phi / d t~    = -tau (R_i^T da - hat(omega_i) R_i^T a)
//     d phi / d kappa = <B, dB>                     d phi / d eta_k = -kappa <hat(e_k), R~^T (R_i^T dB - hat(omega_i) R_i^T B)>.
// sens_one writes MINUS these: dL/dtheta_e = -d phi_e / d theta_e for the adjoint lambda = H^-1 c of an upstream gradient c.
#pragma once
#include "cov.h"
#include "edge_math.h"

namespace dpgo {

// y = hat(w) v  (D = 3: w x v; D = 2: w [[0, -1], [1, 0]] v)
template <int D>
__host__ __device__ __forceinline__ void sens_hat(const double *w, const double *v, double *y) {
  if (D == 3) {
    y[0] = fma(w[1], v[2], -(w[2] * v[1]));
    y[1] = fma(w[2], v[0], -(w[0] * v[2]));
    y[2] = fma(w[0], v[1], -(w[1] * v[0]));
  } else {
    y[0] = -(w[0] * v[1]);
    y[1] = w[0] * v[0];
  }
}

// q: the edge record; xi, xj: the pose records of its poses; lam_i, lam_j: their dof coordinates of the adjoint.
// out: 2 + dof doubles, -d phi / d (kappa, tau, t~[0..D), eta[0..dof - D)); phi (optional): phi_e.
template <int D>
__host__ __device__ inline void sens_one(const double *q, const double *xi, const double *xj, const double *lam_i,
                                         const double *lam_j, double *out, double *phi) {
  constexpr int NR = D * (D - 1) / 2;
  const double *R = q + 2, *t = q + 2 + D * D;
  const double kappa = q[2 + D * D + D], tau = q[2 + D * D + D + 1];
  const double *Yi = xi + D, *Yj = xj + D, *wi = lam_i + D, *wj = lam_j + D;
  // the translation part: a, da (world frame), their images under R_i^T = Y_i
  double hw[D], a[D], da[D];
  sens_hat<D>(wi, t, hw);
#pragma unroll
  for (int c = 0; c < D; c++) {
    double p = 0, h = 0;
#pragma unroll
    for (int k = 0; k < D; k++) {
      p = fma(t[k], Yi[k * D + c], p);
      h = fma(hw[k], Yi[k * D + c], h);
    }
    a[c] = (xj[c] - xi[c]) - p;
    da[c] = (lam_j[c] - lam_i[c]) - h;
  }
  double s_tau = 0;
#pragma unroll
  for (int c = 0; c < D; c++) s_tau = fma(a[c], da[c], s_tau);
  double ra[D], rda[D], hra[D];
#pragma unroll
  for (int k = 0; k < D; k++) {
    double u = 0, v = 0;
#pragma unroll
    for (int c = 0; c < D; c++) {
      u = fma(Yi[k * D + c], a[c], u);
      v = fma(Yi[k * D + c], da[c], v);
    }
    ra[k] = u;
    rda[k] = v;
  }
  sens_hat<D>(wi, ra, hra);
  // the rotation part on the transposes: Bt = B^T = Y_j - R~^T Y_i, dBt = dB^T = R~^T (hat(omega_i) Y_i) - hat(omega_j) Y_j
  double P[D * D], Q[D * D], Bt[D * D], dBt[D * D];
#pragma unroll
  for (int c = 0; c < D; c++) {
    double col[D], y[D];
#pragma unroll
    for (int k = 0; k < D; k++) col[k] = Yi[k * D + c];
    sens_hat<D>(wi, col, y);
#pragma unroll
    for (int k = 0; k < D; k++) P[k * D + c] = y[k];
#pragma unroll
    for (int k = 0; k < D; k++) col[k] = Yj[k * D + c];
    sens_hat<D>(wj, col, y);
#pragma unroll
    for (int k = 0; k < D; k++) Q[k * D + c] = y[k];
  }
  double s_kappa = 0;
#pragma unroll
  for (int r = 0; r < D; r++)
#pragma unroll
    for (int c = 0; c < D; c++) {
      double g = 0, h = 0;
#pragma unroll
      for (int k = 0; k < D; k++) {
        g = fma(R[k * D + r], Yi[k * D + c], g);
        h = fma(R[k * D + r], P[k * D + c], h);
      }
      Bt[r * D + c] = Yj[r * D + c] - g;
      dBt[r * D + c] = h - Q[r * D + c];
      s_kappa = fma(Bt[r * D + c], dBt[r * D + c], s_kappa);
    }
  // C = Y_i dB - hat(omega_i) Y_i B (row k, column r), column by column; then Z = R~^T C
  double C[D * D];
#pragma unroll
  for (int r = 0; r < D; r++) {
    double g[D], y[D];
#pragma unroll
    for (int k = 0; k < D; k++) {
      double u = 0;
#pragma unroll
      for (int c = 0; c < D; c++) u = fma(Yi[k * D + c], Bt[r * D + c], u);
      g[k] = u;
    }
    sens_hat<D>(wi, g, y);
#pragma unroll
    for (int k = 0; k < D; k++) {
      double u = 0;
#pragma unroll
      for (int c = 0; c < D; c++) u = fma(Yi[k * D + c], dBt[r * D + c], u);
      C[k * D + r] = u - y[k];
    }
  }
  out[0] = -s_kappa;
  out[1] = -s_tau;
#pragma unroll
  for (int k = 0; k < D; k++) out[2 + k] = tau * (rda[k] - hra[k]);
#pragma unroll
  for (int k = 0; k < NR; k++) {
    int r1, r2;
    cov_rot_rows<D>(k, r1, r2);
    // <hat(e_k), Z> = Z[r2][r1] - Z[r1][r2],  Z[p][r] = sum_l R~[l][p] C[l][r]
    double z = 0;
#pragma unroll
    for (int l = 0; l < D; l++) z = fma(R[l * D + r2], C[l * D + r1], fma(-R[l * D + r1], C[l * D + r2], z));
    out[2 + D + k] = kappa * z;
  }
  if (phi) *phi = fma(tau, s_tau, kappa * s_kappa);
}

}  // namespace dpgo
