// The per-edge arithmetic of the sensitivities of the ROBUST objective (rsens.h): what the loss adds to sens_math.h.  Plain fp64
// with explicit FMAs in a fixed order, no memory but the caller's arrays: k_rsens_prep and k_rsens_edge (rsens.hip) run it on
// the device, robust_sens_edge_host (rsens.cpp) on the host.
//
// Records, a, B and phi_e as in sens_math.h.  With F = 1/2 sum_intra s_e + 1/2 sum_inter rho(s_e; delta), w_e = rho'(s_e) and
// c_e = 2 rho''(s_e) (robust_math.h: robust_curv) the gradient is g = sum_e w_e ghat_e, so for an adjoint lambda
//     lambda^T g = sum_e w_e phi_e,      d/dtheta_e (lambda^T g) = w_e d phi_e / d theta_e + (c_e / 2) phi_e d s_e / d theta_e,
//     d/ddelta (lambda^T g) = sum_inter (d w_e / d delta) phi_e
// with s_e = tau |a|^2 + kappa |B|_F^2 and the parameters of sens_math.h (kappa, tau, t~ raw, R~ <- R~ Exp(hat(eta))):
//     d s / d kappa = |B|_F^2     d s / d tau = |a|^2     d s / d t~ = -2 tau R_i^T a     d s / d eta_k = -2 kappa <hat(e_k), R~^T R_i^T B>.
// d w / d delta from edge_loss's formulas (edge_math.h), on the branch robust_curv takes: Huber w / (2 delta) for s > delta and
// 0 for s <= delta; Geman-McClure 2 delta s / (s + delta)^3; Welsch w s / delta^2; 0 on intra edges, under the trivial loss and
// where w is exactly 0.
#pragma once
#include "cov.h"
#include "edge_math.h"

namespace dpgo {

// q: the edge record; xi, xj: the pose records of its poses.  ds: 2 + dof doubles, d s_e / d (kappa, tau, t~[0..D), eta[0..dof - D))
template <int D>
__host__ __device__ inline void rsens_ds(const double *q, const double *xi, const double *xj, double *ds) {
  constexpr int NR = D * (D - 1) / 2;
  const double *R = q + 2, *t = q + 2 + D * D;
  const double kappa = q[2 + D * D + D], tau = q[2 + D * D + D + 1];
  const double *Yi = xi + D, *Yj = xj + D;
  // a (world frame), |a|^2, R_i^T a = Y_i a
  double a[D], aa = 0;
#pragma unroll
  for (int c = 0; c < D; c++) {
    double p = 0;
#pragma unroll
    for (int k = 0; k < D; k++) p = fma(t[k], Yi[k * D + c], p);
    a[c] = (xj[c] - xi[c]) - p;
    aa = fma(a[c], a[c], aa);
  }
  const double tau2 = -2.0 * tau, kappa2 = -2.0 * kappa;
#pragma unroll
  for (int k = 0; k < D; k++) {
    double u = 0;
#pragma unroll
    for (int c = 0; c < D; c++) u = fma(Yi[k * D + c], a[c], u);
    ds[2 + k] = tau2 * u;
  }
  // Bt = B^T = Y_j - R~^T Y_i, |B|_F^2
  double Bt[D * D], bb = 0;
#pragma unroll
  for (int r = 0; r < D; r++)
#pragma unroll
    for (int c = 0; c < D; c++) {
      double g = 0;
#pragma unroll
      for (int k = 0; k < D; k++) g = fma(R[k * D + r], Yi[k * D + c], g);
      Bt[r * D + c] = Yj[r * D + c] - g;
      bb = fma(Bt[r * D + c], Bt[r * D + c], bb);
    }
  ds[0] = bb;
  ds[1] = aa;
  // C = Y_i B (row k, column r); <hat(e_k), R~^T C> as in sens_one
  double C[D * D];
#pragma unroll
  for (int r = 0; r < D; r++)
#pragma unroll
    for (int k = 0; k < D; k++) {
      double u = 0;
#pragma unroll
      for (int c = 0; c < D; c++) u = fma(Yi[k * D + c], Bt[r * D + c], u);
      C[k * D + r] = u;
    }
#pragma unroll
  for (int k = 0; k < NR; k++) {
    int r1, r2;
    cov_rot_rows<D>(k, r1, r2);
    double z = 0;
#pragma unroll
    for (int l = 0; l < D; l++) z = fma(R[l * D + r2], C[l * D + r1], fma(-R[l * D + r1], C[l * D + r2], z));
    ds[2 + D + k] = kappa2 * z;
  }
}

// d w_e / d delta at s with w = rho'(s) as edge_loss left it
__host__ __device__ inline double rsens_dw(int loss, double dl, double s, double w, bool inter) {
  if (!inter || loss == 0 || w == 0.0) return 0.0;
  if (loss == 1) return s > dl ? w / (2.0 * dl) : 0.0;   // Huber: robust_curv's side of the kink
  if (loss == 2) {                                       // Geman-McClure
    const double q = s + dl;
    return (2.0 * dl * s) / (q * q * q);
  }
  return (w * s) / (dl * dl);                            // Welsch
}

// o: what sens_one wrote for this (edge, adjoint), phi: its phi_e; ds, dw: of the edge.  out: 3 + dof doubles,
// dL / d (kappa, tau, t~, eta) and the edge's term of dL / d delta.
template <int D>
__host__ __device__ __forceinline__ void rsens_combine(double w, double c, double phi, const double *ds, double dw, const double *o,
                                                       double *out) {
  constexpr int NO = 2 + D + D * (D - 1) / 2;
  const double h = -(0.5 * c) * phi;
#pragma unroll
  for (int a = 0; a < NO; a++) out[a] = fma(h, ds[a], w * o[a]);
  out[NO] = -(dw * phi);
}

}  // namespace dpgo
