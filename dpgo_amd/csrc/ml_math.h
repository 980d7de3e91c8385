// The per-edge arithmetic of the maximum-likelihood objective (ml.h), as functions the device kernels (ml.hip) and the host's
// debug hook (ml_edge_host, ml.cpp; no GPU needed) both compile.  Plain fp64 with explicit FMAs in a fixed order, no memory but
// the caller's arrays.
//
// Records as in edge_math.h: an edge record q (ints i, j, inter; R~ row-major, t~, kappa, tau), a pose record [t | rows of
// Y = R^T].  Omega: dof x dof row-major.  With A = R~^T Y_i, u = Y_i (t_j - t_i), E = A Y_j^T, phi = Log(E):
//
//   r = [ R~^T (u - t~) ; phi ]
//   J_i = [ -A   R~^T hat(u) ]        J_j = [ A   0          ]        (rows: r; columns: cov.h's unknowns of the pose)
//         [  0   -Jl R~^T    ]              [ 0   Jr         ]
//
// Jr = I + 1/2 hat(phi) + c (phi phi^T - |phi|^2 I) is the inverse right Jacobian of SO(3) at phi, Jl = Jr^T the inverse left
// one, c = 1 / theta^2 - (1 + cos theta) / (2 theta sin theta), 1/12 + theta^2 / 720 below theta^2 = 1e-8.  d = 2: hat(u) is the
// column (u_1, -u_0), phi the angle, Jr = Jl = 1.  theta = atan2(|a|, (tr E - 1) / 2) with a the vector of E's antisymmetric
// part, phi = (theta / |a|) a, (1 + theta^2 / 6) a below theta^2 = 1e-8.
#pragma once
#include <cmath>

#include "cov.h"

namespace dpgo {

constexpr double ML_SERIES_T2 = 1e-8;    // theta^2 below which Log and Jr use their series (the polish's retraction has the same)
constexpr double ML_NEAR_PI = 1e-3;      // edges with theta > pi - this are counted (near_pi); their values are not specified

// r (dof), Ji, Jj (dof x dof row-major) of one edge; returns whether theta > pi - ML_NEAR_PI
template <int D>
__host__ __device__ inline bool ml_residual(const double *q, const double *a, const double *b, double *r, double *Ji, double *Jj) {
  constexpr int DOF = cov_dof(D);
  const double *R = q + 2, *t = q + 2 + D * D;
  const double *Yi = a + D, *Yj = b + D;
#pragma unroll
  for (int k = 0; k < DOF * DOF; k++) Ji[k] = Jj[k] = 0.0;
  double u[D], v[D], A[D * D];
#pragma unroll
  for (int r0 = 0; r0 < D; r0++) {
    double s = 0;
#pragma unroll
    for (int c = 0; c < D; c++) s = fma(Yi[r0 * D + c], b[c] - a[c], s);
    u[r0] = s;
    v[r0] = s - t[r0];
  }
#pragma unroll
  for (int k = 0; k < D; k++) {
    double s = 0;
#pragma unroll
    for (int r0 = 0; r0 < D; r0++) s = fma(R[r0 * D + k], v[r0], s);
    r[k] = s;
#pragma unroll
    for (int c = 0; c < D; c++) {
      double g = 0;
#pragma unroll
      for (int r0 = 0; r0 < D; r0++) g = fma(R[r0 * D + k], Yi[r0 * D + c], g);
      A[k * D + c] = g;
      Ji[k * DOF + c] = -g;
      Jj[k * DOF + c] = g;
    }
  }
  double E[D * D];
#pragma unroll
  for (int k = 0; k < D; k++)
#pragma unroll
    for (int l = 0; l < D; l++) {
      double s = 0;
#pragma unroll
      for (int c = 0; c < D; c++) s = fma(A[k * D + c], Yj[l * D + c], s);
      E[k * D + l] = s;
    }
  if constexpr (D == 2) {
#pragma unroll
    for (int k = 0; k < 2; k++) Ji[k * DOF + 2] = fma(R[k], u[1], -(R[2 + k] * u[0]));
    const double th = atan2(0.5 * (E[2] - E[1]), 0.5 * (E[0] + E[3]));
    r[2] = th;
    Ji[2 * DOF + 2] = -1.0;
    Jj[2 * DOF + 2] = 1.0;
    return fabs(th) > M_PI - ML_NEAR_PI;
  } else {
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
      for (int l = 0; l < 3; l++) {
        const int l1 = (l + 1) % 3, l2 = (l + 2) % 3;
        Ji[k * DOF + 3 + l] = fma(R[l1 * 3 + k], u[l2], -(R[l2 * 3 + k] * u[l1]));
      }
    const double a0 = 0.5 * (E[7] - E[5]), a1 = 0.5 * (E[2] - E[6]), a2 = 0.5 * (E[3] - E[1]);
    const double sn = sqrt(fma(a0, a0, fma(a1, a1, a2 * a2))), cs = 0.5 * ((E[0] + E[4] + E[8]) - 1.0);
    const double th = atan2(sn, cs), t2 = th * th;
    double scale, c;
    if (t2 < ML_SERIES_T2) {
      scale = 1.0 + t2 / 6.0;
      c = 1.0 / 12.0 + t2 / 720.0;
    } else {
      scale = th / sn;
      c = 1.0 / t2 - (1.0 + cs) / (2.0 * th * sn);
    }
    const double p[3] = {scale * a0, scale * a1, scale * a2};
    const double pp = fma(p[0], p[0], fma(p[1], p[1], p[2] * p[2]));
    double Jr[9];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      r[3 + k] = p[k];
#pragma unroll
      for (int l = 0; l < 3; l++) Jr[k * 3 + l] = fma(c, k == l ? fma(p[k], p[l], -pp) : p[k] * p[l], k == l ? 1.0 : 0.0);
    }
    // + 1/2 hat(phi)
    Jr[1] = fma(-0.5, p[2], Jr[1]);
    Jr[2] = fma(0.5, p[1], Jr[2]);
    Jr[3] = fma(0.5, p[2], Jr[3]);
    Jr[5] = fma(-0.5, p[0], Jr[5]);
    Jr[6] = fma(-0.5, p[1], Jr[6]);
    Jr[7] = fma(0.5, p[0], Jr[7]);
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
      for (int l = 0; l < 3; l++) {
        Jj[(3 + k) * DOF + 3 + l] = Jr[k * 3 + l];
        double s = 0;
#pragma unroll
        for (int r0 = 0; r0 < 3; r0++) s = fma(Jr[r0 * 3 + k], R[l * 3 + r0], s);
        Ji[(3 + k) * DOF + 3 + l] = -s;
      }
    return th > M_PI - ML_NEAR_PI;
  }
}

// wr = Omega r, chi2 = r' wr
template <int D>
__host__ __device__ inline double ml_weigh(const double *Om, const double *r, double *wr) {
  constexpr int DOF = cov_dof(D);
  double chi2 = 0;
#pragma unroll
  for (int k = 0; k < DOF; k++) {
    double s = 0;
#pragma unroll
    for (int l = 0; l < DOF; l++) s = fma(Om[k * DOF + l], r[l], s);
    wr[k] = s;
  }
#pragma unroll
  for (int k = 0; k < DOF; k++) chi2 = fma(r[k], wr[k], chi2);
  return chi2;
}

// entry a of J^T wr: the edge's term of a pose's gradient
template <int D>
__host__ __device__ inline double ml_grad_entry(const double *J, const double *wr, int a) {
  constexpr int DOF = cov_dof(D);
  double s = 0;
#pragma unroll
  for (int k = 0; k < DOF; k++) s = fma(J[k * DOF + a], wr[k], s);
  return s;
}

// entry (k, a) of W = Omega J
template <int D>
__host__ __device__ inline double ml_w_entry(const double *Om, const double *J, int k, int a) {
  constexpr int DOF = cov_dof(D);
  double s = 0;
#pragma unroll
  for (int l = 0; l < DOF; l++) s = fma(Om[k * DOF + l], J[l * DOF + a], s);
  return s;
}

// Entry (a, b) of the edge's term J_rr^T Omega J_rc of the block between its pose of role rr (0: i, 1: j; the rows) and that
// of role rc (the columns), from the edge's stored record jw = [J_i | J_j | Omega J_i | Omega J_j].  The (j, i) block is the
// (i, j) block transposed and a diagonal block is evaluated on a <= b, so the entries of a symmetric pair have the same bits.
template <int D>
__host__ __device__ inline double ml_block_entry(const double *jw, int rr, int rc, int a, int b) {
  constexpr int DOF = cov_dof(D), DD = DOF * DOF;
  if (rr > rc || (rr == rc && a > b)) {
    const int s = rr, x = a;
    rr = rc;
    rc = s;
    a = b;
    b = x;
  }
  const double *J = jw + rr * DD, *W = jw + (2 + rc) * DD;
  double s = 0;
#pragma unroll
  for (int k = 0; k < DOF; k++) s = fma(J[k * DOF + a], W[k * DOF + b], s);
  return s;
}

}  // namespace dpgo
