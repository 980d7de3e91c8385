// The arithmetic of one pair of poses (pairs.h): the relative pose, the Jacobian of its perturbation, the relative covariance,
// the residual of a candidate measurement and its Mahalanobis distance.  Plain fp64 in a fixed order, no memory but the
// caller's arrays: k_pairs_gate (pairs.hip) runs it with one lane per pair, dpgo_debug_pairs_gate (capi_debug.cpp) on the host.
//
// A pose record is t (D doubles), then Y = R^T row-major (D x D), as everywhere in the library.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define PAIRS_HD __host__ __device__ __forceinline__
#else
#define PAIRS_HD inline
#endif

namespace dpgo {

template <int D>
struct PairsDims {
  static constexpr int DOF = D + D * (D - 1) / 2, DD = DOF * DOF, RS = (D + 1) * D;
  static constexpr int CAND = D * D + D + 2;   // a candidate: R~ (D x D row-major), t~ (D), kappa, tau
};

// R_pq = R_p^T R_q = Y_p Y_q^T (row-major),  t_pq = R_p^T (t_q - t_p) = Y_p (t_q - t_p)
template <int D>
PAIRS_HD void pairs_relative(const double *recp, const double *recq, double *Rpq, double *tpq) {
  const double *Yp = recp + D, *Yq = recq + D;
  double dt[D];
#pragma unroll
  for (int i = 0; i < D; i++) dt[i] = recq[i] - recp[i];
#pragma unroll
  for (int i = 0; i < D; i++) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < D; j++) s = fma(Yp[i * D + j], dt[j], s);
    tpq[i] = s;
#pragma unroll
    for (int j = 0; j < D; j++) {
      double r = 0.0;
#pragma unroll
      for (int k = 0; k < D; k++) r = fma(Yp[i * D + k], Yq[j * D + k], r);
      Rpq[i * D + j] = r;
    }
  }
}

// J = [J_p  J_q] (DOF x 2 DOF row-major) of (dt_pq, domega_pq) in the tangent coordinates of cov.h (dt in the world frame,
// omega in the body frame):
//   J_p = [[-R_p^T, hat(t_pq)], [0, -R_pq^T]],   J_q = [[R_p^T, 0], [0, I]]
// with hat(t_pq) omega = t_pq x omega for D = 3 and the column -[[0, -1], [1, 0]] t_pq = (t_y, -t_x) for D = 2, where the
// rotation block is the scalar -1 (plane rotations commute).
template <int D>
PAIRS_HD void pairs_jacobian(const double *recp, const double *Rpq, const double *tpq, double *J) {
  constexpr int DOF = PairsDims<D>::DOF, LD = 2 * DOF;
  const double *Yp = recp + D;
#pragma unroll
  for (int i = 0; i < DOF * LD; i++) J[i] = 0.0;
#pragma unroll
  for (int i = 0; i < D; i++)
#pragma unroll
    for (int j = 0; j < D; j++) {
      J[i * LD + j] = -Yp[i * D + j];
      J[i * LD + DOF + j] = Yp[i * D + j];
    }
  if (D == 3) {
    J[0 * LD + D + 1] = -tpq[2]; J[0 * LD + D + 2] = tpq[1];
    J[1 * LD + D + 0] = tpq[2];  J[1 * LD + D + 2] = -tpq[0];
    J[2 * LD + D + 0] = -tpq[1]; J[2 * LD + D + 1] = tpq[0];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) J[(D + i) * LD + D + j] = -Rpq[j * D + i];
  } else {
    J[0 * LD + D] = tpq[1];
    J[1 * LD + D] = -tpq[0];
    J[D * LD + D] = -1.0;
  }
#pragma unroll
  for (int i = D; i < DOF; i++) J[i * LD + DOF + i] = 1.0;
}

// rel = J Sigma_joint J^T (DOF x DOF row-major), Sigma_joint = [[S_pp, S_pq], [S_pq^T, S_qq]] read from the three blocks
// (S_pq: rows of p, columns of q).  Row by row: T_i = J_i Sigma_joint, rel[i][j] = T_i . J_j, sums in ascending order.
template <int D>
PAIRS_HD void pairs_rel_cov(const double *J, const double *Spp, const double *Spq, const double *Sqq, double *rel) {
  constexpr int DOF = PairsDims<D>::DOF, LD = 2 * DOF;
#pragma unroll
  for (int i = 0; i < DOF; i++) {
    double T[LD];
#pragma unroll
    for (int c = 0; c < LD; c++) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < LD; k++) {
        const double sig = k < DOF ? (c < DOF ? Spp[k * DOF + c] : Spq[k * DOF + c - DOF])
                                   : (c < DOF ? Spq[c * DOF + k - DOF] : Sqq[(k - DOF) * DOF + c - DOF]);
        s = fma(J[i * LD + k], sig, s);
      }
      T[c] = s;
    }
#pragma unroll
    for (int j = 0; j < DOF; j++) {
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < LD; c++) s = fma(T[c], J[j * LD + c], s);
      rel[i * DOF + j] = s;
    }
  }
}

// w = vee Log(E), E a rotation (row-major).  D = 2: the angle atan2(E10, E00).  D = 3: with v = vee(E - E^T) / 2 = sin(theta) a
// and c = (tr E - 1) / 2, theta = atan2(|v|, c) and w = (theta / |v|) v; for |v| below 1e-8 the series 1 + theta^2 / 6 near the
// identity and, near theta = pi, the axis from the diagonal of the symmetric part, its signs from the largest component's row.
template <int D>
PAIRS_HD void pairs_log(const double *E, double *w) {
  if (D == 2) {
    w[0] = atan2(E[2], E[0]);
    return;
  }
  const double v[3] = {0.5 * (E[7] - E[5]), 0.5 * (E[2] - E[6]), 0.5 * (E[3] - E[1])};
  const double c = 0.5 * (E[0] + E[4] + E[8] - 1.0);
  const double s = sqrt(fma(v[0], v[0], fma(v[1], v[1], v[2] * v[2])));
  const double theta = atan2(s, c);
  if (s > 1e-8) {
    const double f = theta / s;
    for (int i = 0; i < 3; i++) w[i] = f * v[i];
  } else if (c > 0) {
    const double f = 1.0 + theta * theta / 6.0;
    for (int i = 0; i < 3; i++) w[i] = f * v[i];
  } else {
    // E + E^T = 2 c I + 2 (1 - c) a a^T: a_i^2 from the diagonal, the signs relative to the largest component
    double a[3];
    int big = 0;
    for (int i = 0; i < 3; i++) {
      a[i] = sqrt(fmax((E[4 * i] - c) / (1.0 - c), 0.0));
      if (a[i] > a[big]) big = i;
    }
    for (int i = 0; i < 3; i++)
      if (i != big && E[3 * big + i] + E[3 * i + big] < 0) a[i] = -a[i];
    // the sign of the whole axis: that of v where v still has one
    if (fma(a[0], v[0], fma(a[1], v[1], a[2] * v[2])) < 0)
      for (int i = 0; i < 3; i++) a[i] = -a[i];
    for (int i = 0; i < 3; i++) w[i] = theta * a[i];
  }
}

// r = [t_pq - t~ ; vee Log(R~^T R_pq)]
template <int D>
PAIRS_HD void pairs_residual(const double *Rpq, const double *tpq, const double *cand, double *r) {
  constexpr int DOF = PairsDims<D>::DOF;
  const double *Rt = cand, *tt = cand + D * D;
  double E[D * D], w[DOF - D];
#pragma unroll
  for (int i = 0; i < D; i++)
#pragma unroll
    for (int j = 0; j < D; j++) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < D; k++) s = fma(Rt[k * D + i], Rpq[k * D + j], s);
      E[i * D + j] = s;
    }
  pairs_log<D>(E, w);
#pragma unroll
  for (int i = 0; i < D; i++) r[i] = tpq[i] - tt[i];
#pragma unroll
  for (int i = 0; i < DOF - D; i++) r[D + i] = w[i];
}

// d^2 = r^T S^-1 r with S = rel + Omega^-1, Omega = blkdiag(tau I_D, 2 kappa I_{DOF - D}): Cholesky of the lower triangle of S
// and one forward substitution.  false (and d2 = 0) where a pivot is not positive.
template <int D>
PAIRS_HD bool pairs_mahalanobis(const double *rel, const double *r, double kappa, double tau, double *d2) {
  constexpr int DOF = PairsDims<D>::DOF;
  double L[DOF * DOF], z[DOF];
  *d2 = 0.0;
#pragma unroll
  for (int i = 0; i < DOF; i++)
#pragma unroll
    for (int j = 0; j < DOF; j++) L[i * DOF + j] = rel[i * DOF + j] + (i == j ? (i < D ? 1.0 / tau : 1.0 / (2.0 * kappa)) : 0.0);
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < DOF; j++) {
    double dj = L[j * DOF + j];
#pragma unroll
    for (int k = 0; k < DOF; k++)
      if (k < j) dj = fma(-L[j * DOF + k], L[j * DOF + k], dj);
    if (!(dj > 0.0)) return false;
    const double lj = sqrt(dj);
    L[j * DOF + j] = lj;
#pragma unroll
    for (int i = 0; i < DOF; i++)
      if (i > j) {
        double s = L[i * DOF + j];
#pragma unroll
        for (int k = 0; k < DOF; k++)
          if (k < j) s = fma(-L[i * DOF + k], L[j * DOF + k], s);
        L[i * DOF + j] = s / lj;
      }
    double zj = r[j];
#pragma unroll
    for (int k = 0; k < DOF; k++)
      if (k < j) zj = fma(-L[j * DOF + k], z[k], zj);
    z[j] = zj / lj;
    acc = fma(z[j], z[j], acc);
  }
  *d2 = acc;
  return true;
}

// One pair: rel (DOF x DOF) from the joint blocks and the records; with a candidate (cand != null) gate = (d^2, not_pd,
// residual[DOF]).
template <int D>
PAIRS_HD void pairs_one(const double *recp, const double *recq, const double *Spp, const double *Spq, const double *Sqq,
                        const double *cand, double *rel, double *gate) {
  constexpr int DOF = PairsDims<D>::DOF;
  double Rpq[D * D], tpq[D], J[DOF * 2 * DOF];
  pairs_relative<D>(recp, recq, Rpq, tpq);
  pairs_jacobian<D>(recp, Rpq, tpq, J);
  pairs_rel_cov<D>(J, Spp, Spq, Sqq, rel);
  if (!cand) return;
  double r[DOF], d2;
  pairs_residual<D>(Rpq, tpq, cand, r);
  const bool pd = pairs_mahalanobis<D>(rel, r, cand[D * D + D], cand[D * D + D + 1], &d2);
  gate[0] = d2;
  gate[1] = pd ? 0.0 : 1.0;
#pragma unroll
  for (int i = 0; i < DOF; i++) gate[2 + i] = r[i];
}

}  // namespace dpgo
