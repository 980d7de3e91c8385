// Marginal pose covariances: how uncertain is each pose at the point X the optimiser stopped at?
//
// The covariance of the poses relative to a fixed pose `anchor` is the inverse of the Riemannian Hessian of
// F = 1/2 tr(X^T M X) in tangent coordinates with the anchor's coordinates struck out (what g2o and GTSAM hand out as
// marginal covariances).  Here:
//
//  * Unknowns dof p + a, dof = d + d (d - 1) / 2 (6 for SE(3), 3 for SE(2)).  a < d: the translation increment
//    t_p + dt in the world frame; the rest: omega with R_p <- R_p Exp(hat(omega)) in the body frame, which on the record
//    is Ydot_p = -hat(omega) Y_p (Y_p = R_p^T).  hat is the standard one; hat(omega) = [[0, -omega], [omega, 0]] for d = 2.
//  * For every block (p, q) of the certificate's pattern (cert.h: one per pair of poses M couples)
//        H_pq[a, b] = tr(E_a(p)^T S_pq E_b(q)),   E_i = e_0 e_i^T (translation),   E_{d+k} = [0 ; -hat(e_k) Y_p] (rotation)
//    with S_pq the (d+1) x (d+1) block of S = M - blkdiag(0, Lambda(X)), no eta: H = J^T S J, the second derivative of F
//    along the retraction at a critical point.
//  * Gauge: the anchor's off-diagonal blocks are written as zeros and its diagonal block as the identity, so the pattern
//    stays the pose graph and the ordering on the quotient graph of `dof` consecutive unknowns stays exact; every
//    covariance block that involves the anchor is returned as zeros.
//  * k_cov_hessian (cov.hip) writes the dof x dof blocks straight into the value array of a second multifrontal factor
//    (spd.h) whose pattern is the certificate's with dof^2 instead of (d+1)^2 entries per block; the factor keeps W, and
//    spd_selinv_device turns it into the entries of H^-1 inside the factor's pattern -- which holds every diagonal block
//    and the block of every edge.
//
// The same restrictions as the certificate, for the same reasons: the trivial loss only (a group created with a robust loss
// returns -1: its S operator is not assembled, and the Hessian is that of the quadratic objective), and the group must host
// every node of the graph (-1 otherwise).  Covariances exist at any point where the anchored H is positive definite -- a
// local minimum whose certificate is NEGATIVE included; COV_NOT_PD is the answer where it is not.  `stationarity` = |S X|_F
// says whether X is a critical point at all.
#pragma once
#include <hip/hip_runtime.h>

#include "hess.h"

namespace dpgo {

enum { COV_OK = 0, COV_NOT_PD = 1, COV_SKIPPED = 2 };

// The analysis' numbers (hess.h); device_bytes: the numeric phase with its W / WT panels, the blocks of the selected inversion,
// the maps.  numeric_ms: host milliseconds from the launch of k_cov_hessian to the blocks of the inverse, ending in a
// synchronise.
struct CovResult : HessAnalysis {
  int outcome = COV_SKIPPED;
  double stationarity = 0, numeric_ms = 0;
  // numeric_ms taken apart -- factor_ms (hess.h): k_cov_hessian and the factorisation up to its verdict, selinv_ms: the selected
  // inversion up to a synchronise -- and the useful flops of its products, sum over the fronts of 2 u^2 w + 2 u w^2 + w^3
  double selinv_ms = 0, selinv_flops = 0;
};

constexpr int cov_dof(int d) { return d + d * (d - 1) / 2; }
// B_k(p) = -hat(e_k) Y_p has two non-zero rows: B_k[r1] = Y_p[r2], B_k[r2] = -Y_p[r1]  (d = 3: r1, r2 = k + 1, k + 2 mod 3;
// d = 2: the one generator, r1 = 0, r2 = 1).  Shared by cov.hip, polish.hip and robust_math.h.
template <int D>
__host__ __device__ __forceinline__ void cov_rot_rows(int k, int &r1, int &r2) {
  if (D == 3) {
    r1 = k == 2 ? 0 : k + 1;
    r2 = k == 0 ? 2 : k - 1;
  } else {
    r1 = 0;
    r2 = 1;
  }
}

// ---- kernel (cov.hip) ----
// out = H in the CSR order of the pose-major matrix with dof x dof blocks: the dof^2 nb_p values of pose p's rows are one
// run starting at dof^2 bptr[p] (row a, block j, column b at a dof nb_p + j dof + b).  Mval: M in the certificate's order
// ((d+1)^2 bptr[p] + r (d+1) nb_p + j (d+1) + c), bcol[k]: the pose of block k's columns, Lam: Lambda_p (d x d row-major),
// X: the pose records ((d+1) d doubles: t, then Y row-major).  anchor: the unified own row held fixed.
void launch_cov_hessian(int d, hipStream_t st, int nposes, const int *bptr, const int *bcol, const double *Mval, const double *Lam,
                        const double *X, int anchor, double *out);

}  // namespace dpgo
