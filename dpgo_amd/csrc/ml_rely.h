// Edge reliability and candidate gating on the measurements' full information matrices: rely.h's and pairs.h's questions asked
// of the maximum-likelihood objective (ml.h), so that d2_loo and the gate's d2 are chi-square quantities of dof degrees of
// freedom for an edge whose noise is anisotropic or couples translation with rotation, measured against the Omega that
// ml_polish minimised and ml_gnc thresholded.
//
// For an edge or candidate (p -> q) with residual r, Jacobian J = [J_p | J_q] (ml_math.h, as k_ml_edge<FULL> stores them at X),
// information Omega and Sigma_joint = [[S_pp, S_pq], [S_pq^T, S_qq]] from the factor of H = sum J^T Omega J (k_ml_hessian):
//     rel = J Sigma_joint J^T          the covariance of the predicted residual
//     C = Omega^-1 - rel               (an edge of the graph),   d2_loo = r^T C^-1 r,  r_loo = Omega^-1 C^-1 r, ... as rely.h
//     d2 = r^T (rel + Omega^-1)^-1 r   (a candidate that is not in the graph), as pairs.h
// evaluated in the whitened form of ml_rely_math.h, which never forms Omega^-1.  The records are rely.h's (rely_width(d)
// doubles; flag 2 does not occur: an Omega that is not positive definite is refused when the plan is built) and pairs.h's gate
// (2 + dof doubles).  sum_e redundancy_e = dof (m - N + 1) at ANY point: sum tr(Omega_e J_e Sigma J_e^T) = tr(Sigma H).
//
// Two kernels (ml_rely.hip): k_ml_rel, one thread per (edge, entry of rel's lower triangle), and k_ml_rely_edge, one lane per
// edge.  Everything upstream is reused: k_ml_edge<FULL> leaves r and [J_i | J_j | ...] on the device, k_ml_hessian writes H,
// the selected inversion with k_rely_gather or pairs_solve_joint deliver the three blocks (Group::rely_joint, rely.cpp).
//
// The restrictions are ml_covariance's: the trivial loss, one group hosting every node, the group's graph, every Omega_e
// symmetric positive definite.  The optimiser's state is not touched.
#pragma once
#include <hip/hip_runtime.h>

#include "rely.h"

namespace dpgo {

// ---- kernels (ml_rely.hip) ----
// rel (n x dof^2) <- J Sigma_joint J^T: listed edge k reads [J_p | J_q] at J + (idx ? idx[k] : k) ldj (the stored records: ldj =
// ml_jw_doubles(d)) and its blocks at joint + k 3 dof^2
void launch_ml_rel(int d, hipStream_t st, int n, const int *idx, const double *J, long long ldj, const double *joint, double *rel);
// rec <- ml_rely_one<d, sign> of every listed edge: rel at rel + k dof^2; Omega (dof^2) and r (dof) at index idx ? idx[k] : k of
// Om and r.  sign -1: n x rely_width(d) reliability records; +1: n x (2 + dof) gate records
void launch_ml_rely_edge(int d, int sign, hipStream_t st, int n, const int *idx, const double *rel, const double *Om, const double *r,
                         double *rec);

// host only: n edges through ml_rely_math.h -- J: n x 2 dof^2 ([J_p | J_q]), joint: n x 3 dof^2, Om: n x dof^2, r: n x dof;
// rel: n x dof^2, rec: n x (sign < 0 ? rely_width(d) : 2 + dof).  -1: bad sizes, or an Omega that is not positive definite
int ml_rely_edge_host(int d, int n, int sign, const double *J, const double *joint, const double *Om, const double *r, double *rel,
                      double *rec);
// the two kernels alone on the same (host) arrays, on the current device
int ml_rely_edge_device(int d, int n, int sign, const double *J, const double *joint, const double *Om, const double *r, double *rel,
                        double *rec);

}  // namespace dpgo
