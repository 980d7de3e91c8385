"""Restatement of the per-edge reliability records (dpgo_amd/csrc/rely.h, rely_math.h): test infrastructure in the style of
tests/pairs_restatement.py, whose relative pose, Jacobian, residual and Omega it uses.  Plain numpy; nothing of the library is
imported here.  np.longdouble is the reference.

For an edge (p, q) with its own measurement (R~, t~, kappa, tau) taken as pairs_restatement's candidate, and Sigma_rel, r, Omega as
there:
    C = Omega^-1 - Sigma_rel,   z = C^-1 r,   d2_loo = r^T z,   r_loo = Omega^-1 z,   influence = z^T Sigma_rel z,
    redundancy = dof - sum_i Omega_ii rel_ii,   redundancy_trans = d - tau sum_{i<d} rel_ii,   d2_own = r^T Omega r,
C from the LOWER triangle of Sigma_rel (which is symmetric up to rounding: C is Omega^-1 - rel after cancellation, so which
triangle is read matters at the level of the margins below when the inputs are taken as exact), influence from all of it;
flag 1 where C is not positive definite (d2_loo, influence and r_loo are then zeros), 2 where kappa or tau is not > 0 (all zeros).
The library's record is [d2_loo, flag, redundancy, redundancy_trans, d2_own, influence, r[dof], r_loo[dof]] (vector()).

Why these: with H = H_rest + J^T Omega J the Hessian and H_rest that of the graph without the edge, Woodbury gives
J H_rest^-1 J^T = rel + rel (Omega^-1 - rel)^-1 rel, the Gauss-Newton step of the reduced problem from X is dx = Sigma J^T Omega
(I - rel Omega)^-1 r, the edge's residual after it r + J dx = Omega^-1 C^-1 r, the drop of the optimum 1/2 r^T C^-1 r, and
dx^T H dx = z^T rel z.  tests/test_rely_host.py holds that against re-solved graphs: that, not this paragraph, is the judge.

The margins (u = 2^-53), to first order, from the margins m_rel (entrywise) and m_r of pairs_restatement -- nothing in them comes
from the library:
  d2_loo           2 |z|^T m_r + |z|^T (m_rel + u |C|) |z| + 4 (dof + 1) u kappa_2(C) d2_loo      (margin_d2's argument on C)
  z                m_z = |C^-1| (m_r + (m_rel + u |C|) |z|) + 4 (dof + 1) u kappa_2(C) |z|_2      (dz = C^-1 (dr - dC z), and
                   the Cholesky solve in registers)
  r_loo            Omega^-1 m_z + u |r_loo|
  influence        2 m_z^T |rel| |z| + |z|^T m_rel |z| + (2 dof + 2) u |z|^T |rel| |z|
  redundancy       sum_i Omega_ii m_rel,ii + (dof + 2) u sum_i Omega_ii |rel_ii| + u |redundancy|      (and with d, tau for
                   redundancy_trans).  The last term is the rounding of the result itself: dof - s is one fp64 number, within
                   u |redundancy| of the exact difference whatever computes it, and for a well-checked edge (s small beside
                   dof) no multiple of u s covers that -- on the d = 2 ladder, with exact inputs, a correctly rounded
                   redundancy_trans is up to 11 times the first two terms away from the long-double value.
  d2_own           2 sum_i Omega_ii |r_i| m_r,i + (dof + 2) u d2_own
"""
import numpy as np

import cov_restatement as cr
import factor_restatement as fr
import pairs_restatement as pr

LD = pr.LD
U = pr.U
FAULTS = ("plus", "kappa", "no_omega", "trace", "transpose")


def width(d):
    return 6 + 2 * cr.dof_of(d)


def candidate_of(mm, e):
    """(R~, t~, kappa, tau) of edge e of an oracle Measurements."""
    return np.asarray(mm.R[e]), np.asarray(mm.t[e]), float(mm.kappa[e]), float(mm.tau[e])


def rel_and_r(X, d, p, q, cand, Sj, dtype=LD, fault=None):
    """(Sigma_rel, r) of an edge from the joint covariance Sj (2 dof x 2 dof).  fault "transpose": S_pq read transposed."""
    dof = cr.dof_of(d)
    Sj = np.array(Sj, dtype)
    if fault == "transpose":
        Sj[:dof, dof:], Sj[dof:, :dof] = Sj[:dof, dof:].T.copy(), Sj[dof:, :dof].T.copy()
    return pr.rel_cov(pr.jacobian(X, d, p, q, dtype), Sj), pr.residual(X, d, p, q, cand, dtype)


def record(rel, r, d, kappa, tau, fault=None):
    """The definitions in long double: a dict of the record's fields plus C, z, lam_min (of C, fp64) and omega_min."""
    dof = cr.dof_of(d)
    rel, r = np.asarray(rel, LD), np.asarray(r, LD)
    out = dict(d2_loo=LD(0), flag=0, redundancy=LD(0), redundancy_trans=LD(0), d2_own=LD(0), influence=LD(0), r=np.zeros(dof, LD),
               r_loo=np.zeros(dof, LD), C=None, z=None, lam_min=None, omega_min=None)
    if not (kappa > 0) or not (tau > 0):
        out["flag"] = 2
        return out
    om = np.diag(pr.omega(d, kappa, tau, LD)).copy()
    if fault == "kappa":
        om[d:] = LD(kappa)
    low = np.tril(rel) + np.tril(rel, -1).T   # (the library factors the lower triangle of C; rel is symmetric to rounding only)
    C = np.diag(1 / om) + low if fault == "plus" else np.diag(1 / om) - low
    out["r"] = r
    out["redundancy"] = dof - (np.trace(rel) if fault == "trace" else np.sum(om * np.diag(rel)))
    out["redundancy_trans"] = d - (np.trace(rel[:d, :d]) if fault == "trace" else LD(tau) * np.sum(np.diag(rel)[:d]))
    out["d2_own"] = np.sum(om * r * r)
    lam = np.linalg.eigvalsh(np.asarray(C, np.float64))
    out.update(C=C, lam_min=float(lam[0]), lam_max=float(lam[-1]), omega_min=float(om.min()))
    L, kstar, _ = fr.cholesky_ld(C)
    if kstar >= 0:
        out["flag"] = 1
        return out
    Li = fr.lower_inverse_ld(L)
    z = Li.T @ (Li @ r)
    out.update(z=z, Cinv=Li.T @ Li, d2_loo=r @ z, r_loo=z if fault == "no_omega" else z / om, influence=z @ rel @ z)
    return out


def vector(rec, d):
    """The record as the library lays it out, in long double."""
    return np.concatenate([[rec["d2_loo"], LD(rec["flag"]), rec["redundancy"], rec["redundancy_trans"], rec["d2_own"], rec["influence"]],
                           np.asarray(rec["r"], LD), np.asarray(rec["r_loo"], LD)]).astype(LD)


def margins(rec, rel, d, kappa, tau, m_rel=None, m_r=None):
    """The margin of every entry of vector(rec, d) (the flag's is zero), given the margins of rel and r (None: exact inputs)."""
    dof = cr.dof_of(d)
    m = np.zeros(width(d))
    if rec["flag"] == 2:
        return m
    m_rel = np.zeros((dof, dof)) if m_rel is None else np.asarray(m_rel, np.float64)
    m_r = np.zeros(dof) if m_r is None else np.asarray(m_r, np.float64)
    om = np.diag(pr.omega(d, kappa, tau))
    ra = np.abs(np.asarray(rel, np.float64))
    r = np.abs(np.asarray(rec["r"], np.float64))
    m[2] = np.sum(om * np.diag(m_rel)) + (dof + 2) * U * np.sum(om * np.diag(ra)) + U * abs(float(rec["redundancy"]))
    m[3] = tau * np.sum(np.diag(m_rel)[:d]) + (d + 2) * U * tau * np.sum(np.diag(ra)[:d]) + U * abs(float(rec["redundancy_trans"]))
    m[4] = 2 * np.sum(om * r * m_r) + (dof + 2) * U * float(rec["d2_own"])
    m[6:6 + dof] = m_r
    if rec["flag"] == 1:
        return m
    C = np.abs(np.asarray(rec["C"], np.float64))
    za = np.abs(np.asarray(rec["z"], np.float64))
    kap = rec["lam_max"] / rec["lam_min"]
    dC = m_rel + U * C
    m[0] = 2 * za @ m_r + za @ dC @ za + 4 * (dof + 1) * U * kap * abs(float(rec["d2_loo"]))
    m_z = np.abs(np.asarray(rec["Cinv"], np.float64)) @ (m_r + dC @ za) + 4 * (dof + 1) * U * kap * float(np.linalg.norm(za))
    m[6 + dof:] = m_z / om + U * np.abs(np.asarray(rec["r_loo"], np.float64))
    m[5] = 2 * m_z @ ra @ za + za @ m_rel @ za + (2 * dof + 2) * U * (za @ ra @ za)
    return m


def decided(rec):
    """Whether the restated sign of lambda_min(C) is beyond what rounding decides: |lambda_min(C)| min Omega_ii >= 1e-6."""
    return rec["flag"] == 2 or abs(rec["lam_min"]) * rec["omega_min"] >= 1e-6
