"""Restatement of the edge reliability and the candidate gate on the full information matrices (dpgo_amd/csrc/ml_rely.h,
ml_rely_math.h): test infrastructure on top of tests/ml_restatement.py (edge, assemble), in the style of
tests/rely_restatement.py.  Plain numpy; nothing of the library is imported here.  np.longdouble is the reference.

For an edge or candidate (p -> q) with residual r, Jacobians J_p, J_q (ml_restatement.edge), information Omega and the joint
covariance Sj = [[S_pp, S_pq], [S_pq^T, S_qq]] of its poses from the inverse of the anchored H = sum J' Omega J:

    rel = [J_p | J_q] Sj [J_p | J_q]^T
    Omega = L L^T,   A = L^T rel L,   rho = L^T r                          (A from the LOWER triangle of rel, mirrored)
    d2_own = rho' rho,   redundancy = dof - tr A,   redundancy_trans = d - sum_{a<d} (Omega rel)_aa
    sign -1:  Q = I - A,  zeta = Q^-1 rho,  d2_loo = rho' zeta,  r_loo = L^-T zeta,  influence = zeta' A zeta
    sign +1:  Q = I + A,  d2 = rho' Q^-1 rho

The record of sign -1 is rely_restatement's [d2_loo, flag, redundancy, redundancy_trans, d2_own, influence, r, r_loo], flag 1
where a pivot of Q's Cholesky factor is not > 0 (d2_loo, influence, r_loo zeros); of sign +1 [d2, not_pd, r].  `classical`
evaluates the textbook forms r' (Omega^-1 -+ rel)^-1 r with an explicit inverse: tests/test_ml_rely_host.py holds the two against
each other, and d2_loo and r_loo against graphs re-solved without the edge -- that, not this paragraph, is the judge.

The margins (U = 2^-53), first order, in 2-norms of the WHITENED quantities, which are O(1) whatever the scale of Omega.  With
m_rel (entrywise) and m_r the bounds of the inputs' own errors (None: exact inputs):
  e_Om  = (dof + 1) U || |L^-1| (|L| |L|^T) |L^-T| ||        the factorisation of Omega, whitened
  e_A   = || |L|^T m_rel |L| || + (2 dof + 2) U || |L|^T |rel| |L| || + 2 e_Om ||A||
  e_rho = || |L|^T m_r || + (dof + 1) U || |L|^T |r| || + e_Om ||rho||
  d2 (either sign)   2 ||zeta|| e_rho + ||zeta||^2 (e_A + U ||Q||) + 4 (dof + 1) U kappa_2(Q) d2     (rely_restatement's argument)
  zeta               m_z = ||Q^-1|| (e_rho + (e_A + U ||Q||) ||zeta||) + 4 (dof + 1) U kappa_2(Q) ||zeta||
  r_loo              ||L^-T|| (m_z + e_Om ||zeta||) + (dof + 1) U |L^-T| |zeta|                      (entrywise)
  influence          2 m_z ||A|| ||zeta|| + ||zeta||^2 e_A + (2 dof + 2) U ||zeta||^2 ||A||
  redundancy         tr(|L|^T m_rel |L|) + (2 dof + 2) U tr(|L|^T |rel| |L|) + 2 e_Om tr|A| + U |redundancy|
  redundancy_trans   sum_{a<d} (|Omega| m_rel)_aa + (dof + 2) U sum_{a<d} (|Omega| |rel|)_aa + U |redundancy_trans|
  d2_own             2 ||rho|| e_rho + (dof + 2) U d2_own
  a pivot of Q       (e_A + (dof + 1) U ||Q||) (1 + |w|^2), w = Q_11^-1 q the leading block's solve (d_j = v' Q v, v = (-w, 1))
  rel (exact J, Sj)  5 dof U |J| |Sj| |J|^T                                                          (entrywise: rel_margin)
What the factorisation's and the inversion's own rounding moves rel and the redundancy sum by is bounded in the SCALED sense, the
one that does not see the scale of Omega: a Cholesky factorisation with its two triangular solves is the exact one of H + dH
with |dH_ij| <= (3 n + 1) U sqrt(H_ii H_jj) (Higham, Accuracy and Stability of Numerical Algorithms, theorems 10.3 and 10.4 with
|R^T| |R|_ij <= sqrt(H_ii H_jj)), so to first order dSigma = -Sigma dH Sigma and, with h = sqrt(diag H) and G = J_full Sigma
(dof x n, the anchor's columns zero),
  rel (Sigma's part)     (3 n + 1) U (|G| h) (|G| h)^T                                               (entrywise: rel_margin_sigma)
  the redundancy sum     sum_e tr(Omega_e J_e dSigma J_e^T) = -tr(dH Sigma):   (3 n + 1) U h^T |Sigma| h          (sum_margin_sigma)
The selected inversion is a recursion over the same factor, no deeper than n; its rounding has the same form.
Nothing in them comes from the library.  `bound` puts a constant in front of the rounding part of each field; the constants
are measured in tests/test_ml_rely_host.py as that file says.
"""
import numpy as np

import cov_restatement as cr

LD = cr.LD
U = 2.0 ** -53
FAULTS = ("sign", "l_transposed", "transpose", "diag_omega", "trace")
FIELDS = ("d2", "redundancy", "redundancy_trans", "d2_own", "influence", "r_loo")


def width(d, sign=-1):
    return 6 + 2 * cr.dof_of(d) if sign < 0 else 2 + cr.dof_of(d)


def joint_matrix(blocks, dtype=LD):
    """(2 dof, 2 dof) from the library's (3, dof, dof) = S_pp, S_pq, S_qq."""
    b = np.asarray(blocks, dtype)
    return np.block([[b[0], b[1]], [b[1].T, b[2]]])


def rel_of(Ji, Jj, Sj, dtype=LD, fault=None):
    """J Sj J^T.  fault "transpose": S_pq read transposed."""
    dof = np.shape(Ji)[0]
    Sj = np.array(Sj, dtype)
    if fault == "transpose":
        Sj[:dof, dof:], Sj[dof:, :dof] = Sj[:dof, dof:].T.copy(), Sj[dof:, :dof].T.copy()
    J = np.concatenate([np.asarray(Ji, dtype), np.asarray(Jj, dtype)], axis=1)
    return J @ Sj @ J.T


def mirrored(rel):
    """rel as the library defines it where Sj is symmetric to rounding only (the blocks of batched solves): entry (a, b), a >= b,
    of J Sj J^T, written to both places."""
    return np.tril(rel) + np.tril(rel, -1).T


def rel_margin(Ji, Jj, Sj):
    """The rounding bound of rel's entries for exact J and Sj, in units of its constant."""
    dof = np.shape(Ji)[0]
    J = np.abs(np.concatenate([np.asarray(Ji, np.float64), np.asarray(Jj, np.float64)], axis=1))
    return 5 * dof * U * (J @ np.abs(np.asarray(Sj, np.float64)) @ J.T)


def cholesky(A, dtype):
    """(L, pivots): the lower Cholesky factor in dtype, row by row; behind a pivot that is not > 0 the rest of L is not
    computed and the pivot list ends with it."""
    n = A.shape[0]
    L = np.zeros((n, n), dtype)
    piv = []
    for j in range(n):
        dj = A[j, j] - L[j, :j] @ L[j, :j]
        piv.append(dj)
        if not dj > 0:
            return L, piv
        L[j, j] = np.sqrt(dj)
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    return L, piv


def lower_solve(L, b, transpose=False):
    n = L.shape[0]
    x = np.array(b, L.dtype)
    if not transpose:
        for i in range(n):
            x[i] = (x[i] - L[i, :i] @ x[:i]) / L[i, i]
    else:
        for i in range(n - 1, -1, -1):
            x[i] = (x[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def record(rel, Om, r, d, sign=-1, dtype=LD, fault=None):
    """The definitions in dtype: a dict of the record's fields plus L, A, rho, Q, zeta and the pivots of Q."""
    dof = cr.dof_of(d)
    rel, Om, r = np.asarray(rel, dtype), np.asarray(Om, dtype), np.asarray(r, dtype)
    if fault == "diag_omega":
        Om = np.diag(np.diag(Om))
    low = np.tril(rel) + np.tril(rel, -1).T   # (the library reads rel's lower triangle)
    L, pl = cholesky(Om, dtype)
    assert len(pl) == dof and pl[-1] > 0, "Omega is not positive definite"
    if fault == "l_transposed":
        A, rho = L @ low @ L.T, L @ r
    else:
        A, rho = L.T @ low @ L, L.T @ r
    s = -sign if fault == "sign" else sign
    Q = np.eye(dof, dtype=dtype) + s * A
    out = dict(sign=sign, flag=0, r=r, d2=dtype(0), d2_own=rho @ rho, influence=dtype(0), r_loo=np.zeros(dof, dtype),
               redundancy=dof - (np.trace(low) if fault == "trace" else np.trace(A)),
               redundancy_trans=d - (np.trace(low[:d, :d]) if fault == "trace" else np.trace((Om @ low)[:d, :d])),
               L=L, A=A, rho=rho, Q=Q, zeta=None, low=low, Om=Om)
    K, piv = cholesky(Q, dtype)
    out["pivots"] = piv
    if not piv[-1] > 0:
        out["flag"] = 1
        return out
    zeta = lower_solve(K, lower_solve(K, rho), transpose=True)
    out.update(zeta=zeta, d2=rho @ zeta)
    if sign < 0:
        out.update(r_loo=lower_solve(L, zeta, transpose=True), influence=zeta @ A @ zeta)
    return out


def classical(rel, Om, r, sign=-1):
    """r' (Omega^-1 + sign rel)^-1 r with an explicit long-double inverse of Omega: rely.h's and pairs.h's own forms."""
    rel, Om, r = np.asarray(rel, LD), np.asarray(Om, LD), np.asarray(r, LD)
    low = np.tril(rel) + np.tril(rel, -1).T
    Li = lower_solve(cholesky(Om, LD)[0], np.eye(len(r), dtype=LD))
    C = Li.T @ Li + sign * low
    K, piv = cholesky(C, LD)
    assert piv[-1] > 0
    y = lower_solve(K, r)
    return y @ y


def vector(rec, d):
    """The record as the library lays it out, in long double."""
    if rec["sign"] > 0:
        return np.concatenate([[rec["d2"], LD(rec["flag"])], np.asarray(rec["r"], LD)]).astype(LD)
    return np.concatenate([[rec["d2"], LD(rec["flag"]), rec["redundancy"], rec["redundancy_trans"], rec["d2_own"], rec["influence"]],
                           np.asarray(rec["r"], LD), np.asarray(rec["r_loo"], LD)]).astype(LD)


def fields(d, sign=-1):
    """The field (a key of the constants; None: the flag and r, which carry no rounding of this arithmetic) of every entry."""
    dof = cr.dof_of(d)
    if sign > 0:
        return ["d2", None] + [None] * dof
    return ["d2", None, "redundancy", "redundancy_trans", "d2_own", "influence"] + [None] * dof + ["r_loo"] * dof


def _n2(M):
    return float(np.linalg.norm(np.asarray(M, np.float64), 2))


def margins(rec, d, m_rel=None, m_r=None):
    """(margin of every entry of vector(rec, d), margin of every pivot of Q that was computed), given the margins of rel and
    r (None: exact inputs).  The flag's margin is zero; r's is m_r."""
    dof = cr.dof_of(d)
    sign = rec["sign"]
    m = np.zeros(width(d, sign))
    m_rel = np.zeros((dof, dof)) if m_rel is None else np.asarray(m_rel, np.float64)
    m_r = np.zeros(dof) if m_r is None else np.asarray(m_r, np.float64)
    f64 = lambda x: np.asarray(x, np.float64)   # noqa: E731
    L, A, rho, Q, low, Om = (f64(rec[k]) for k in ("L", "A", "rho", "Q", "low", "Om"))
    La, r = np.abs(L), np.abs(f64(rec["r"]))
    Li = np.linalg.inv(L)
    e_Om = (dof + 1) * U * _n2(np.abs(Li) @ (La @ La.T) @ np.abs(Li).T)
    wm, wr = La.T @ m_rel @ La, La.T @ np.abs(low) @ La
    e_A = _n2(wm) + (2 * dof + 2) * U * _n2(wr) + 2 * e_Om * _n2(A)
    e_rho = float(np.linalg.norm(La.T @ m_r)) + (dof + 1) * U * float(np.linalg.norm(La.T @ r)) + e_Om * float(np.linalg.norm(rho))
    nQ = _n2(Q)
    m_piv = []
    for j in range(len(rec["pivots"])):
        w = np.linalg.solve(Q[:j, :j], Q[:j, j]) if j else np.zeros(0)
        m_piv.append((e_A + (dof + 1) * U * nQ) * (1 + float(w @ w)))
    off = 2 if sign > 0 else 6
    m[off:off + dof] = m_r
    if sign < 0:
        m[2] = np.trace(wm) + (2 * dof + 2) * U * np.trace(wr) + 2 * e_Om * np.trace(np.abs(A)) + U * abs(float(rec["redundancy"]))
        Oa = np.abs(Om)
        m[3] = (np.trace((Oa @ m_rel)[:d, :d]) + (dof + 2) * U * np.trace((Oa @ np.abs(low))[:d, :d]) +
                U * abs(float(rec["redundancy_trans"])))
        m[4] = 2 * float(np.linalg.norm(rho)) * e_rho + (dof + 2) * U * float(rec["d2_own"])
    if rec["flag"] == 1:
        return m, np.array(m_piv)
    zeta = f64(rec["zeta"])
    nz = float(np.linalg.norm(zeta))
    lam = np.linalg.eigvalsh((Q + Q.T) / 2)
    kap, qinv = float(lam[-1] / lam[0]), 1 / float(lam[0])
    m[0] = 2 * nz * e_rho + nz * nz * (e_A + U * nQ) + 4 * (dof + 1) * U * kap * abs(float(rec["d2"]))
    if sign < 0:
        m_z = qinv * (e_rho + (e_A + U * nQ) * nz) + 4 * (dof + 1) * U * kap * nz
        m[5] = 2 * m_z * _n2(A) * nz + nz * nz * e_A + (2 * dof + 2) * U * nz * nz * _n2(A)
        m[6 + dof:] = _n2(Li) * (m_z + e_Om * nz) + (dof + 1) * U * (np.abs(Li).T @ np.abs(zeta))
    return m, np.array(m_piv)


def bound(rec, d, constants, m_rel=None, m_r=None):
    """(the bound of every entry, of every pivot): the inputs' part as it is, the rounding part times the field's constant
    (pivots: the constant of d2)."""
    full, fp = margins(rec, d, m_rel, m_r)
    rnd, rp = margins(rec, d)
    c = np.array([constants[f] if f else 1.0 for f in fields(d, rec["sign"])])
    return full + (c - 1) * rnd, fp + (constants["d2"] - 1) * rp


def decided(rec, piv_bound):
    """Whether every pivot of Q the restatement computed sits at least 4 of its bounds from zero: the flag is then not
    rounding's to decide."""
    return bool(np.all(np.abs(np.asarray(rec["pivots"], np.float64)) >= 4 * np.asarray(piv_bound)))


def rel_margin_sigma(Ji, Jj, Sigma, h, p, q, anchor):
    """What the rounding of Sigma's computation moves rel by (entrywise, first order): see the module's docstring."""
    dof = np.shape(Ji)[0]
    n = len(h)
    S = np.array(Sigma, np.float64)
    S[dof * anchor:dof * anchor + dof, :] = 0
    S[:, dof * anchor:dof * anchor + dof] = 0
    G = np.asarray(Ji, np.float64) @ S[dof * p:dof * p + dof] + np.asarray(Jj, np.float64) @ S[dof * q:dof * q + dof]
    g = np.abs(G) @ np.asarray(h, np.float64)
    return (3 * n + 1) * U * np.outer(g, g)


def sum_margin_sigma(Sigma, h, anchor, dof):
    """What the rounding of Sigma's computation moves the sum of all redundancies by."""
    n = len(h)
    S = np.abs(np.array(Sigma, np.float64))
    S[dof * anchor:dof * anchor + dof, :] = 0
    S[:, dof * anchor:dof * anchor + dof] = 0
    return (3 * n + 1) * U * float(h @ S @ h)


def inverse(H):
    """The long-double inverse of a symmetric positive definite matrix through its Cholesky factor."""
    import factor_restatement as fr
    A = np.asarray(H, LD)
    L, kstar, _ = fr.cholesky_ld(0.5 * (A + A.T))
    assert kstar < 0
    Xi = fr.lower_inverse_ld(L)
    return Xi.T @ Xi


def edge_inputs(E, X, Sigma, anchor, per_edge, dtype=LD, fault=None, edges=None):
    """Per listed edge of E (None: all): dict(p, q, Ji, Jj, Sj, rel, r, Om) in dtype from the dense Sigma (anchor's blocks
    zeroed) and ml_restatement.edges_all's per_edge values."""
    import pairs_restatement as pr
    dof = cr.dof_of(E["d"])
    out = []
    for e in (range(len(E["I"])) if edges is None else edges):
        p, q = int(E["I"][e]), int(E["J"][e])
        Sj = np.asarray(pr.joint_of(np.asarray(Sigma), dof, p, q, anchor), dtype)
        Ji, Jj = np.asarray(per_edge["Ji"][e], dtype), np.asarray(per_edge["Jj"][e], dtype)
        out.append(dict(e=e, p=p, q=q, Ji=Ji, Jj=Jj, Sj=Sj, rel=rel_of(Ji, Jj, Sj, dtype, fault), r=np.asarray(per_edge["r"][e], dtype),
                        Om=np.asarray(E["Om"][e], dtype)))
    return out
