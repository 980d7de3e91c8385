"""Restatement of the joint pair covariances and the loop-closure gate (dpgo_amd/csrc/pairs.h, pairs_math.h): test
infrastructure in the style of tests/cov_restatement.py, whose layout, hat map and retraction it uses.  Plain numpy; nothing of
the library is imported here.  Every function takes a dtype: np.float64 is "what ordinary fp64 reaches", np.longdouble the
reference.

Coordinates (cov.h).  Per pose dof = d + d (d - 1) / 2 tangent coordinates: dt in the world frame, omega in the body frame,
R <- R Exp(hat(omega)).  X is in the reference layout: row p the translation, rows N + d p ... the rows of Y_p = R_p^T.

The relative pose T_pq = T_p^-1 T_q:   R_pq = R_p^T R_q = Y_p Y_q^T,   t_pq = R_p^T (t_q - t_p) = Y_p (t_q - t_p),
perturbed the same way (t_pq + dt_pq, R_pq Exp(hat(domega_pq))).  To first order
    domega_pq = omega_q - R_pq^T omega_p,      dt_pq = R_p^T (dt_q - dt_p) + hat(t_pq) omega_p
(d = 2: R_pq^T omega_p = omega_p and the last term is -omega_p [[0, -1], [1, 0]] t_pq), i.e.
    J = [J_p  J_q],   J_p = [[-Y_p, hat(t_pq)], [0, -R_pq^T]],   J_q = [[Y_p, 0], [0, I]],   Sigma_rel = J Sigma_joint J^T.
tests/test_pairs_host.py holds J against the central difference of (t_pq, Log) along cov_restatement.retract: that, not this
paragraph, is the judge of signs and frames.

The gate.  A candidate (R~, t~, kappa, tau): r = [t_pq - t~ ; vee Log(R~^T R_pq)], Omega = blkdiag(tau I_d, 2 kappa I_{dof-d})
-- the Hessian of 1/2 (kappa |R_pq - R~|_F^2 + tau |t_pq - t~|^2) in (dt_pq, domega_pq) at zero residual --
S = Sigma_rel + Omega^-1, d^2 = r^T S^-1 r.

The margins (u = 2^-53), fixed here before any device is asked, to first order in u:
  joint blocks   bS: tests/test_gpu_covariance.py's bound of an entry of the inverse, C u kappa_2 |A^-1|_2 plus
                 |A^-1|_2^2 | bound of the matrix |_2 for the Hessian's own error.  It is an input of what follows.
  J              only hat(t_pq) and R_pq^T are computed: |dt_pq| <= e_t = (d + 2) u |Y_p| |t_q - t_p| (one subtraction, d
                 products, d - 1 additions), |dR_pq| <= e_R = (d + 1) u |Y_p| |Y_q|^T.  EJ holds them in J's pattern.
  Sigma_rel      m_rel = |J| (bS 11^T) |J|^T + EJ |Sigma| |J|^T + |J| |Sigma| EJ^T + (4 dof + 2) u |J| |Sigma| |J|^T
                 (the blocks' error through J; J's error; two chained sums of 2 dof products each).
  r              translation: e_t + u |t_pq - t~|.  rotation: E = R~^T R_pq has |dE| <= eE = e_R through |R~|^T plus
                 (d + 1) u |R~|^T |R_pq|; Log moves by |dw / dE| eE (the partials of the restated Log, central differences in
                 long double) plus 4 u |w| for atan2 and the division.
  d^2            with z = S^-1 r:  2 |z|^T m_r + |z|^T (m_rel + u |S|) |z| + 4 (dof + 1) u kappa_2(S) d^2  (the residual's error,
                 S's error, the Cholesky and the substitution in registers).
tests/test_pairs_host.py asserts that the fp64 restatement stays within a quarter of m_rel and m_d2 on every fixture -- the two
margins whose leading term is the modelled bS -- and inside m_r.  m_r has no modelled term: on the translation it is the plain
count of roundings (one subtraction, d products, d - 1 additions: at most d + 1 on any path, d + 2 taken) times
|Y_p| |t_q - t_p|, and fp64 realises up to 1.8 of those roundings on the fixtures (0.36 of m_r).  No term is missing there,
and a count of five roundings has no factor of four in reserve; it is kept as counted.
"""
import numpy as np

import cov_restatement as cr

LD = cr.LD
U = cr.U


def record(X, d, p, dtype=np.float64):
    """(t_p, Y_p) of pose p from the reference layout."""
    N = X.shape[0] // (d + 1)
    return np.asarray(X[p], dtype), np.asarray(X[N + d * p:N + d * p + d], dtype)


def relative(X, d, p, q, dtype=np.float64):
    tp, Yp = record(X, d, p, dtype)
    tq, Yq = record(X, d, q, dtype)
    return Yp @ Yq.T, Yp @ (tq - tp)


def hat(w, d, dtype=np.float64):
    return np.asarray(cr.hat(np.asarray(w, np.float64), d), dtype) if dtype == np.float64 else _hat_ld(w, d)


def _hat_ld(w, d):
    w = np.asarray(w, LD)
    if d == 2:
        return np.array([[0, -w[0]], [w[0], 0]], LD)
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], LD)


def jacobian(X, d, p, q, dtype=np.float64):
    """J (dof x 2 dof) = [J_p  J_q]."""
    dof = cr.dof_of(d)
    _, Yp = record(X, d, p, dtype)
    Rpq, tpq = relative(X, d, p, q, dtype)
    J = np.zeros((dof, 2 * dof), dtype)
    J[:d, :d] = -Yp
    J[:d, dof:dof + d] = Yp
    if d == 3:
        J[:d, d:dof] = hat(tpq, d, dtype)
        J[d:, d:dof] = -Rpq.T
    else:
        J[:d, d] = -(np.array([[0, -1], [1, 0]], dtype) @ tpq)
        J[d, d] = -1
    J[d:, dof + d:] = np.eye(dof - d, dtype=dtype)
    return J


def joint_of(Sigma, dof, p, q, anchor=None):
    """[[S_pp, S_pq], [S_pq^T, S_qq]] from a dense inverse on the unknowns dof g + a; the anchor's blocks are zero."""
    rp, rq = slice(dof * p, dof * p + dof), slice(dof * q, dof * q + dof)
    S = np.block([[Sigma[rp, rp], Sigma[rp, rq]], [Sigma[rq, rp], Sigma[rq, rq]]])
    if p == anchor:
        S[:dof, :] = 0
        S[:, :dof] = 0
    if q == anchor:
        S[dof:, :] = 0
        S[:, dof:] = 0
    return S


def blocks_of(Sj, dof):
    """(3, dof, dof): S_pp, S_pq, S_qq of a joint matrix, as the library hands them out."""
    return np.stack([Sj[:dof, :dof], Sj[:dof, dof:], Sj[dof:, dof:]])


def joint_from_blocks(B):
    return np.block([[B[0], B[1]], [B[1].T, B[2]]])


def rel_cov(J, Sj):
    return J @ Sj @ J.T


def log_so(E, d, dtype=np.float64):
    """vee Log(E): the angle for d = 2; theta / sin(theta) times vee(E - E^T) / 2 for d = 3 (theta away from pi)."""
    E = np.asarray(E, dtype)
    if d == 2:
        return np.array([np.arctan2(E[1, 0], E[0, 0])], dtype)
    v = np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]], dtype) / 2
    c = (np.trace(E) - 1) / 2
    s = np.sqrt(v @ v)
    theta = np.arctan2(s, c)
    if s < 1e-8:
        assert c > 0, "the restatement does not take logarithms next to pi"
        return v * (1 + theta * theta / 6)
    return v * (theta / s)


def exp_so(w, d, dtype=LD):
    """Exp(hat(w)) by Rodrigues, in dtype."""
    w = np.asarray(w, dtype)
    if d == 2:
        c, s = np.cos(w[0]), np.sin(w[0])
        return np.array([[c, -s], [s, c]], dtype)
    th = np.sqrt(w @ w)
    K = hat(w, d, dtype)
    if th < 1e-12:
        return np.eye(3, dtype=dtype) + K
    return np.eye(3, dtype=dtype) + (np.sin(th) / th) * K + ((1 - np.cos(th)) / (th * th)) * (K @ K)


def residual(X, d, p, q, cand, dtype=np.float64):
    Rt, tt = np.asarray(cand[0], dtype), np.asarray(cand[1], dtype)
    Rpq, tpq = relative(X, d, p, q, dtype)
    return np.concatenate([tpq - tt, log_so(Rt.T @ Rpq, d, dtype)])


def omega(d, kappa, tau, dtype=np.float64):
    dof = cr.dof_of(d)
    return np.diag(np.asarray([tau] * d + [2 * kappa] * (dof - d), dtype))


def gate(rel, r, d, kappa, tau, dtype=np.float64):
    """(S, z = S^-1 r, d^2)."""
    S = np.asarray(rel, dtype) + np.diag(1 / np.diag(omega(d, kappa, tau, dtype)))
    if dtype == np.float64:
        z = np.linalg.solve(S, r)
    else:
        import factor_restatement as fr
        L, kstar, _ = fr.cholesky_ld((S + S.T) / 2)
        assert kstar < 0
        Li = fr.lower_inverse_ld(L)
        z = Li.T @ (Li @ r)
    return S, z, r @ z


def edge_term(X, d, p, q, cand):
    """1/2 (kappa |R_pq - R~|_F^2 + tau |t_pq - t~|^2) in long double: one edge's own term of F."""
    Rpq, tpq = relative(X, d, p, q, LD)
    Rt, tt, kappa, tau = cand
    return 0.5 * (kappa * np.sum((Rpq - np.asarray(Rt, LD)) ** 2) + tau * np.sum((tpq - np.asarray(tt, LD)) ** 2))


def pair_tangent(N, d, p, q, vp, vq):
    """The tangent vector (dof N) that moves pose p by vp and pose q by vq (p == q: by their sum)."""
    dof = cr.dof_of(d)
    v = np.zeros(dof * N)
    v[dof * p:dof * p + dof] += vp
    v[dof * q:dof * q + dof] += vq
    return v


# ---------------------------------------------------------------------------------------------------------------
# the margins
# ---------------------------------------------------------------------------------------------------------------
def jacobian_error(X, d, p, q):
    """(EJ in J's pattern, e_t, e_R)."""
    dof = cr.dof_of(d)
    tp, Yp = record(X, d, p)
    tq, Yq = record(X, d, q)
    e_t = (d + 2) * U * (np.abs(Yp) @ np.abs(tq - tp))
    e_R = (d + 1) * U * (np.abs(Yp) @ np.abs(Yq).T)
    EJ = np.zeros((dof, 2 * dof))
    if d == 3:
        EJ[0, d + 1], EJ[0, d + 2] = e_t[2], e_t[1]
        EJ[1, d + 0], EJ[1, d + 2] = e_t[2], e_t[0]
        EJ[2, d + 0], EJ[2, d + 1] = e_t[1], e_t[0]
        EJ[d:, d:dof] = e_R.T
    else:
        EJ[0, d], EJ[1, d] = e_t[1], e_t[0]
    return EJ, e_t, e_R


def margin_rel(X, d, p, q, Sj, bS):
    dof = cr.dof_of(d)
    J = np.abs(jacobian(X, d, p, q))
    EJ = jacobian_error(X, d, p, q)[0]
    Sa = np.abs(np.asarray(Sj, np.float64))
    return J @ np.full((2 * dof, 2 * dof), bS) @ J.T + EJ @ Sa @ J.T + J @ Sa @ EJ.T + (4 * dof + 2) * U * (J @ Sa @ J.T)


def margin_residual(X, d, p, q, cand):
    dof = cr.dof_of(d)
    _, e_t, e_R = jacobian_error(X, d, p, q)
    Rt, tt = np.asarray(cand[0], np.float64), np.asarray(cand[1], np.float64)
    Rpq, tpq = relative(X, d, p, q)
    m = np.zeros(dof)
    m[:d] = e_t + U * np.abs(tpq - tt)
    eE = np.abs(Rt).T @ e_R + (d + 1) * U * (np.abs(Rt).T @ np.abs(Rpq))
    E = np.asarray(Rt, LD).T @ np.asarray(relative(X, d, p, q, LD)[0], LD)
    w = log_so(E, d, LD)
    h = LD(1e-7)
    dw = np.zeros(dof - d)
    for i in range(d):
        for j in range(d):
            Ep, Em = E.copy(), E.copy()
            Ep[i, j] += h
            Em[i, j] -= h
            dw += np.asarray(np.abs(log_so(Ep, d, LD) - log_so(Em, d, LD)) / (2 * h), np.float64) * eE[i, j]
    m[d:] = dw + 4 * U * np.asarray(np.abs(w), np.float64)
    return m


def margin_d2(rel, r, d, kappa, tau, m_rel, m_r):
    dof = cr.dof_of(d)
    S, z, d2 = gate(np.asarray(rel, np.float64), np.asarray(r, np.float64), d, kappa, tau)
    za = np.abs(z)
    lam = np.linalg.eigvalsh((S + S.T) / 2)
    assert lam[0] > 0
    return float(2 * za @ m_r + za @ (m_rel + U * np.abs(S)) @ za + 4 * (dof + 1) * U * (lam[-1] / lam[0]) * abs(d2))
