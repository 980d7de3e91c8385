"""numpy restatement of the robust objective behind the Newton polish and the covariances (dpgo_amd/csrc/robust.h): test
infrastructure, like tests/newton_restatement.py, tests/cov_restatement.py, tests/cert_restatement.py and
tests/edge_restatement.py, which it imports.  Nothing of the library is imported here.

    F(X) = 1/2 sum_intra s_e + 1/2 sum_inter rho(s_e),     w_e = rho'(s_e),     c_e = 2 rho''(s_e)
    M_w  = sum_e w_e M_e,      g = sum_e w_e g_e,          g_e[dof p + a] = tr(E_a(p)^T (M_e X)_p)
    H    = H(S_w) + sum_inter c_e g_e g_e^T,               S_w = M_w - blkdiag(0, Lambda_w(X))

A problem is a dict(d, N, I, J, R, t, kappa, tau, inter); X is in the reference layout ((d+1)N x d, t_p = row p, the rows of
Y_p = rows N + d p ..).  M_e = tau a a^T + kappa sum_r b_r b_r^T with a = e_{j,t} - e_{i,t} - sum_k t[k] e_{i,k} and
b_r = e_{j,r} - sum_k R[k, r] e_{i,k}, R R^T taken as the identity in the rotation block of pose i as the reference's assembly
does (DPGO_utils.cpp:1541-1641), so that sum_e M_e is the certificate's M: s_e = tr(X^T M_e X) are edge_restatement's residuals
for an orthogonal R, and a measured R that is orthogonal to six digits only changes neither g nor H (a symmetric change of a
pose's rotation block is absorbed by Lambda and drops out of every tangent trace).  Every function takes dtype:
np.float64 (plain numpy) or np.longdouble (the reference the device is held to).
"""
import numpy as np
import scipy.linalg as sla

import cert_restatement as cert
import cov_restatement as cr
import edge_restatement as er
import newton_restatement as nr
from oracle.problem import LOSS_GM, LOSS_HUBER, LOSS_NONE, LOSS_WELSCH

U = 2.0 ** -53
TINY = 2.0 ** -1074   # the spacing of the doubles below 2^-1022
CONVERGED, MAX_STEPS, STALLED = nr.CONVERGED, nr.MAX_STEPS, nr.STALLED


def problem(d, N, I, J, R, t, kappa, tau, num_nodes):
    I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
    return dict(d=d, N=N, I=I, J=J, R=np.asarray(R, np.float64), t=np.asarray(t, np.float64), kappa=np.asarray(kappa, np.float64),
                tau=np.asarray(tau, np.float64), inter=er.inter_mask(N, num_nodes, I, J), num_nodes=num_nodes)


def edges_of(P):
    return P["I"], P["J"], P["R"], P["t"], P["kappa"], P["tau"]


def edge_index(P):
    """(m, 2 (d+1)): the reference rows of [t_i, rows of Y_i, t_j, rows of Y_j]."""
    d, N = P["d"], P["N"]
    r = np.arange(d)
    return np.concatenate([P["I"][:, None], N + d * P["I"][:, None] + r, P["J"][:, None], N + d * P["J"][:, None] + r], axis=1)


def edge_matrices(P, dtype=np.float64, absolute=False):
    """(m, 2B, 2B): M_e on the rows of edge_index.  absolute=True: the same formula with every operand replaced by its absolute
    value -- the magnitudes of the terms an entry is made of, which the bounds need."""
    d, m = P["d"], len(P["I"])
    B = d + 1
    R, t = np.asarray(P["R"], dtype), np.asarray(P["t"], dtype)
    kappa, tau = np.asarray(P["kappa"], dtype), np.asarray(P["tau"], dtype)
    if absolute:
        R = np.abs(R)
    a = np.zeros((m, 2 * B), dtype)
    a[:, B] = 1
    a[:, 0] = -1
    a[:, 1:B] = -t
    if absolute:
        a = np.abs(a)
    Me = tau[:, None, None] * a[:, :, None] * a[:, None, :]
    for k in range(d):
        Me[:, 1 + k, 1 + k] += kappa
        Me[:, B + 1 + k, B + 1 + k] += kappa
        for c in range(d):
            Me[:, 1 + k, B + 1 + c] = (kappa * R[:, k, c]) * (1 if absolute else -1)
            Me[:, B + 1 + c, 1 + k] = Me[:, 1 + k, B + 1 + c]
    return Me


def weights(P, X, loss, delta, dtype=np.float64):
    """(s, rho, w, c) per edge."""
    sr, st = er.edge_s(*edges_of(P), X, dtype)
    s = sr + st
    inter = P["inter"]
    rho, w, c = s.copy(), np.ones_like(s), np.zeros_like(s)
    if loss != LOSS_NONE and inter.any():
        rho[inter], w[inter] = er.rho_w(s[inter], loss, delta, dtype)
        c[inter] = curvature(s[inter], w[inter], loss, delta, dtype)
    return s, rho, w, c


def curvature(s, w, loss, delta, dtype=np.float64):
    """c = 2 rho''(s) as a function of s and w = rho'(s); exactly 0 where w is exactly 0."""
    s, w, dl = np.asarray(s, dtype), np.asarray(w, dtype), dtype(delta)
    if loss == LOSS_NONE:
        return np.zeros_like(s)
    if loss == LOSS_HUBER:
        return np.where(s > dl, -w / np.where(s > dl, s, 1), 0)
    if loss == LOSS_GM:
        c = -4 * w / (s + dl)
    elif loss == LOSS_WELSCH:
        c = -2 * w / dl
    else:
        raise ValueError("loss")
    return np.where(w == 0, 0, c)


def objective(P, X, loss, delta, dtype=np.float64):
    s, rho, _, _ = weights(P, X, loss, delta, dtype)
    return 0.5 * np.sum(s[~P["inter"]]) + 0.5 * np.sum(rho[P["inter"]])


def weighted_matrix(P, w, dtype=np.float64):
    """M_w, dense, in the reference layout."""
    n = (P["d"] + 1) * P["N"]
    Me, idx = edge_matrices(P, dtype), edge_index(P)
    M = np.zeros((n, n), dtype)
    w = np.asarray(w, dtype)
    for e in range(len(idx)):
        M[np.ix_(idx[e], idx[e])] += w[e] * Me[e]
    return M


def edge_rows(P, X, dtype=np.float64):
    """(m, 2, d+1, d): the rows of (M_e X)_i and (M_e X)_j, the translation's first."""
    X = np.asarray(X, dtype)
    Me, idx = edge_matrices(P, dtype), edge_index(P)
    d = P["d"]
    Xe = X[idx]                                              # (m, 2B, d)
    out = np.zeros((len(idx), 2 * (d + 1), d), dtype)
    for k in range(2 * (d + 1)):                             # explicit sums: no long-double einsum
        out += Me[:, :, k, None] * Xe[:, k, None, :]
    return out.reshape(len(idx), 2, d + 1, d)


def generators(d):
    dof = cr.dof_of(d)
    return [-cr.hat(np.eye(dof - d)[k], d) for k in range(dof - d)]


def edge_ghat(P, X, dtype=np.float64, rows=None):
    """(m, 2, dof): g_e at the edge's pose i and at its pose j."""
    d, N = P["d"], P["N"]
    X = np.asarray(X, dtype)
    rows = edge_rows(P, X, dtype) if rows is None else np.asarray(rows, dtype)
    Y = X[N:].reshape(N, d, d)
    G = generators(d)
    out = np.zeros((len(P["I"]), 2, cr.dof_of(d)), dtype)
    for role, pose in enumerate((P["I"], P["J"])):
        out[:, role, :d] = rows[:, role, 0, :]
        for k, Gk in enumerate(G):
            Bk = np.zeros((len(pose), d, d), dtype)          # B_k(p) = -hat(e_k) Y_p
            for r in range(d):
                for q in range(d):
                    Bk[:, r, :] += dtype(Gk[r, q]) * Y[pose, q, :]
            out[:, role, d + k] = np.sum(np.sum(Bk * rows[:, role, 1:, :], axis=2), axis=1)
    return out


def tangent_basis(X, d, dtype=np.float64):
    """cov_restatement.tangent_basis in dtype."""
    X = np.asarray(X, dtype)
    N = X.shape[0] // (d + 1)
    dof = cr.dof_of(d)
    J = np.zeros((d, (d + 1) * N, dof * N), dtype)
    G = generators(d)
    for p in range(N):
        Y = X[N + d * p:N + d * p + d]
        for i in range(d):
            J[i, p, dof * p + i] = 1
        for k, Gk in enumerate(G):
            Bk = np.asarray(Gk, dtype) @ Y
            for c in range(d):
                J[c, N + d * p:N + d * p + d, dof * p + d + k] = Bk[:, c]
    return J


def project(S, X, d, dtype=np.float64):
    """sum_c J[c]^T S J[c] with J = tangent_basis(X), pose by pose (J is block diagonal): the same sums without the zeros."""
    X = np.asarray(X, dtype)
    N = X.shape[0] // (d + 1)
    dof = cr.dof_of(d)
    G = generators(d)
    rows = [np.concatenate([[p], N + d * p + np.arange(d)]) for p in range(N)]
    E = np.zeros((N, d, d + 1, dof), dtype)               # E[p, c][:, a] = column c of E_a(p)
    for p in range(N):
        Y = X[N + d * p:N + d * p + d]
        for i in range(d):
            E[p, i, 0, i] = 1
        for k, Gk in enumerate(G):
            Bk = np.asarray(Gk, dtype) @ Y
            for c in range(d):
                E[p, c, 1:, d + k] = Bk[:, c]
    H = np.zeros((dof * N, dof * N), dtype)
    for c in range(d):
        T = np.zeros((S.shape[0], dof * N), dtype)
        for q in range(N):
            T[:, dof * q:dof * q + dof] = S[:, rows[q]] @ E[q, c]
        for p in range(N):
            H[dof * p:dof * p + dof] += E[p, c].T @ T[rows[p]]
    return H


def add_rank1(P, H, ge_left, ge_right, coef):
    """H += sum_e coef_e u_e v_e^T for vectors given by their two pose blocks (m, 2, dof)."""
    dof = cr.dof_of(P["d"])
    for e in np.nonzero(coef)[0]:
        pose = (P["I"][e], P["J"][e])
        for a in range(2):
            for b in range(2):
                H[dof * pose[a]:dof * pose[a] + dof, dof * pose[b]:dof * pose[b] + dof] += coef[e] * ge_left[e, a][:, None] * ge_right[e, b][None, :]
    return H


def scatter(P, ge, coef, dtype=np.float64):
    """sum_e coef_e g_e as a vector of dof N."""
    dof = cr.dof_of(P["d"])
    g = np.zeros(dof * P["N"], dtype)
    for role, pose in enumerate((P["I"], P["J"])):
        for e in range(len(pose)):
            g[dof * pose[e]:dof * pose[e] + dof] += coef[e] * ge[e, role]
    return g


def grad(P, X, loss, delta, anchor=None, dtype=np.float64):
    _, _, w, _ = weights(P, X, loss, delta, dtype)
    g = scatter(P, edge_ghat(P, X, dtype), w, dtype)
    if anchor is not None:
        dof = cr.dof_of(P["d"])
        g[dof * anchor:dof * anchor + dof] = 0
    return g


def S_w(P, X, w, dtype=np.float64):
    """(M_w, S_w = M_w - blkdiag(0, Lambda_w(X))), dense."""
    d, N = P["d"], P["N"]
    X = np.asarray(X, dtype)
    M = weighted_matrix(P, w, dtype)
    MX = M @ X
    S = M.copy()
    for p in range(N):
        r = slice(N + d * p, N + d * p + d)
        Pm = MX[r] @ X[r].T
        S[r, r] -= (Pm + Pm.T) / 2
    return M, S


def full_edge_vectors(P, ge, dtype=np.float64):
    """(m, dof N): g_e as vectors."""
    dof = cr.dof_of(P["d"])
    V = np.zeros((len(P["I"]), dof * P["N"]), dtype)
    for e in range(len(P["I"])):
        V[e, dof * P["I"][e]:dof * P["I"][e] + dof] += ge[e, 0]
        V[e, dof * P["J"][e]:dof * P["J"][e] + dof] += ge[e, 1]
    return V


def hessian(P, X, loss, delta, curvature=1, anchor=None, dtype=np.float64, drop_rank1=()):
    """H, dense; anchored when anchor is given."""
    d = P["d"]
    X = np.asarray(X, dtype)
    _, _, w, c = weights(P, X, loss, delta, dtype)
    _, S = S_w(P, X, w, dtype)
    H = project(S, X, d, dtype)
    if curvature:
        ge = edge_ghat(P, X, dtype)
        c = np.array(c)
        c[list(drop_rank1)] = 0
        add_rank1(P, H, ge, ge, c)
    return H if anchor is None else anchored(H, anchor, cr.dof_of(d))


def anchored(H, anchor, dof):
    A = np.array(H)
    r = slice(dof * anchor, dof * anchor + dof)
    A[r, :] = 0
    A[:, r] = 0
    A[r, r] = np.eye(dof)
    return A


def polish_full(P, X, loss, delta, curvature=1, anchor=0, max_steps=20, max_tries=8, rel_tol=1e-9, grad_tol=0.0):
    """newton_restatement.polish_full with the robust F, g and H (fp64)."""
    d = P["d"]
    dof = cr.dof_of(d)
    X = np.array(X, dtype=np.float64)
    n = dof * P["N"]
    free = np.ones(n, bool)
    free[dof * anchor:dof * anchor + dof] = False
    mu = 0.0
    steps = factorisations = indefinite = 0
    log = []
    outcome = STALLED
    F_initial = grad_initial = None
    for k in range(max_steps + 1):
        g = grad(P, X, loss, delta, anchor)
        gn = float(np.linalg.norm(g))
        F0 = float(objective(P, X, loss, delta))
        H = hessian(P, X, loss, delta, curvature, anchor)
        hmax = nr.hmax_of(H, anchor, dof)
        if k == 0:
            F_initial, grad_initial = F0, gn
        mu_in = mu
        if gn <= (grad_tol if grad_tol > 0 else rel_tol * hmax):
            outcome = CONVERGED
            log.append((F0, gn, mu_in, 0.0, 0))
            break
        if k == max_steps:
            outcome = MAX_STEPS
            log.append((F0, gn, mu_in, 0.0, 0))
            break
        accepted = False
        tries = 0
        rho = 0.0
        for _ in range(max_tries):
            tries += 1
            A = H + mu * np.diag(free.astype(np.float64))
            factorisations += 1
            try:
                L = np.linalg.cholesky(A)
            except np.linalg.LinAlgError:
                if mu == 0.0:
                    indefinite += 1
                mu = max(10.0 * mu, 1e-3 * hmax)
                continue
            delta_x = -sla.cho_solve((L, True), g)
            Z = nr.retract(X, delta_x, d, anchor)
            F1 = float(objective(P, Z, loss, delta))
            pred = -0.5 * float(g @ delta_x) + 0.5 * mu * float(delta_x @ delta_x)
            rho = (F0 - F1) / pred if pred > 0 else -1.0
            if rho >= 0.1 or abs(F0 - F1) <= 1e-13 * abs(F0):
                X = Z
                accepted = True
                steps += 1
                if rho > 0.75:
                    mu = mu / 10.0
                    if mu < 1e-8 * hmax:
                        mu = 0.0
                break
            mu = max(10.0 * mu, 1e-3 * hmax)
        log.append((F0, gn, mu_in, rho if accepted else 0.0, tries))
        if not accepted:
            break
    log = np.array(log, dtype=np.float64).reshape(-1, 5)
    return dict(X=X, outcome=outcome, steps=steps, factorisations=factorisations, indefinite=indefinite, log=log, hmax=hmax,
                mu_final=mu, F_initial=F_initial, F_final=float(log[-1, 0]), grad_initial=grad_initial, grad_final=float(log[-1, 1]))


# ---- first-order bounds of the per-edge quantities, in the manner of edge_restatement.s_bound ----
def rows_bound(P, X):
    """(m, 2, d+1, d): the bound of every entry of the rows.  An entry of (M_e X) is a weight times a residual entry (a dot
    product of length d and up to two differences: d + 2 roundings against the magnitudes it is made of), and for pose i a
    second sum of d + 1 such products: 2 d + 6 roundings against the same formula on absolute values."""
    d = P["d"]
    Me = edge_matrices(P, np.longdouble, absolute=True)
    Xe = np.abs(np.asarray(X, np.longdouble))[edge_index(P)]
    out = np.zeros((len(P["I"]), 2 * (d + 1), d), np.longdouble)
    for k in range(2 * (d + 1)):
        out += Me[:, :, k, None] * Xe[:, k, None, :]
    return np.asarray((2 * d + 6) * U * out, np.float64).reshape(len(P["I"]), 2, d + 1, d)


def ghat_bound(P, X, rows_b):
    """(m, 2, dof): a translation entry is a row entry; a rotation entry a sum of 2 d products of an entry of Y (magnitude
    <= 1 + the rows' own error) with a row entry: the rows' bounds through the sum, plus 2 d + 1 roundings of the sum."""
    d, N = P["d"], P["N"]
    dof = cr.dof_of(d)
    rows_abs = np.abs(np.asarray(edge_rows(P, X, np.longdouble), np.float64))
    Y = np.abs(np.asarray(X, np.float64))[N:].reshape(N, d, d)
    G = [np.abs(g) for g in generators(d)]
    out = np.zeros((len(P["I"]), 2, dof))
    for role, pose in enumerate((P["I"], P["J"])):
        out[:, role, :d] = rows_b[:, role, 0, :]
        for k, Gk in enumerate(G):
            Bk = np.einsum("rq,eqc->erc", Gk, Y[pose])
            out[:, role, d + k] = np.sum(Bk * (rows_b[:, role, 1:, :] + (2 * d + 1) * U * rows_abs[:, role, 1:, :]), axis=(1, 2))
    return out


def c_bound(P, X, loss, delta):
    """The bound of c_e given the bound of s_e: |dc/ds| * bound(s) + 6 roundings of the formula; infinite inside the bound of
    s around Huber's kink (the tests' inputs keep every edge outside it).  Below 2^-1022 a result is rounded to a multiple of
    TINY = 2^-1074 whatever its size (Welsch's w on its way to exactly 0.0): w is then off by up to 2 TINY (an exponential is
    not correctly rounded), which c = f w multiplies by f = |dc/dw|, and c itself is rounded once more: (2 f + 1) TINY."""
    s, _, w, c = (np.asarray(a, np.float64) for a in weights(P, X, loss, delta, np.longdouble))
    sb = er.s_bound(*edges_of(P), X)[2]
    if loss == LOSS_NONE:
        return np.zeros_like(s)
    if loss == LOSS_HUBER:
        dc = 1.5 * np.abs(c) / np.maximum(s, delta)
        b = dc * sb + 6 * U * np.abs(c) + (2 / np.maximum(s, delta) + 1) * TINY
        b[np.abs(s - delta) <= sb] = np.inf
    elif loss == LOSS_GM:
        b = 3 * np.abs(c) / (s + delta) * sb + 6 * U * np.abs(c) + (8 / (s + delta) + 1) * TINY
    else:
        b = np.abs(c) / delta * sb + (6 + s / delta) * U * np.abs(c) + (4 / delta + 1) * TINY
    return np.where(P["inter"], b, 0.0)


def w_bound(P, X, loss, delta):
    """The bound of w_e given the bound of s_e: |dw/ds| bound(s) plus the relative rounding of the formula that
    edge_restatement.check_run allows (4 * 2^-52, and s / delta * 2^-52 more for Welsch's exponential)."""
    s, _, w, _ = (np.asarray(a, np.float64) for a in weights(P, X, loss, delta, np.longdouble))
    sb = er.s_bound(*edges_of(P), X)[2]
    if loss == LOSS_NONE:
        return np.zeros_like(s)
    rel = 8 * U + (2 * U * s / delta if loss == LOSS_WELSCH else 0.0)
    if loss == LOSS_HUBER:
        dw = np.where(s > delta - sb, w / (2 * np.maximum(s, delta)), 0.0)
    elif loss == LOSS_GM:
        dw = 2 * w / (s + delta)
    else:
        dw = w / delta
    return np.where(P["inter"], dw * sb + rel * w + 2 * TINY, 0.0)   # (TINY: see c_bound)


def reference(P, X, loss, delta, curvature=1, anchor=0):
    """Everything the device's debug calls are held against, in long double, with its first-order bounds (float64):
    dict(w, c, F, g, H, M, bw, bc, bF, bg, bH, bM).  The bounds follow the operands: the per-edge bounds above carried through
    the sums that use them, plus (terms + 2) roundings of every sum against the same sum on absolute values."""
    LD = np.longdouble
    d, N, m = P["d"], P["N"], len(P["I"])
    dof, B = cr.dof_of(d), d + 1
    n = B * N
    Xl = np.asarray(X, LD)
    s, rho, w, c = weights(P, Xl, loss, delta, LD)
    rows, ge = edge_rows(P, Xl, LD), None
    ge = edge_ghat(P, Xl, LD, rows)
    bw, bc = w_bound(P, X, loss, delta), (c_bound(P, X, loss, delta) if curvature else np.zeros(m))
    rb = rows_bound(P, X)
    gb = ghat_bound(P, X, rb)
    wa, ca = np.abs(np.asarray(w, np.float64)), np.abs(np.asarray(c, np.float64))
    rows_a, ge_a = np.abs(np.asarray(rows, np.float64)), np.abs(np.asarray(ge, np.float64))
    idx = edge_index(P)
    Me_a = edge_matrices(P, absolute=True)
    # M_w, entry by entry: the terms of an entry, their magnitudes, the weights' bounds
    Mabs, bMw, cnt = np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n))
    for e in range(m):
        ix = np.ix_(idx[e], idx[e])
        Mabs[ix] += wa[e] * Me_a[e]
        bMw[ix] += bw[e] * Me_a[e]
        cnt[ix] += Me_a[e] > 0
    bM = bMw + (cnt + 4) * U * Mabs                       # (an entry of M_e is itself up to d + 2 operations: 4 roundings)
    M, S = S_w(P, Xl, w, LD)
    # (M_w X) per pose: the rows' bounds and the weights' through the incidence sums
    deg = np.bincount(np.concatenate([P["I"], P["J"]]), minlength=N)
    bMX, MXa = np.zeros((N, B, d)), np.zeros((N, B, d))
    for role, pose in enumerate((P["I"], P["J"])):
        np.add.at(bMX, pose, wa[:, None, None] * rb[:, role] + bw[:, None, None] * rows_a[:, role])
        np.add.at(MXa, pose, wa[:, None, None] * rows_a[:, role])
    bMX += (deg[:, None, None] + 2) * U * MXa
    Ya = np.abs(np.asarray(X, np.float64))[N:].reshape(N, d, d)
    bL = bMX[:, 1:] @ Ya.transpose(0, 2, 1) + (d + 2) * U * (MXa[:, 1:] @ Ya.transpose(0, 2, 1))
    bL = 0.5 * (bL + bL.transpose(0, 2, 1))
    La = MXa[:, 1:] @ Ya.transpose(0, 2, 1)
    bS, Sabs = bM.copy(), Mabs.copy()
    for p in range(N):
        r = slice(N + d * p, N + d * p + d)
        bS[r, r] = (1 + 2 * U) * (bM[r, r] + bL[p]) + 2 * U * (Mabs[r, r] + La[p])
        Sabs[r, r] += La[p]
    Ja = np.abs(tangent_basis(X, d))
    bH = sum(Ja[k].T @ bS @ Ja[k] for k in range(d)) + 2 * (4 * d + 2) * U * sum(Ja[k].T @ Sabs @ Ja[k] for k in range(d))
    H = project(S, Xl, d, LD)
    if curvature:
        add_rank1(P, H, ge, ge, c)
        live = (ca != 0).astype(np.float64)
        add_rank1(P, bH, ge_a, ge_a, np.where(ca != 0, bc, 0.0))
        add_rank1(P, bH, gb, ge_a, ca)
        add_rank1(P, bH, ge_a, gb, ca)
        R1 = add_rank1(P, np.zeros((dof * N, dof * N)), ge_a, ge_a, ca)
        per_block = add_rank1(P, np.zeros((dof * N, dof * N)), np.ones_like(ge_a), np.ones_like(ge_a), live)
        bH += (per_block + 4) * U * R1
    # g: the tangent projection of M_w X
    g = scatter(P, ge, w, LD)
    bg = np.zeros(dof * N)
    for role, pose in enumerate((P["I"], P["J"])):
        for e in range(m):
            bg[dof * pose[e]:dof * pose[e] + dof] += wa[e] * gb[e, role] + bw[e] * ge_a[e, role] + (deg[pose[e]] + 2 * d + 3) * U * wa[e] * ge_a[e, role]
    if anchor is not None:
        r = slice(dof * anchor, dof * anchor + dof)
        H = anchored(H, anchor, dof)
        bH[r, :] = 0
        bH[:, r] = 0
        g[r] = 0
        bg[r] = 0
    inter = P["inter"]
    F = 0.5 * np.sum(s[~inter]) + 0.5 * np.sum(rho[inter])
    bF = m * float(np.max(er.s_bound(*edges_of(P), X)[2]))     # (tests/test_gpu_edges.py's tolerance of the summary)
    return dict(w=w, c=c, F=F, g=g, H=H, M=M, bw=bw, bc=bc, bF=bF, bg=bg, bH=bH, bM=bM, s=s, rho=rho)


def to_pose_major(A, N, d):
    """A matrix in the reference layout on the unknowns (d+1) g + r of cert_matrix."""
    B = d + 1
    perm = np.empty(B * N, np.int64)
    for g in range(N):
        perm[B * g] = g
        perm[B * g + 1:B * g + B] = N + d * g + np.arange(d)
    return A[np.ix_(perm, perm)]
