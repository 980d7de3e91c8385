"""Restatement of the maximum-likelihood objective (dpgo_amd/csrc/ml.h): test infrastructure, like tests/newton_restatement.py,
which it imports.  Plain numpy / scipy; nothing of the library is imported here.

For an edge e = (i -> j) with measurement (R~, t~) and information Omega (dof x dof, translation first, then rotation):

    r_t = R~^T (R_i^T (t_j - t_i) - t~),   r_R = Log(R~^T R_i^T R_j)    (d = 2: the angle in (-pi, pi])
    F_ml = 1/2 sum r' Omega r,   g = sum J' Omega r,   H = sum J' Omega J   (Gauss-Newton)

in cov_restatement's unknowns (t_p + dt in the world frame, R_p <- R_p Exp(hat(omega)) in the body frame) with its anchor
convention.  Every function takes a dtype: np.float64, or cov_restatement.LD, in which the products, the sums and the Log run
in long double (the reference the device is held to).  X is in the reference layout: row p the translation of pose p, rows
N + d p ... the rows of Y_p = R_p^T.

The Levenberg-Marquardt rule is newton_restatement.polish_full's with the objective's three functions swapped; `decisions`
lists, for every branch the loop took, how far the deciding number was from the alternative and that number's rounding bound.

Rounding bounds (`edge_bounds`, `sum_bounds`): first-order, from the magnitudes of the inputs alone, in units of U = 2^-53; the
constant in front of each is measured in tests/test_ml_host.py as that file says and used by the GPU tests.
"""
import numpy as np

import cov_restatement as cr
import newton_restatement as nr

LD = cr.LD
U = 2.0 ** -53
SERIES_T2 = 1e-8
NEAR_PI = 1e-3


def dof_of(d):
    return cr.dof_of(d)


def hat3(w, dtype):
    z = dtype(0)
    return np.array([[z, -w[2], w[1]], [w[2], z, -w[0]], [-w[1], w[0], z]], dtype=dtype)


def edge(d, R, t, Xi, Xj, dtype=np.float64):
    """(r (dof), Ji, Jj (dof x dof), near_pi) of one edge.  Xi, Xj: (t_p, Y_p) of its poses."""
    dof = dof_of(d)
    R, t = np.asarray(R, dtype), np.asarray(t, dtype)
    ti, Yi = np.asarray(Xi[0], dtype), np.asarray(Xi[1], dtype)
    tj, Yj = np.asarray(Xj[0], dtype), np.asarray(Xj[1], dtype)
    u = Yi @ (tj - ti)
    A = R.T @ Yi
    E = A @ Yj.T
    r = np.zeros(dof, dtype)
    Ji, Jj = np.zeros((dof, dof), dtype), np.zeros((dof, dof), dtype)
    r[:d] = R.T @ (u - t)
    Ji[:d, :d] = -A
    Jj[:d, :d] = A
    if d == 2:
        Ji[:d, 2] = R.T @ np.array([u[1], -u[0]], dtype=dtype)
        th = np.arctan2((E[1, 0] - E[0, 1]) / 2, (E[0, 0] + E[1, 1]) / 2)
        r[2] = th
        Ji[2, 2], Jj[2, 2] = -1, 1
        return r, Ji, Jj, bool(abs(th) > np.pi - NEAR_PI)
    Ji[:d, d:] = R.T @ hat3(u, dtype)
    a = np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]], dtype=dtype) / 2
    sn = np.sqrt(a @ a)
    cs = (np.trace(E) - 1) / 2
    th = np.arctan2(sn, cs)
    t2 = th * th
    if t2 < SERIES_T2:   # (the long-double reference carries one more term of each series: 1e-16 relative is fp64's unit)
        scale = 1 + t2 / 6 + 7 * t2 * t2 / 360
        c = dtype(1) / 12 + t2 / 720 + t2 * t2 / 30240
    else:
        scale = th / sn
        c = 1 / t2 - (1 + cs) / (2 * th * sn)
    p = scale * a
    Jr = np.eye(3, dtype=dtype) + hat3(p, dtype) / 2 + c * (np.outer(p, p) - (p @ p) * np.eye(3, dtype=dtype))
    r[d:] = p
    Jj[d:, d:] = Jr
    Ji[d:, d:] = -Jr.T @ R.T
    return r, Ji, Jj, bool(th > np.pi - NEAR_PI)


def poses_of(X, d):
    N = X.shape[0] // (d + 1)
    return [(X[p], X[N + d * p:N + d * p + d]) for p in range(N)]


def edges_all(E, X, dtype=np.float64):
    """Per edge of E = dict(d, I, J, R, t, Om): r, wr, chi2, Ji, Jj, grad (m, 2, dof), blocks (m, 4, dof, dof), near_pi."""
    d, m = E["d"], len(E["I"])
    dof = dof_of(d)
    P = poses_of(np.asarray(X, np.float64), d)
    o = {"r": np.zeros((m, dof), dtype), "wr": np.zeros((m, dof), dtype), "chi2": np.zeros(m, dtype),
         "Ji": np.zeros((m, dof, dof), dtype), "Jj": np.zeros((m, dof, dof), dtype), "grad": np.zeros((m, 2, dof), dtype),
         "blocks": np.zeros((m, 4, dof, dof), dtype), "near_pi": 0}
    for e in range(m):
        r, Ji, Jj, near = edge(d, E["R"][e], E["t"][e], P[E["I"][e]], P[E["J"][e]], dtype)
        Om = np.asarray(E["Om"][e], dtype)
        wr = Om @ r
        o["r"][e], o["wr"][e], o["chi2"][e], o["Ji"][e], o["Jj"][e] = r, wr, r @ wr, Ji, Jj
        o["grad"][e, 0], o["grad"][e, 1] = Ji.T @ wr, Jj.T @ wr
        J = (Ji, Jj)
        for ab in range(4):
            o["blocks"][e, ab] = J[ab >> 1].T @ Om @ J[ab & 1]
        o["near_pi"] += near
    return o


def assemble(E, X, anchor=None, dtype=np.float64, per_edge=None):
    """(F_ml, g (dof N), H (dof N x dof N dense)); with an anchor its gradient entries are zero and its rows and columns of H
    the identity's."""
    d = E["d"]
    dof = dof_of(d)
    N = X.shape[0] // (d + 1)
    o = per_edge if per_edge is not None else edges_all(E, X, dtype)
    g, H = np.zeros(dof * N, dtype), np.zeros((dof * N, dof * N), dtype)
    for e in range(len(E["I"])):
        pq = (int(E["I"][e]), int(E["J"][e]))
        for a in range(2):
            g[dof * pq[a]:dof * pq[a] + dof] += o["grad"][e, a]
            for b in range(2):
                H[dof * pq[a]:dof * pq[a] + dof, dof * pq[b]:dof * pq[b] + dof] += o["blocks"][e, 2 * a + b]
    F = o["chi2"].sum() / 2
    if anchor is not None:
        g[dof * anchor:dof * anchor + dof] = 0
        H = np.asarray(cr.anchored(H, anchor, dof), dtype)
    return F, g, H


def objective(E, X, dtype=np.float64):
    d = E["d"]
    P = poses_of(np.asarray(X, np.float64), d)
    F = dtype(0)
    for e in range(len(E["I"])):
        r = edge(d, E["R"][e], E["t"][e], P[E["I"][e]], P[E["J"][e]], dtype)[0]
        F += r @ (np.asarray(E["Om"][e], dtype) @ r)
    return F / 2


def omega_iso(d, kappa, tau):
    """diag(tau I_d, 2 kappa I): the matrix for which F_ml and the project's F agree to second order in the residual."""
    dof = dof_of(d)
    Om = np.zeros((len(kappa), dof, dof))
    for k in range(dof):
        Om[:, k, k] = tau if k < d else 2 * np.asarray(kappa)
    return Om


# ---------------------------------------------------------------------------------------------------------------
# rounding bounds, in units of their constants (tests/test_ml_host.py: CONSTANTS)
# ---------------------------------------------------------------------------------------------------------------
def edge_bounds(E, X, ref):
    """Per output of edges_all the first-order rounding bound of an fp64 evaluation, from the inputs' magnitudes and the
    long-double values `ref` alone.  r_t: a dot product of length d on |t_j - t_i| (its subtraction included) and |t~|, then one
    of length d with R~; r_R: two products of rotations (entries <= 1) and atan2 (relative), so 1 + theta, times theta / sin theta for
    d = 3, where phi = (theta / sin theta) a carries the absolute error of a's entries.  J: its entries are products of those
    quantities, (1 + |t_j - t_i| + theta) theta / sin theta; structural zeros and the d = 2 rotation entries carry no error.  The
    rest is propagated through |Omega| and |J| with the length of each dot product."""
    d, m = E["d"], len(E["I"])
    dof = dof_of(d)
    P = poses_of(np.asarray(X, np.float64), d)
    b = {k: np.zeros(np.shape(ref[k]), np.float64) for k in ("r", "wr", "chi2", "Ji", "Jj", "grad", "blocks")}
    for e in range(m):
        dt = float(np.linalg.norm(P[E["J"][e]][0] - P[E["I"][e]][0]))
        tn = float(np.linalg.norm(E["t"][e]))
        r, wr = np.abs(np.asarray(ref["r"][e], np.float64)), np.abs(np.asarray(ref["wr"][e], np.float64))
        th = float(np.linalg.norm(r[d:]))
        Om = np.abs(np.asarray(E["Om"][e], np.float64))
        cond = th / np.sin(th) if d == 3 and th > 1e-4 else 1.0   # Log's conditioning: phi = (theta / sin theta) a
        br = np.concatenate([np.full(d, 2 * d * U * (dt + tn)), np.full(dof - d, 2 * d * U * (1 + th) * cond)])
        bJ = 2 * d * U * (1 + dt + th) * cond
        J = [np.abs(np.asarray(ref[k][e], np.float64)) for k in ("Ji", "Jj")]
        bJm = [np.where(j > 0, bJ, 0.0) for j in J]
        if d == 2:
            for x in bJm:
                x[2, 2] = 0.0
        bwr = Om @ br + dof * U * (Om @ r)
        b["r"][e], b["wr"][e] = br, bwr
        b["chi2"][e] = r @ bwr + br @ wr + dof * U * (r @ (Om @ r))
        b["Ji"][e], b["Jj"][e] = bJm
        for a in range(2):
            b["grad"][e, a] = J[a].T @ bwr + bJm[a].T @ wr + dof * U * (J[a].T @ wr)
            for c in range(2):
                b["blocks"][e, 2 * a + c] = (bJm[a].T @ Om @ J[c] + J[a].T @ Om @ bJm[c] + 2 * dof * U * (J[a].T @ Om @ J[c]))
    return b


def sum_bounds(E, N, ref, eb):
    """(bound of F_ml, of g (dof N), of H (dense)) from the per-edge bounds eb and the long-double per-edge values ref: the
    terms' own bounds, plus U times the number of additions times the sum of the terms' magnitudes."""
    d, m = E["d"], len(E["I"])
    dof = dof_of(d)
    bg, bH = np.zeros(dof * N), np.zeros((dof * N, dof * N))
    cnt_g, cnt_H = np.zeros(dof * N), np.zeros((dof * N, dof * N))
    ag, aH = np.zeros(dof * N), np.zeros((dof * N, dof * N))
    for e in range(m):
        pq = (int(E["I"][e]), int(E["J"][e]))
        for a in range(2):
            s = slice(dof * pq[a], dof * pq[a] + dof)
            bg[s] += eb["grad"][e, a]
            ag[s] += np.abs(np.asarray(ref["grad"][e, a], np.float64))
            cnt_g[s] += 1
            for c in range(2):
                s2 = slice(dof * pq[c], dof * pq[c] + dof)
                bH[s, s2] += eb["blocks"][e, 2 * a + c]
                aH[s, s2] += np.abs(np.asarray(ref["blocks"][e, 2 * a + c], np.float64))
                cnt_H[s, s2] += 1
    chi2 = np.abs(np.asarray(ref["chi2"], np.float64))
    bF = 0.5 * float(eb["chi2"].sum()) + 0.5 * U * (np.ceil(np.log2(max(m, 2))) + 6) * float(chi2.sum())
    return bF, bg + U * cnt_g * ag, bH + U * cnt_H * aH


# ---------------------------------------------------------------------------------------------------------------
# the Levenberg-Marquardt rule (newton_restatement.polish_full with F_ml, g and the Gauss-Newton H)
# ---------------------------------------------------------------------------------------------------------------
def polish_full(E, X, anchor=0, max_steps=20, max_tries=8, rel_tol=1e-9, grad_tol=0.0):
    """As newton_restatement.polish_full; `decisions`: per branch taken (kind, distance of the deciding number from the
    alternative, the rounding bound of that number)."""
    import scipy.linalg as sla
    d = E["d"]
    dof = dof_of(d)
    X = np.array(X, dtype=np.float64)
    N = X.shape[0] // (d + 1)
    n = dof * N
    free = np.ones(n, bool)
    free[dof * anchor:dof * anchor + dof] = False
    mu = 0.0
    steps = factorisations = indefinite = 0
    log, rounding, decisions = [], [], []
    outcome = nr.STALLED
    F_initial = grad_initial = None

    def f_bound(Z):
        ref = edges_all(E, Z, LD)
        return sum_bounds(E, N, ref, edge_bounds(E, Z, ref))

    for k in range(max_steps + 1):
        F0, g, H = assemble(E, X, anchor)
        F0 = float(F0)
        bF0, bg, _ = f_bound(X)
        gn = float(np.linalg.norm(g))
        bgn = float(np.linalg.norm(bg))
        hmax = nr.hmax_of(H, anchor, dof)
        if k == 0:
            F_initial, grad_initial = F0, gn
        mu_in = mu
        tol = grad_tol if grad_tol > 0 else rel_tol * hmax
        decisions.append(("converged", abs(gn - tol), bgn))
        if gn <= tol:
            outcome = nr.CONVERGED
            log.append((F0, gn, mu_in, 0.0, 0))
            rounding.append(False)
            break
        if k == max_steps:
            outcome = nr.MAX_STEPS
            log.append((F0, gn, mu_in, 0.0, 0))
            rounding.append(False)
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
            delta = -sla.cho_solve((L, True), g)
            Z = nr.retract(X, delta, d, anchor)
            F1 = float(objective(E, Z))
            bF1 = f_bound(Z)[0]
            pred = -0.5 * float(g @ delta) + 0.5 * mu * float(delta @ delta)
            rho = (F0 - F1) / pred if pred > 0 else -1.0
            by_rounding = abs(F0 - F1) <= 1e-13 * abs(F0)
            # the accept test in F's own units: F0 - F1 against 0.1 pred (and against the rounding clause's 1e-13 |F0|)
            decisions.append(("accept", min(abs((F0 - F1) - 0.1 * pred), abs(abs(F0 - F1) - 1e-13 * abs(F0))) if pred > 0
                              else abs(abs(F0 - F1) - 1e-13 * abs(F0)), bF0 + bF1))
            if rho >= 0.1 or by_rounding:
                X = Z
                accepted = True
                steps += 1
                rounding.append(bool(by_rounding and not rho >= 0.1))
                if rho > 0.75:
                    decisions.append(("shrink", abs((F0 - F1) - 0.75 * pred), bF0 + bF1))
                    mu = mu / 10.0
                    if mu < 1e-8 * hmax:
                        mu = 0.0
                else:
                    decisions.append(("keep", abs((F0 - F1) - 0.75 * pred), bF0 + bF1))
                break
            mu = max(10.0 * mu, 1e-3 * hmax)
        log.append((F0, gn, mu_in, rho if accepted else 0.0, tries))
        if not accepted:
            rounding.append(False)
            break
    log = np.array(log, dtype=np.float64).reshape(-1, 5)
    return dict(X=X, outcome=outcome, steps=steps, factorisations=factorisations, indefinite=indefinite, log=log,
                rounding=rounding, hmax=hmax, mu_final=mu, F_initial=F_initial, F_final=float(log[-1, 0]),
                grad_initial=grad_initial, grad_final=float(log[-1, 1]), decisions=decisions)
