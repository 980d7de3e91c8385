"""numpy restatement of graduated non-convexity on the maximum-likelihood objective (dpgo_amd/csrc/ml_gnc.h): test
infrastructure, like tests/gnc_restatement.py and tests/ml_restatement.py, which it imports.  Nothing of the library is
imported here.

    s_e = chi2_e = r_e' Omega_e r_e           (ml_restatement.edge)
    F_w(X)  = 1/2 sum_e w_e chi2_e,           F_mu(X) = 1/2 sum_{not R} chi2_e + 1/2 sum_R rho_mu(chi2_e)
    g_w = sum_e w_e J_e' Omega_e r_e,         H_w = sum_e w_e J_e' Omega_e J_e

weight_mu, rho_mu, the sums, the thresholds and the bound of w are gnc_restatement's, applied to s = chi2.  The loop is
gnc_restatement.run's with ml_restatement.polish_full on Omega_e scaled by w_e as the inner solve, and with the one change of
ml_gnc.h: an inner MAX_STEPS is a level like any other; only an inner STALLED is INNER_FAILED.

An edge of weight exactly 0 is taken out BY SELECTION (`weighted_edges`): its wr, its gradient terms and its record are
exact zeros whatever its residual holds.

Bounds of the weighted per-edge quantities (`weighted_bounds`), u = 2^-53: a weighted quantity w q, with q held by
ml_restatement.edge_bounds times its constant (tests/test_ml_host.py: CONSTANTS) and w by gnc_restatement.w_bound, gets
w bound(q) + bound(w) |q| + u |w q|.  No further constant is needed.
"""
import numpy as np

import gnc_restatement as gr
import ml_restatement as mr
import newton_restatement as nr

U = gr.U
LD = mr.LD
TLS, GM = gr.TLS, gr.GM
CONVERGED, ALL_INLIERS, MAX_LEVELS, INNER_FAILED, SKIPPED = gr.CONVERGED, gr.ALL_INLIERS, gr.MAX_LEVELS, gr.INNER_FAILED, gr.SKIPPED
DEFAULTS = dict(max_steps=20, max_tries=8, rel_tol=1e-9, grad_tol=0.0)   # the polish's


def scaled(E, w):
    """E with every Omega_e scaled by w_e (a zero weight gives a zero matrix: the restatement's sums then skip the edge exactly)."""
    out = dict(E)
    out["Om"] = np.asarray(E["Om"], np.float64) * np.asarray(w, np.float64)[:, None, None]
    return out


def chi2_theta(E, X, dtype=np.float64):
    """(chi2 (m), theta (m): the norm of the rotation residual, near_pi flags (m)) at X."""
    d, m = E["d"], len(E["I"])
    P = mr.poses_of(np.asarray(X, np.float64), d)
    c, th, near = np.zeros(m, dtype), np.zeros(m), np.zeros(m, bool)
    for e in range(m):
        r, _, _, near[e] = mr.edge(d, E["R"][e], E["t"][e], P[E["I"][e]], P[E["J"][e]], dtype)
        c[e] = r @ (np.asarray(E["Om"][e], dtype) @ r)
        th[e] = float(np.sqrt(r[d:] @ r[d:]))
    return c, th, near


def weighted_edges(E, X, w, dtype=np.float64, unweighted=None):
    """What a FULL pass writes, per edge: r, chi2 (unweighted), wr = w (Omega r), grad (m, 2, dof), Ji, Jj, Wi, Wj = w Omega J
    (m, dof, dof), near (m flags); the edges with w == 0 exact zeros in wr, grad and the four matrices, by selection.
    unweighted: an earlier call's result in the same dtype, whose unweighted part is then not computed again."""
    o = unweighted["unweighted"] if unweighted is not None else mr.edges_all(E, X, dtype)
    w = np.asarray(w, dtype)
    m = len(w)
    Om = np.asarray(E["Om"], dtype)
    out = dict(r=o["r"], chi2=o["chi2"], wr=np.zeros_like(o["wr"]), grad=np.zeros_like(o["grad"]), Ji=np.zeros_like(o["Ji"]),
               Jj=np.zeros_like(o["Jj"]), Wi=np.zeros_like(o["Ji"]), Wj=np.zeros_like(o["Jj"]))
    for e in range(m):
        if w[e] == 0:
            continue
        out["wr"][e] = w[e] * o["wr"][e]
        out["grad"][e] = w[e] * o["grad"][e]
        out["Ji"][e], out["Jj"][e] = o["Ji"][e], o["Jj"][e]
        out["Wi"][e], out["Wj"][e] = w[e] * (Om[e] @ o["Ji"][e]), w[e] * (Om[e] @ o["Jj"][e])
    out["near"] = unweighted["near"] if unweighted is not None else chi2_theta(E, X)[2]
    out["unweighted"] = o
    return out


def weighted_bounds(E, X, ref, w, bw, C):
    """Bounds of weighted_edges' outputs, the constants C of tests/test_ml_host.py (CONSTANTS) included.  ref: the long-double
    weighted_edges; w: the weights, bw: their own bound (0 where they are given).  r, chi2, Ji, Jj: C times edge_bounds' own.
    A weighted quantity w q:  w C b(q) + bw |q| + u |w q|  -- wr with q = Omega r; W with q = Omega J, whose bound is
    |Omega| C b(J) + dof u |Omega| |J| (tests/test_gpu_ml_ops.py); grad with q = J' Omega r, where the kernel scales Omega r
    before the product with J', so that the last term is u w |J|' |Omega r| (no cancellation).  Zero where w == 0."""
    un = ref["unweighted"]
    b = mr.edge_bounds(E, X, un)
    w = np.asarray(w, np.float64)
    bw = np.broadcast_to(np.asarray(bw, np.float64), w.shape)
    dof = mr.dof_of(E["d"])
    live = (w != 0).astype(np.float64)
    w1, w2, b1, b2, l2 = w[:, None], w[:, None, None], bw[:, None], bw[:, None, None], live[:, None, None]
    A = {k: np.abs(np.asarray(un[k], np.float64)) for k in ("wr", "grad", "Ji", "Jj")}
    out = dict(r=C["r"] * b["r"], chi2=C["chi2"] * b["chi2"])
    out["wr"] = (w1 * C["wr"] * b["wr"] + b1 * A["wr"] + U * w1 * A["wr"]) * live[:, None]
    nocancel = np.stack([np.einsum("eka,ek->ea", A[k], A["wr"]) for k in ("Ji", "Jj")], axis=1)
    out["grad"] = (w2 * C["grad"] * b["grad"] + b2 * A["grad"] + U * w2 * nocancel) * l2
    Om = np.abs(np.asarray(E["Om"], np.float64))
    for k, kw in (("Ji", "Wi"), ("Jj", "Wj")):
        q = Om @ A[k]
        bq = Om @ (C[k] * b[k]) + dof * U * q
        out[k] = C[k] * b[k] * l2
        out[kw] = (w2 * bq + b2 * q + U * w2 * q) * l2
    return out


def assemble_w(E, X, w, anchor=None, dtype=np.float64):
    """(F_w, g_w, H_w) as ml_restatement.assemble hands out (F, g, H), on Omega scaled by w."""
    return mr.assemble(scaled(E, w), X, anchor, dtype)


def sums(kind, mu, c2, chi2, w, R, near=None, dtype=np.float64):
    """gnc_restatement.sums on chi2, with near_pi (over w > 0) and near_pi_all."""
    s = gr.sums(kind, mu, c2, chi2, w, R, dtype)
    if near is not None:
        near = np.asarray(near, bool)
        s["near_pi"], s["near_pi_all"] = int(np.sum(near & (np.asarray(w) > 0))), int(np.sum(near))
    return s


def run(E, X, kind, c2, R, mu_step=1.4, max_levels=100, anchor=0, polish=None, **inner):
    """The loop of ml_gnc.h in float64.  R: the robust set (bool per edge).  Returns gnc_restatement.run's fields -- outcome, X,
    w, levels, log, mu_initial, mu_final, s_max_initial, steps, factorisations, inner (the inner outcomes of the levels 0 ..),
    num_outliers, margin (TLS: the smallest relative distance of a robust chi2_e(X_{k-1}) from either threshold), F_initial --
    plus decision_margin: the smallest ratio (distance of a deciding number from its alternative) / (its rounding bound) over
    the inner solves' decisions, and theta_max: the largest theta over the edges with w > 0 at any level's point.
    polish: the inner solve (default ml_restatement.polish_full; a stand-in must return its fields)."""
    m = len(E["I"])
    R = np.asarray(R, bool)
    opts = dict(DEFAULTS)
    opts.update(inner)
    polish = polish or mr.polish_full
    w = np.ones(m)
    out = dict(steps=0, factorisations=0, inner=[], levels=0, log=np.zeros((0, 10)), mu_initial=0.0, mu_final=0.0, margin=np.inf,
               decision_margin=np.inf, theta_max=0.0, s_max_initial=0.0)

    def solve(Xs, ws):
        r = polish(scaled(E, ws), Xs, anchor, **opts)
        out["steps"] += r["steps"]
        out["factorisations"] += r["factorisations"]
        out["inner"].append(r["outcome"])
        for _, dist, bound in r.get("decisions", ()):
            if bound > 0:
                out["decision_margin"] = min(out["decision_margin"], dist / bound)
        return r

    def look(Xs, ws):
        s, th, near = chi2_theta(E, Xs)
        if np.any(ws > 0):
            out["theta_max"] = max(out["theta_max"], float(np.max(th[ws > 0])))
        return s, near

    def done(outcome, Xf, wf, log=()):
        s, near = look(Xf, wf)
        out.update(outcome=outcome, X=Xf, w=wf, num_outliers=int(np.sum(s[R] > c2)), log=np.array(log, np.float64).reshape(-1, 10),
                   near_pi=int(np.sum(near & (wf > 0))), near_pi_all=int(np.sum(near)))
        return out

    r0 = solve(X, w)
    out["F_initial"] = r0["F_initial"]
    if r0["outcome"] == nr.STALLED:
        return done(INNER_FAILED, np.array(X, np.float64), w)
    Xk = r0["X"]
    s, _ = look(Xk, w)
    s_max = float(np.max(s[R])) if R.any() else 0.0
    out["s_max_initial"] = s_max
    if not R.any() or (kind == TLS and 2 * s_max <= c2):
        return done(ALL_INLIERS, Xk, w)
    mu = c2 / (2 * s_max - c2) if kind == TLS else max(1.0, 2 * s_max / c2)
    out["mu_initial"] = mu
    log = []
    outcome = MAX_LEVELS
    for k in range(1, max_levels + 1):
        w_prev = w
        w = w.copy()
        w[R] = gr.weight_rho(kind, mu, c2, s[R])[0]
        if kind == TLS:
            lo, hi = gr.thresholds(mu, c2)
            out["margin"] = min(out["margin"], float(np.min(np.abs(s[R] - lo) / lo)), float(np.min(np.abs(s[R] - hi) / hi)))
        before = gr.sums(kind, mu, c2, s, w, R)
        out["levels"], out["mu_final"] = k, mu
        rk = solve(Xk, w)
        if rk["outcome"] == nr.STALLED:
            return done(INNER_FAILED, Xk, w_prev, log)
        Xk = rk["X"]
        s, _ = look(Xk, w)
        after = gr.sums(kind, mu, c2, s, w, R)
        log.append((mu, before["F_mu"], before["F_w"], after["F_w"], after["F_mu"], rk["steps"], rk["outcome"], before["zero"],
                    before["one"], before["between"]))
        if (before["between"] == 0) if kind == TLS else (mu == 1.0):
            outcome = CONVERGED
            break
        mu = mu_step * mu if kind == TLS else max(mu / mu_step, 1.0)
    return done(outcome, Xk, w, log)
