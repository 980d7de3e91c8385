"""numpy restatement of graduated non-convexity (dpgo_amd/csrc/gnc.h): test infrastructure, like tests/robust_restatement.py and
tests/newton_restatement.py, which it imports.  Nothing of the library is imported here.

    F_w(X)  = 1/2 sum_e w_e s_e,        F_mu(X) = 1/2 sum_{not R} s_e + 1/2 sum_R rho_mu(s_e)
    TLS:  s <= mu/(mu+1) c2: w = 1, rho = s;   s >= (mu+1)/mu c2: w = 0, rho = c2;   otherwise
          w = sqrt(c2 (mu (mu+1)) / s) - mu (clamped to [0, 1]),   rho = 2 sqrt(c2 (mu (mu+1)) s) - mu (c2 + s)
    GM:   delta = mu c2:  w = delta^2 / (s + delta)^2,   rho = delta s / (s + delta)
    Black-Rangarajan:  rho_mu(s) = min_w [w s + Phi_mu(w)], attained at weight_mu(s);
          TLS: Phi_mu(w) = mu (1 - w) / (mu + w) c2,     GM: Phi_mu(w) = mu c2 (sqrt(w) - 1)^2

Every function takes dtype: np.float64 (plain numpy, the operation order of gnc_math.h) or np.longdouble (the reference).

The first-order bounds of w (u = 2^-53, float64 against the exact value at the same float64 s, mu, c2):
  TLS, between the thresholds.  a = c2 (mu (mu+1)) takes 3 roundings, a / s one, the square root one (it halves the relative
    error before it: 2 u, and adds its own): q = sqrt(a / s) is off by at most 3 u q, and q <= mu + 1 there (q = mu + 1 at the
    lower threshold and falls with s).  The difference q - mu rounds once more, and is at most 1: |dw| <= 3 u (mu+1) + u <=
    4 u (mu + 1).  The thresholds themselves take 3 roundings each, so a float64 classification may differ from the exact one
    within 3 u relative of a threshold.  w is continuous there (1 and 0 are the limits of the middle formula, and the clamp
    keeps it inside) with slope |dw/ds| = q / (2 s), so a misclassified s is wrong by at most 3 u s q / (2 s) = 1.5 u q:
    1.5 u (mu+1) at the lower threshold, 1.5 u mu at the upper one.  Both are inside the same form: |dw| <= 4 u (mu+1).
  GM.  delta = mu c2 (1 rounding), q = s + delta (1), delta^2 (1), q^2 (1), the quotient (1), with the errors of delta and q
    entering twice: |dw| <= 9 u w.
  W_BOUND_C is four times the derived constant (TLS 16, GM 36), so that a computation that obeys the derivation -- the float64
  restatement here -- uses at most a quarter of it; its worst ratio over the grid of tests/test_gnc_host.py is printed there.
The bound of rho is not used by any test that holds the device: rho enters only through the sums, which are held by
m u sum |terms| around the restated sum of the device's own s.
"""
import numpy as np

import edge_restatement as er
import newton_restatement as nr
import robust_restatement as rr

U = 2.0 ** -53
TLS, GM = 0, 1
CONVERGED, ALL_INLIERS, MAX_LEVELS, INNER_FAILED, SKIPPED = 0, 1, 2, 3, 4
W_BOUND_C = {TLS: 16.0, GM: 36.0}


def weight_rho(kind, mu, c2, s, dtype=np.float64, swap_thresholds=False):
    """(w, rho) per value of s.  swap_thresholds: the built-in slip the tests must catch (mu/(mu+1) and (mu+1)/mu swapped)."""
    s = np.asarray(s, dtype)
    mu, c2 = dtype(mu), dtype(c2)
    if kind == GM:
        dl = mu * c2
        q = s + dl
        return dl * dl / (q * q), dl * (s / q)
    m1 = mu + dtype(1)
    lo, hi = mu / m1 * c2, m1 / mu * c2
    if swap_thresholds:
        lo, hi = hi, lo
    a = c2 * (mu * m1)
    safe = np.where(s > 0, s, dtype(1))
    w = np.minimum(np.maximum(np.sqrt(a / safe) - mu, dtype(0)), dtype(1))
    rho = dtype(2) * np.sqrt(a * s) - mu * (c2 + s)
    upper = s >= hi
    w = np.where(upper, dtype(0), w)
    rho = np.where(upper, c2, rho)
    lower = s <= lo                      # (taken first, as the kernel does)
    return np.where(lower, dtype(1), w), np.where(lower, s, rho)


def w_bound(kind, mu, w_ref):
    """The first-order bound of a float64 w against the exact one (module docstring)."""
    return W_BOUND_C[kind] * U * ((mu + 1.0) * np.ones_like(np.asarray(w_ref, np.float64)) if kind == TLS else np.asarray(w_ref, np.float64))


def phi(kind, mu, c2, w, dtype=np.float64):
    """The Black-Rangarajan penalty."""
    w = np.asarray(w, dtype)
    mu, c2 = dtype(mu), dtype(c2)
    if kind == TLS:
        return mu * (dtype(1) - w) / (mu + w) * c2
    r = np.sqrt(w) - dtype(1)
    return mu * c2 * r * r


def thresholds(mu, c2, dtype=np.float64):
    mu, c2 = dtype(mu), dtype(c2)
    return mu / (mu + dtype(1)) * c2, (mu + dtype(1)) / mu * c2


def sums(kind, mu, c2, s, w, R, dtype=np.float64):
    """What k_gnc_final leaves, from per-edge s and w: dict(sum_out, sum_ws, sum_rho, s_max, w_min, zero, one, between, F_w, F_mu,
    abs_w, abs_mu: the sums of the magnitudes of the terms of F_w and F_mu)."""
    s, w = np.asarray(s, dtype), np.asarray(w, dtype)
    R = np.asarray(R, bool)
    rho = weight_rho(kind, mu, c2, s[R], dtype)[1]
    so, sw, sr = np.sum(s[~R]), np.sum(w[R] * s[R]), np.sum(rho)
    return dict(sum_out=so, sum_ws=sw, sum_rho=sr, s_max=(np.max(s[R]) if R.any() else dtype(0)),
                w_min=(np.min(w[R]) if R.any() else dtype(np.inf)), zero=int(np.sum(w[R] == 0)), one=int(np.sum(w[R] == 1)),
                between=int(np.sum((w[R] > 0) & (w[R] < 1))), F_w=(so + sw) / 2, F_mu=(so + sr) / 2,
                abs_w=(np.sum(np.abs(s[~R])) + np.sum(np.abs(w[R] * s[R]))) / 2, abs_mu=(np.sum(np.abs(s[~R])) + np.sum(np.abs(rho))) / 2)


def edge_s(P, X, dtype=np.float64):
    sr, st = er.edge_s(*rr.edges_of(P), X, dtype)
    return sr + st


def run(P, X, kind, c2, R=None, mu_step=1.4, max_levels=100, anchor=0, swap_thresholds=False, **inner):
    """The loop of gnc.h in float64: inner = newton_restatement.polish_full on robust_restatement.weighted_matrix.  R: the robust
    set (default: P["inter"]).  Returns dict(outcome, X, w, levels, log, mu_initial, mu_final, s_max_initial, steps,
    factorisations, inner, num_outliers, margin); log: one row per level k >= 1 in the columns of the library's log; inner:
    the inner outcomes of the levels 0 ..; margin: the smallest relative distance of a robust s_e(X_{k-1}) from either TLS
    threshold over all levels (inf for GM)."""
    d, m = P["d"], len(P["I"])
    R = np.asarray(P["inter"] if R is None else R, bool)
    opts = dict(nr.DEFAULTS)
    opts.update(inner)
    w = np.ones(m)
    r0 = nr.polish_full(rr.weighted_matrix(P, w), X, d, anchor, **opts)
    out = dict(steps=r0["steps"], factorisations=r0["factorisations"], inner=[r0["outcome"]], levels=0, log=np.zeros((0, 10)),
               mu_initial=0.0, mu_final=0.0, margin=np.inf, F_initial=r0["F_initial"])

    def done(outcome, Xf, wf, log=()):
        s = edge_s(P, Xf)
        out.update(outcome=outcome, X=Xf, w=wf, num_outliers=int(np.sum(s[R] > c2)), log=np.array(log, np.float64).reshape(-1, 10))
        return out

    if r0["outcome"] == nr.STALLED:
        return done(INNER_FAILED, np.array(X, np.float64), w)
    Xk = r0["X"]
    s = edge_s(P, Xk)
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
        w[R] = weight_rho(kind, mu, c2, s[R], swap_thresholds=swap_thresholds)[0]
        if kind == TLS:
            lo, hi = thresholds(mu, c2)
            out["margin"] = min(out["margin"], float(np.min(np.abs(s[R] - lo) / lo)), float(np.min(np.abs(s[R] - hi) / hi)))
        before = sums(kind, mu, c2, s, w, R)
        out["levels"], out["mu_final"] = k, mu
        rk = nr.polish_full(rr.weighted_matrix(P, w), Xk, d, anchor, **opts)
        out["steps"] += rk["steps"]
        out["factorisations"] += rk["factorisations"]
        out["inner"].append(rk["outcome"])
        if rk["outcome"] == nr.STALLED:
            return done(INNER_FAILED, Xk, w_prev, log)
        Xk = rk["X"]
        s = edge_s(P, Xk)
        after = sums(kind, mu, c2, s, w, R)
        log.append((mu, before["F_mu"], before["F_w"], after["F_w"], after["F_mu"], rk["steps"], rk["outcome"], before["zero"],
                    before["one"], before["between"]))
        if (before["between"] == 0) if kind == TLS else (mu == 1.0):
            outcome = CONVERGED
            break
        mu = mu_step * mu if kind == TLS else max(mu / mu_step, 1.0)
    return done(outcome, Xk, w, log)
