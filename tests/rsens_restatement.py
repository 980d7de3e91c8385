"""Restatement of the sensitivities of the ROBUST objective (dpgo_amd/csrc/rsens.h, rsens_math.h): test infrastructure on
tests/sens_restatement.py (the layout, phi_e and its derivatives) and tests/robust_restatement.py (weights, curvature, grad,
hessian, polish_full).  Plain numpy; nothing of the library is imported here.  Every function takes a dtype: np.float64 is
"what ordinary fp64 reaches", np.longdouble the reference.

    F = 1/2 sum_intra s_e + 1/2 sum_inter rho(s_e; delta),    w_e = rho'(s_e),    c_e = 2 rho''(s_e),    g = sum_e w_e ghat_e
    lambda^T g = sum_e w_e phi_e,                               phi_e = lambda_i^T ghat_e(i) + lambda_j^T ghat_e(j)
    dL/dtheta_e = -[ w_e d phi_e/d theta_e + (c_e / 2) phi_e d s_e/d theta_e ],          theta_e = (kappa, tau, t~, eta)
    dL/ddelta   = -sum_inter (d w_e/d delta) phi_e
    d s/d kappa = |B|_F^2     d s/d tau = |a|^2     d s/d t~ = -2 tau R_i^T a     d s/d eta_k = -2 kappa <hat(e_k), R~^T R_i^T B>
    d w/d delta: Huber w / (2 delta) for s > delta, 0 for s <= delta; Geman-McClure 2 delta s / (s + delta)^3; Welsch w s / delta^2

tests/test_rsens_host.py holds these closed forms against central differences of lam^T g (robust_restatement.grad) in theta and
in delta, and the whole chain against re-solved critical points: that, not this paragraph, is the judge of signs and factors.

The margin (u = 2^-53), fixed here before any device is asked, to first order in u.  The device computes, per (edge, adjoint),
    out_a = fma(-(c / 2) phi, ds_a, w o_a)   (a < 2 + dof),        out_delta = -(dw phi),
with o = sens_one's output (bound margin_sens, which carries the entrywise bound b of lambda), phi = tau (a . da) + kappa <B, dB>
(bound tau margin_sens[tau] + kappa margin_sens[kappa] + 3 u |phi|, tests/test_sens_host.py (d)), w and c within
robust_restatement.w_bound and c_bound, and
  * ds: sums of products like sens_one's, the longest path (the eta entries) B^T (d + 1 roundings), the product with Y_i (d),
    the two sums of d products over R~ (2 d), the weight (1; the factor 2 is exact); |B|_F^2 is B^T and a sum of d^2 squares.
    (d^2 + 3 d + 4) u T_ds covers every entry, T_ds the same expression on the magnitudes of the operands.
  * dw: Huber w / (2 delta): w_bound / (2 delta) and 2 roundings; Geman-McClure 2 delta s / (s + delta)^3: the derivative in s
    (2 delta / q^3 + 6 delta s / q^4 in magnitude, q = s + delta) times the bound of s, and 6 roundings; Welsch w s / delta^2:
    (w_bound s + w bound(s)) / delta^2 and 4 roundings; each with robust_restatement's TINY terms for results below 2^-1022;
    infinite inside the bound of s around Huber's kink, as c_bound.
  * the new products: w o, (c / 2) phi and the fma are 3 roundings (c / 2 is exact), one more for what first order leaves out:
    4 u (|w o| + |c phi ds| / 2); dw phi is one product: 2 u |dw phi|.
margin_rsens = |w| margin_sens + w_bound |o| + c_bound |phi ds| / 2 + |c| (bound(phi) |ds| + |phi| bound(ds)) / 2
               + 4 u (|w o| + |c phi ds| / 2)                                                        (a < 2 + dof)
             = bound(dw) |phi| + |dw| bound(phi) + 2 u |dw phi|                                      (the delta entry)
"""
import numpy as np

import cov_restatement as cr
import edge_restatement as er
import robust_restatement as rr
import sens_restatement as sn
from oracle.problem import LOSS_GM, LOSS_HUBER, LOSS_NONE, LOSS_WELSCH

LD = sn.LD
U = sn.U
TINY = rr.TINY

dof_of = sn.dof_of
perturbed = sn.perturbed


def ds_dtheta(P, X, dtype=np.float64, absolute=False):
    """(m, 2 + dof): d s_e / d (kappa, tau, t~, eta).  absolute: the sums of the magnitudes of the terms."""
    d, N = P["d"], P["N"]
    X = np.asarray(X, dtype)
    I, J = np.asarray(P["I"]), np.asarray(P["J"])
    Rt, tt = np.asarray(P["R"], dtype), np.asarray(P["t"], dtype)
    kappa, tau = np.asarray(P["kappa"], dtype), np.asarray(P["tau"], dtype)
    if absolute:
        X, Rt, tt = np.abs(X), np.abs(Rt), np.abs(tt)
    sub = (lambda a, b: a + b) if absolute else (lambda a, b: a - b)
    Y = X[N:].reshape(N, d, d)
    Ri, Rj, ti, tj = sn._T(Y[I]), sn._T(Y[J]), X[I], X[J]
    a = sub(sub(tj, ti), sn._mv(Ri, tt))
    B = sub(Rj, sn._mm(Ri, Rt))
    s_tau = np.sum(a * a, axis=-1)
    s_kappa = np.sum(np.sum(B * B, axis=-1), axis=-1)
    sg = 1 if absolute else -1
    s_t = sg * 2 * tau[:, None] * sn._mv(sn._T(Ri), a)
    Z = sn._mm(sn._T(Rt), sn._mm(sn._T(Ri), B))
    if d == 2:
        h = np.stack([sub(Z[..., 1, 0], Z[..., 0, 1])], axis=-1)
    else:
        h = np.stack([sub(Z[..., 2, 1], Z[..., 1, 2]), sub(Z[..., 0, 2], Z[..., 2, 0]), sub(Z[..., 1, 0], Z[..., 0, 1])], axis=-1)
    s_eta = sg * 2 * kappa[:, None] * h
    return np.concatenate([s_kappa[:, None], s_tau[:, None], s_t, s_eta], axis=-1)


def dw_ddelta(s, w, loss, delta, inter, dtype=np.float64):
    """d w_e / d delta as a function of s and w = rho'(s); 0 on intra edges, and exactly 0 where w is exactly 0."""
    s, w, dl = np.asarray(s, dtype), np.asarray(w, dtype), dtype(delta)
    if loss == LOSS_NONE:
        return np.zeros_like(s)
    if loss == LOSS_HUBER:
        out = np.where(s > dl, w / (2 * dl), 0)
    elif loss == LOSS_GM:
        out = 2 * dl * s / ((s + dl) * (s + dl) * (s + dl))
    elif loss == LOSS_WELSCH:
        out = w * s / (dl * dl)
    else:
        raise ValueError("loss")
    return np.where(np.asarray(inter) & (w != 0), out, 0)


def parts(P, X, lam, loss, delta, dtype=np.float64):
    """dict(o (m, k, 2 + dof), phi (m, k), ds (m, 2 + dof), s, w, c, dw (m,)) in dtype."""
    o, ph = sn._evaluate(P, X, lam, dtype, False)
    s, _, w, c = rr.weights(P, np.asarray(X, dtype), loss, delta, dtype)
    return dict(o=o, phi=ph, ds=ds_dtheta(P, X, dtype), s=s, w=w, c=c, dw=dw_ddelta(s, w, loss, delta, P["inter"], dtype))


def rsens_edge(P, X, lam, loss, delta, dtype=np.float64, drop_c=False, drop_w=False, c_factor=0.5):
    """dL/d(kappa, tau, t~, eta) and the edge's term of dL/ddelta of every edge for the adjoint(s) lam: (m, 3 + dof), or
    (m, k, 3 + dof) for lam (dof N, k).  drop_c, drop_w, c_factor: the mutants of tests/test_rsens_host.py."""
    p = parts(P, X, lam, loss, delta, dtype)
    w = np.ones_like(p["w"]) if drop_w else p["w"]
    c = np.zeros_like(p["c"]) if drop_c else p["c"]
    main = w[:, None, None] * p["o"] - (dtype(c_factor) * c)[:, None, None] * p["phi"][..., None] * p["ds"][:, None, :]
    last = -(p["dw"][:, None] * p["phi"])
    return sn._shape(np.concatenate([main, last[..., None]], axis=-1), lam)


def dloss_reg(P, X, lam, loss, delta, dtype=np.float64):
    """dL/ddelta: a number, or (k,) for lam (dof N, k)."""
    return np.sum(rsens_edge(P, X, lam, loss, delta, dtype)[..., -1], axis=0)


def dw_bound(P, X, loss, delta):
    """The bound of d w_e / d delta given the bounds of s_e and w_e (the module's text)."""
    s, _, w, _ = (np.asarray(a, np.float64) for a in rr.weights(P, X, loss, delta, LD))
    if loss == LOSS_NONE:
        return np.zeros_like(s)
    sb = er.s_bound(*rr.edges_of(P), X)[2]
    bw = rr.w_bound(P, X, loss, delta)
    dw = np.abs(np.asarray(dw_ddelta(s, w, loss, delta, P["inter"]), np.float64))
    if loss == LOSS_HUBER:
        b = bw / (2 * delta) + 2 * U * dw + TINY
        b[np.abs(s - delta) <= sb] = np.inf
    elif loss == LOSS_GM:
        q = s + delta
        b = (2 * delta / q ** 3 + 6 * delta * s / q ** 4) * sb + 6 * U * dw + TINY
    else:
        b = (bw * s + w * sb) / delta ** 2 + 4 * U * dw + (2 * s / delta ** 2 + 1) * TINY
    return np.where(P["inter"], b, 0.0)


def ds_rounding_count(d):
    return d * d + 3 * d + 4


def margin_rsens(P, X, lam, loss, delta, b_lam=0.0):
    """The entrywise bound of the module docstring on the fp64 evaluation of rsens_edge, lam known to within b_lam entrywise
    (a number, or one per column of lam): (m, 3 + dof) or (m, k, 3 + dof)."""
    d = P["d"]
    p = parts(P, X, lam, loss, delta, LD)
    o, ph, ds = (np.abs(np.asarray(p[k], np.float64)) for k in ("o", "phi", "ds"))
    w, c, dw = (np.abs(np.asarray(p[k], np.float64)) for k in ("w", "c", "dw"))
    lam2 = np.asarray(lam, np.float64).reshape(len(np.asarray(lam)), -1)
    bo = sn.margin_sens(P, X, lam2, b_lam)                                       # (m, k, 2 + dof)
    bphi = np.asarray(P["tau"])[:, None] * bo[..., 1] + np.asarray(P["kappa"])[:, None] * bo[..., 0] + 3 * U * ph
    bds = ds_rounding_count(d) * U * np.asarray(ds_dtheta(P, X, np.float64, absolute=True))
    bw, bc, bdw = rr.w_bound(P, X, loss, delta), rr.c_bound(P, X, loss, delta), dw_bound(P, X, loss, delta)
    e3 = lambda v: v[:, None, None]
    pd = ph[..., None] * ds[:, None, :]                                          # |phi ds|
    main = (e3(w) * bo + e3(bw) * o + 0.5 * e3(bc) * pd + 0.5 * e3(c) * (bphi[..., None] * ds[:, None, :] + ph[..., None] * bds[:, None, :])
            + 4 * U * (e3(w) * o + 0.5 * e3(c) * pd))
    last = bdw[:, None] * ph + dw[:, None] * bphi + 2 * U * dw[:, None] * ph
    return sn._shape(np.concatenate([main, last[..., None]], axis=-1), lam)


def ghat_abs(P, X):
    """(m, 2, dof), float64: robust_restatement.edge_ghat with every operand replaced by its magnitude and every difference
    by a sum -- the magnitudes of the terms an entry of g_e is made of."""
    d, N = P["d"], P["N"]
    Me = np.asarray(rr.edge_matrices(dict(P, R=np.asarray(P["R"], np.float64), t=np.asarray(P["t"], np.float64),
                                          kappa=np.asarray(P["kappa"], np.float64), tau=np.asarray(P["tau"], np.float64)), absolute=True))
    Xa = np.abs(np.asarray(X, np.float64))
    Xe = Xa[rr.edge_index(P)]
    rows = np.einsum("eab,ebc->eac", Me, Xe).reshape(len(P["I"]), 2, d + 1, d)
    Y = Xa[N:].reshape(N, d, d)
    out = np.zeros((len(P["I"]), 2, dof_of(d)))
    for role, pose in enumerate((P["I"], P["J"])):
        out[:, role, :d] = rows[:, role, 0, :]
        for k, Gk in enumerate(rr.generators(d)):
            out[:, role, d + k] = np.sum(np.einsum("rq,eqc->erc", np.abs(Gk), Y[pose]) * rows[:, role, 1:, :], axis=(1, 2))
    return out


def lam_g(P, X, lam, loss, delta, dtype=LD):
    """(lam^T g(X; theta, delta), the magnitude its rounding error is measured against) with g from robust_restatement.grad,
    not anchored.  The magnitude, to be multiplied by the unit roundoff of dtype: per edge w_e |lam|^T |g_e| on magnitudes
    (ghat_abs) times the roundings of the longest path -- the rows (2 d + 6, rows_bound), g_e (2 d + 1, ghat_bound), the
    weight's formula (8, w_bound), the sums over a pose's edges and over lam (the largest degree + dof N) -- plus what the
    rounding of s_e ((d + 3) s_bar_e, edge_restatement.s_bound) does through |dw/ds| <= 2 w / delta."""
    d, N = P["d"], P["N"]
    dof = dof_of(d)
    g = rr.grad(P, np.asarray(X, dtype), loss, delta, None, dtype)
    A = ghat_abs(P, X)
    la = np.abs(np.asarray(lam, np.float64)).reshape(N, dof)
    per_edge = np.sum(la[P["I"]] * A[:, 0], axis=1) + np.sum(la[P["J"]] * A[:, 1], axis=1)
    w = np.abs(np.asarray(rr.weights(P, np.asarray(X, np.float64), loss, float(delta))[2], np.float64))
    Pf = [np.asarray(a, np.float64) for a in rr.edges_of(P)]
    sbar = sum(er.edge_s(P["I"], P["J"], *Pf[2:], X, np.float64, absolute=True))
    deg = int(np.max(np.bincount(np.concatenate([P["I"], P["J"]]), minlength=N)))
    count = (2 * d + 6) + (2 * d + 1) + 8 + deg + dof * N
    through_s = 0.0 if loss == LOSS_NONE else 2 * (d + 3) * sbar / float(delta)
    return np.asarray(lam, dtype) @ g, float(np.sum((count + np.where(P["inter"], through_s, 0.0)) * w * per_edge))
