"""The sensitivities of the robust objective without a GPU (dpgo_amd/csrc/rsens.h): the closed forms of
tests/rsens_restatement.py against their definition -- central differences in an edge's parameters and in the loss threshold
delta of lam^T g with g from robust_restatement.grad -- the whole chain dL/dtheta, dL/ddelta against central differences of
L(X*(theta, delta)) with X* re-solved by robust_restatement.polish_full, the library's per-edge arithmetic (rsens_math.h through
dpgo_debug_robust_sens_edge_host) against the long-double restatement within margin_rsens, and the entry points.

Inputs, chosen on the CPU so that the conditions the tests assert hold (they are asserted again here):
  (a) robust_inputs.named("rand2_70") and ("rand3_70") at their own points with Huber, Geman-McClure and Welsch at delta = 5:
      no inter edge within 2^-8 of the Huber kink, the three edges (the intra edge with the largest residual, the inter edges
      next to the kink on either side) on their side at theta -+ h.
  (b) the same two graphs at the critical points robust_restatement.polish_full reaches from their own points with Huber at
      delta = 5 and pose 0 fixed (the start of the committed trajectories random2_huber5 / random3_huber5 on the smaller graph):
      the restated H is positive definite, no inter edge changes its side of the kink at any re-solved point, every tested
      entry is more than two allowances large.  rand3_70 with Geman-McClure and Welsch at delta = 50 covers delta and one inter
      edge for the smooth losses.

The acceptance rule of a central difference is tests/test_sens_host.py's two-step rule, for every parameter (under a robust loss
nothing is a polynomial in the parameter): h = 2^-10 and h / 2, |closed - D_{h/2}| <= |D_h - D_{h/2}| + floor.  The floors are
computed from the magnitudes of the terms; nothing in them comes from the library.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_restatement as cr  # noqa: E402
import robust_inputs as ri  # noqa: E402
import robust_restatement as rr  # noqa: E402
import rsens_restatement as rs  # noqa: E402
import sens_restatement as sn  # noqa: E402

import dpgo_amd  # noqa: E402
from dpgo_amd import LOSS_GM, LOSS_HUBER, LOSS_NONE, LOSS_WELSCH  # noqa: E402
from dpgo_amd import robust_sens_edge_debug  # noqa: E402,F401  (without the feature the file fails here)

LD, U = rs.LD, rs.U
ULD = float(np.finfo(LD).eps) / 2
H0 = 2.0 ** -10
LOSSES = [(LOSS_HUBER, 5.0), (LOSS_GM, 5.0), (LOSS_WELSCH, 5.0)]


def three_edges(P, X, loss, delta):
    """The intra edge with the largest residual, and two inter edges next to the kink: under Huber the largest s <= delta and
    the smallest s > delta; under the smooth losses the two with s nearest to delta (weight and curvature both far from 0)."""
    s = np.asarray(rr.weights(P, X, loss, delta)[0])
    it = P["inter"]
    first = int(np.argmax(np.where(~it, s, -np.inf)))
    if loss == LOSS_HUBER:
        return [first, int(np.argmax(np.where(it & (s <= delta), s, -np.inf))), int(np.argmin(np.where(it & (s > delta), s, np.inf)))]
    near = np.argsort(np.where(it, np.abs(s - delta), np.inf))
    return [first, int(near[0]), int(near[1])]


def sides(P, X, delta):
    return np.asarray(rr.weights(P, np.asarray(X, np.float64), LOSS_HUBER, float(delta))[0], np.float64)[P["inter"]] > float(delta)


def as_f64(Q):
    return dict(Q, R=np.asarray(Q["R"], np.float64), t=np.asarray(Q["t"], np.float64), kappa=np.asarray(Q["kappa"], np.float64),
                tau=np.asarray(Q["tau"], np.float64))


# ---------------------------------------------------------------------------------------------------------------
# (a) the closed forms against the definition
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rand2_70", "rand3_70"])
@pytest.mark.parametrize("loss,delta", LOSSES)
def test_closed_forms_are_the_derivatives_of_lam_g(name, loss, delta):
    P, X = ri.named(name)
    dof = cr.dof_of(P["d"])
    lam = np.random.default_rng(5).standard_normal(dof * P["N"])
    closed = -rs.rsens_edge(P, X, lam, loss, delta, LD)            # d (lam^T g) / d theta_e, and the edge's term in delta
    s0 = np.asarray(rr.weights(P, X, loss, delta)[0])
    assert np.abs(s0[P["inter"]] - delta).min() > 4 * H0            # (c): no inter edge near the kink
    edges = three_edges(P, X, loss, delta)
    assert not P["inter"][edges[0]] and P["inter"][edges[1]] and P["inter"][edges[2]]
    assert loss != LOSS_HUBER or s0[edges[1]] <= delta < s0[edges[2]]
    worst = 0.0
    for e in edges:
        for param in range(2 + dof):
            D = []
            for step in (H0, H0 / 2):
                Qp, Qm = sn.perturbed(P, e, param, step), sn.perturbed(P, e, param, -step)
                for Q in (Qp, Qm):                                  # (c): the edge keeps its side of the kink
                    assert (rr.weights(as_f64(Q), X, loss, delta)[0][e] > delta) == (s0[e] > delta)
                (fp, tp), (fm, tm) = rs.lam_g(Qp, X, lam, loss, delta), rs.lam_g(Qm, X, lam, loss, delta)
                D.append(((fp - fm) / (2 * LD(step)), ULD * (tp + tm) / (2 * step)))
            err, allow = abs(closed[e, param] - D[1][0]), abs(D[0][0] - D[1][0]) + D[1][1]
            worst = max(worst, float(err / allow))
            assert err <= allow, (name, loss, e, param, float(closed[e, param]), float(D[1][0]), float(allow))
            assert abs(closed[e, param]) > 2.0 * allow              # (the entry is there to be checked)
    # delta: the sum of the edges' last entries
    D = []
    for step in (H0, H0 / 2):
        (fp, tp), (fm, tm) = rs.lam_g(P, X, lam, loss, LD(delta) + LD(step)), rs.lam_g(P, X, lam, loss, LD(delta) - LD(step))
        D.append(((fp - fm) / (2 * LD(step)), ULD * (tp + tm) / (2 * step)))
    total = np.sum(closed[:, -1])
    err, allow = abs(total - D[1][0]), abs(D[0][0] - D[1][0]) + D[1][1]
    print("%s loss %d: closed form against the central difference, worst error / allowance: theta %.3g, delta %.3g"
          % (name, loss, worst, float(err / allow)))
    assert err <= allow and abs(total) > 2.0 * allow
    assert not closed[~P["inter"], -1].any()


def test_the_three_mutants_fail_the_rule():
    """The rule has teeth: the c-term dropped, w dropped, the factor 1/2 of c / 2 lost -- each misses the central difference
    by far on an inter edge above the Huber kink."""
    P, X = ri.named("rand3_70")
    loss, delta = LOSS_HUBER, 5.0
    lam = np.random.default_rng(5).standard_normal(6 * P["N"])
    e = three_edges(P, X, loss, delta)[2]
    for param in (0, 1, 3, 6):
        D = [(rs.lam_g(sn.perturbed(P, e, param, s), X, lam, loss, delta)[0] - rs.lam_g(sn.perturbed(P, e, param, -s), X, lam, loss, delta)[0])
             / (2 * LD(s)) for s in (H0, H0 / 2)]
        good = -rs.rsens_edge(P, X, lam, loss, delta, LD)[e, param]
        assert abs(good - D[1]) <= abs(D[0] - D[1]) + 1e-12
        for kw in (dict(drop_c=True), dict(drop_w=True), dict(c_factor=1.0)):
            bad = -rs.rsens_edge(P, X, lam, loss, delta, LD, **kw)[e, param]
            assert abs(bad - D[1]) > 1e3 * (abs(D[0] - D[1]) + 1e-12), (param, kw)


# ---------------------------------------------------------------------------------------------------------------
# (b) end to end: dL/dtheta and dL/ddelta against the re-solved X*(theta, delta)
# ---------------------------------------------------------------------------------------------------------------
_chain = {}


def chain(name, loss, delta):
    """Once per case: the critical point, W, the tangent gradient c of L = <W, X> with the anchor's rows struck out, lam = H^-1 c,
    the restated sensitivities and their margin (lam to C u kappa_2 |H^-1|_2 |c|_1 entrywise), lambda_min of H."""
    key = (name, loss, delta)
    if key not in _chain:
        P, X0 = ri.named(name)
        d, dof = P["d"], cr.dof_of(P["d"])
        out = rr.polish_full(P, X0, loss, delta, 1, 0, max_steps=40, grad_tol=1e-10)
        assert out["outcome"] == rr.CONVERGED and out["grad_final"] <= 1e-10
        X = np.asfortranarray(out["X"])
        W = np.random.default_rng(17).standard_normal(X.shape)
        J = cr.tangent_basis(X, d)
        c = sum(J[k].T @ W[:, k] for k in range(d))
        c[:dof] = 0.0
        A = rr.hessian(P, X, loss, delta, 1, 0)
        ev = np.linalg.eigvalsh(A)
        assert ev[0] > 0                                                    # (c): H is positive definite at the point
        lam = np.linalg.solve(A, c)
        b_lam = cr.C * U * float(ev[-1] / ev[0]) / float(ev[0]) * float(np.abs(c).sum())
        _chain[key] = dict(P=P, X=X, W=W, c=c, lam=lam, lmin=float(ev[0]), sens=rs.rsens_edge(P, X, lam, loss, delta, LD),
                           margin=rs.margin_rsens(P, X, lam, loss, delta, b_lam), edges=three_edges(P, X, loss, delta),
                           sides=sides(P, X, delta))
    return _chain[key]


def resolved_L(R, loss, Q, delta):
    """(L(X*) of the problem Q at delta, the bound of its error): the point is within (|g| + rounding of g) / lambda_min of a
    critical one.  Asserts that no inter edge has changed its side of the Huber kink."""
    P, X, W = R["P"], R["X"], R["W"]
    Q = as_f64(Q)
    out = rr.polish_full(Q, X, loss, delta, 1, 0, max_steps=8, grad_tol=1e-10)
    assert out["outcome"] == rr.CONVERGED
    if loss == LOSS_HUBER:
        assert np.array_equal(sides(Q, out["X"], delta), R["sides"])
    w = np.asarray(rr.weights(Q, out["X"], loss, delta)[2])
    g_round = 64 * U * float(np.linalg.norm(rr.scatter(Q, rs.ghat_abs(Q, out["X"]), w)))
    err = float(np.linalg.norm(R["c"])) * (out["grad_final"] + g_round) / R["lmin"] + 4 * U * float(np.sum(np.abs(W) * np.abs(out["X"])))
    return float(np.sum(np.asarray(W, LD) * np.asarray(out["X"], LD))), err


def judge(closed, margin, D, h):
    floor = D[1][1] + margin + 4 * U * abs(closed) / h
    err, allow = abs(closed - D[1][0]), abs(D[0][0] - D[1][0]) + floor
    return err, allow


@pytest.mark.parametrize("name", ["rand2_70", "rand3_70"])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_the_chain_against_the_resolved_solution_in_theta(name, which):
    loss, delta = LOSS_HUBER, 5.0
    R = chain(name, loss, delta)
    P = R["P"]
    e = R["edges"][which]
    worst, strong = 0.0, np.inf
    for param in range(2 + cr.dof_of(P["d"])):
        h = H0 * (max(1.0, float(P["kappa"][e])) if param == 0 else max(1.0, float(P["tau"][e])) if param == 1 else 1.0)
        D = []
        for step in (h, h / 2):
            (Lp, ep), (Lm, em) = (resolved_L(R, loss, sn.perturbed(P, e, param, s), delta) for s in (step, -step))
            D.append(((Lp - Lm) / (2 * step), (ep + em) / (2 * step)))
        closed = float(R["sens"][e, param])
        err, allow = judge(closed, float(R["margin"][e, param]), D, h)
        worst = max(worst, err / allow)
        assert err <= allow, (name, e, param, closed, D)
        strong = min(strong, abs(closed) / allow)
    print("%s edge %d (%s): dL/dtheta against the re-solved central difference, worst error / allowance %.3g; the smallest entry is "
          "%.3g allowances" % (name, e, ("intra", "inter below the kink", "inter above the kink")[which], worst, strong))
    assert strong > 2.0       # (c): a wrong sign or factor would show on every entry


@pytest.mark.parametrize("name,loss,delta", [("rand2_70", LOSS_HUBER, 5.0), ("rand3_70", LOSS_HUBER, 5.0), ("rand3_70", LOSS_GM, 50.0),
                                             ("rand3_70", LOSS_WELSCH, 50.0)])
def test_the_chain_against_the_resolved_solution_in_delta(name, loss, delta):
    R = chain(name, loss, delta)
    P = R["P"]
    h = H0 * delta
    D = []
    for step in (h, h / 2):
        (Lp, ep), (Lm, em) = (resolved_L(R, loss, P, delta + s) for s in (step, -step))
        D.append(((Lp - Lm) / (2 * step), (ep + em) / (2 * step)))
    closed = float(np.sum(R["sens"][:, -1]))
    err, allow = judge(closed, float(np.sum(R["margin"][:, -1])), D, h)
    print("%s loss %d: dL/ddelta %.6g against the re-solved central difference %.6g, error / allowance %.3g; the entry is %.3g allowances"
          % (name, loss, closed, D[1][0], err / allow, abs(closed) / allow))
    assert err <= allow and abs(closed) > 2.0 * allow
    if loss != LOSS_HUBER:        # one inter edge's kappa and tau under the smooth losses
        e = R["edges"][1]
        for param in (0, 1):
            hh = H0 * max(1.0, float(P["kappa" if param == 0 else "tau"][e]))
            D = []
            for step in (hh, hh / 2):
                (Lp, ep), (Lm, em) = (resolved_L(R, loss, sn.perturbed(P, e, param, s), delta) for s in (step, -step))
                D.append(((Lp - Lm) / (2 * step), (ep + em) / (2 * step)))
            closed = float(R["sens"][e, param])
            err, allow = judge(closed, float(R["margin"][e, param]), D, hh)
            assert err <= allow and abs(closed) > 2.0 * allow, (e, param, closed, D)


# ---------------------------------------------------------------------------------------------------------------
# (d) rsens_math.h against the long-double restatement
# ---------------------------------------------------------------------------------------------------------------
HOOK_INPUTS = ["tiny", "rand3_70", "rand3_160", "ladder3", "rand2_70", "rand2_160", "ladder2", "rand3_40"]


def hook_delta(name):
    return 0.25 if name.startswith("ladder") else 5.0


@pytest.mark.parametrize("name", HOOK_INPUTS)
@pytest.mark.parametrize("loss", [LOSS_HUBER, LOSS_GM, LOSS_WELSCH])
def test_per_edge_arithmetic_against_the_restatement(name, loss):
    P, X = ri.named(name)
    G = ri.graph(P)
    delta = hook_delta(name)
    dof = cr.dof_of(P["d"])
    m_edges = len(P["I"])
    w_lib, c_lib = dpgo_amd.robust_edge_debug(G, X, loss, delta)[:2]
    worst = np.zeros(3)
    for seed in (1, 2):
        lam = np.random.default_rng(seed).standard_normal(dof * P["N"]) * (1.0 if seed == 1 else 1e-3)
        if seed == 2:
            lam[dof:2 * dof] = 0.0                                  # a pose whose adjoint is zero
        sens, ph = dpgo_amd.robust_sens_edge_debug(G, X, lam, loss, delta)
        want = rs.rsens_edge(P, X, lam, loss, delta, LD)
        m = rs.margin_rsens(P, X, lam, loss, delta)
        assert sens.shape == want.shape == m.shape == (m_edges, 3 + dof) and not np.isnan(m).any() and np.all(m >= 0)
        finite = np.isfinite(m).all(axis=1)                         # (an edge inside the bound of s around Huber's kink: none)
        assert finite.all()
        worst[0] = max(worst[0], float(np.max(np.abs(np.asarray(sens, LD) - want) / (m + 1e-300))))
        worst[1] = max(worst[1], float(np.max(np.abs(np.asarray(rs.rsens_edge(P, X, lam, loss, delta), LD) - want) / (m + 1e-300))))
        worst[2] = max(worst[2], float(np.max(np.abs(np.asarray(ph, LD) - sn.phi(P, X, lam, LD)) /
                                              (np.asarray(P["tau"]) * sn.margin_sens(P, X, lam)[:, 1] + np.asarray(P["kappa"]) * sn.margin_sens(P, X, lam)[:, 0]
                                               + 3 * U * np.abs(np.asarray(ph, np.float64)) + 1e-300))))
        # exact zeros where the weight is exactly 0; intra edges carry sens_math.h's values and no delta term
        assert not sens[w_lib == 0].any()
        plain = dpgo_amd.sens_edge_debug(G, X, lam)[0]
        assert np.array_equal(sens[~P["inter"], :-1], plain[~P["inter"]]) and not sens[~P["inter"], -1].any()
        if seed == 1:
            live = w_lib != 0
            # the margin is no blanket: each output scaled by 1 + 1e-9 falls outside on most entries of the live edges
            assert np.mean((np.abs(np.asarray(sens * (1 + 1e-9), LD) - want) > m)[live][:, :-1]) > 0.5
            # the three mutants, each caught: on the edges with curvature the library's output is outside the mutant's margin
            curved = c_lib != 0
            assert curved.sum() >= 3
            for kw in (dict(drop_c=True), dict(drop_w=True), dict(c_factor=1.0)):
                bad = rs.rsens_edge(P, X, lam, loss, delta, LD, **kw)
                assert np.mean((np.abs(np.asarray(sens, LD) - bad) > m)[curved][:, :-1]) > 0.5, kw
    print("%s loss %d: error / margin_rsens: library %.3f, fp64 numpy %.3f; phi %.3f" % (name, loss, worst[0], worst[1], worst[2]))
    assert worst.max() < 1.0, worst
    z, zp = dpgo_amd.robust_sens_edge_debug(G, X, np.zeros(dof * P["N"]), loss, delta)
    assert not z.any() and not zp.any()


# ---------------------------------------------------------------------------------------------------------------
# (e) the trivial loss, and the entry points
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "rand2_70", "rand3_70", "ladder3"])
def test_the_trivial_loss_gives_the_values_of_the_plain_sensitivities(name):
    P, X = ri.named(name)
    G = ri.graph(P)
    lam = np.random.default_rng(3).standard_normal(cr.dof_of(P["d"]) * P["N"])
    sens, ph = dpgo_amd.robust_sens_edge_debug(G, X, lam, LOSS_NONE)
    plain, plain_phi = dpgo_amd.sens_edge_debug(G, X, lam)
    assert np.all(sens[:, :-1] == plain) and np.array_equal(ph, plain_phi) and not sens[:, -1].any()


def test_symbols_and_argument_checks():
    import ctypes as C
    L = dpgo_amd.lib()
    header = open(os.path.join(ri.ROOT, "include", "dpgo_amd.h")).read()
    for sym in ("dpgo_group_robust_sensitivity", "dpgo_debug_robust_sens_edge_host"):
        assert sym + "(" in header and sym in dpgo_amd.SYMBOLS and hasattr(L, sym)
    P, X = ri.named("rand2_70")
    G = ri.graph(P)
    lam = np.ones(3 * P["N"])
    with pytest.raises(ValueError):
        dpgo_amd.robust_sens_edge_debug(G, X[:-1], lam, LOSS_HUBER, 5.0)
    with pytest.raises(ValueError):
        dpgo_amd.robust_sens_edge_debug(G, X, lam[:-1], LOSS_HUBER, 5.0)
    with pytest.raises(ValueError):
        dpgo_amd.robust_sens_edge_debug(G, X, lam, 4, 5.0)
    with pytest.raises(ValueError):
        dpgo_amd.robust_sens_edge_debug(G, X, lam, LOSS_HUBER, 0.0)
    Xf = np.asfortranarray(X)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    out, dreg = np.zeros((len(P["I"]), 6)), np.zeros(1)
    assert L.dpgo_debug_robust_sens_edge_host(None, dp(Xf), Xf.shape[0], 1, 5.0, dp(lam), dp(out), None) == -1
    assert L.dpgo_debug_robust_sens_edge_host(G._h, dp(Xf), Xf.shape[0], 1, 5.0, None, dp(out), None) == -1
    assert L.dpgo_debug_robust_sens_edge_host(G._h, dp(Xf), Xf.shape[0], 1, 5.0, dp(lam), None, None) == -1
    assert L.dpgo_debug_robust_sens_edge_host(G._h, dp(Xf), Xf.shape[0], 1, 5.0, dp(lam), dp(out), None) == 0 and out.any()
    r = dpgo_amd.SensResult()
    assert L.dpgo_group_robust_sensitivity(None, G._h, dp(Xf), Xf.shape[0], 1, 5.0, 0, 0, dp(lam), len(lam), 1, None, dp(out), dp(dreg),
                                           C.byref(r)) == -1
