"""The measurement sensitivities without a GPU (dpgo_amd/csrc/sens.h): the closed forms of tests/sens_restatement.py against
their definition -- the mixed second derivative of an edge's own term, by central differences in the edge's parameters of
lam^T g with g from newton_restatement.grad -- the whole chain dL/dtheta = -lam^T d_theta g, lam = H^-1 c, against central
differences of L(X*(theta)) with X*(theta) re-solved by newton_restatement.polish, two exact identities, the library's per-edge
arithmetic (sens_math.h through dpgo_debug_sens_edge_host) against the long-double restatement within margin_sens, and the
entry points.

Inputs: tinyGrid3D (9 poses, 11 edges, d = 3) and the compacted synthetic.ladder(d=2) (403 poses, 1358 edges), each at a
critical point: tinyGrid3D's from the chordal point by newton_restatement.polish, the ladder's the committed
tests/golden/sens_ladder2_point.npz (tests/golden/make_sens_ladder_point.py: the same polish, 69 steps).

The acceptance rule of a central difference D_h of step h against a closed form: where the function is a polynomial of degree
<= 2 in the parameter (kappa, tau, t~) the difference is exact and |closed - D_h| <= floor; otherwise (eta, and everything
through the re-solve) two steps, |closed - D_{h/2}| <= |D_h - D_{h/2}| + floor: with a truncation error c h^2 the right side is
3/4 c h^2 and the left 1/4 c h^2.  The floors are computed from the magnitudes of the terms; nothing in them comes from the
library.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_restatement as cr  # noqa: E402
import newton_restatement as nr  # noqa: E402
import robust_inputs as ri  # noqa: E402
import robust_restatement as rr  # noqa: E402
import sens_restatement as sn  # noqa: E402

import dpgo_amd  # noqa: E402
from dpgo_amd import synthetic  # noqa: E402

LD, U = sn.LD, sn.U
ULD = float(np.finfo(LD).eps) / 2
_inputs = {}


def ladder2_problem():
    g = synthetic.ladder(2)
    used = np.unique(np.concatenate([g["I"], g["J"]]))
    new = np.full(g["num_poses"], -1, np.int64)
    new[used] = np.arange(len(used))
    return rr.problem(2, len(used), new[g["I"]], new[g["J"]], g["R"], g["t"], g["kappa"], g["tau"], g["num_nodes"])


def instance(name):
    """(P, X*, M) of "tiny" or "ladder2", X* a critical point of F = 1/2 <X, M X> with pose 0 held fixed."""
    if name not in _inputs:
        if name == "tiny":
            P, X0 = ri.named("tiny")
            M = rr.weighted_matrix(P, np.ones(len(P["I"])))
            out = nr.polish_full(M, X0, 3, 0, grad_tol=1e-12)
            assert out["grad_final"] <= 1e-11, out["grad_final"]
            X = out["X"]
        else:
            P = ladder2_problem()
            M = rr.weighted_matrix(P, np.ones(len(P["I"])))
            X = np.load(os.path.join(ri.GOLDEN, "sens_ladder2_point.npz"))["X"]
            assert X.shape == (3 * P["N"], 2) and np.linalg.norm(nr.grad(M, X, 2, 0)) <= 1e-10
        _inputs[name] = (P, np.asfortranarray(X), M)
    return _inputs[name]


def seeded_edges(P, anchor, seed):
    """Three edges: the first one that touches the anchor, two seeded others."""
    I, J = P["I"], P["J"]
    first = int(np.nonzero((I == anchor) | (J == anchor))[0][0])
    rng = np.random.default_rng(seed)
    out = [first]
    while len(out) < 3:
        e = int(rng.integers(0, len(I)))
        if e not in out and anchor not in (I[e], J[e]):
            out.append(e)
    return out


def lam_g(P, X, lam, dtype=LD):
    """(lam^T g, the sum of the magnitudes of its terms times the roundings of its longest sum) on the whole graph."""
    d = P["d"]
    M = rr.weighted_matrix(P, np.ones(len(P["I"])), dtype)
    g = nr.grad(M, np.asarray(X, dtype), d)
    Ja = np.abs(cr.tangent_basis(X, d))
    MXa = np.abs(np.asarray(M, np.float64)) @ np.abs(X)
    terms = float(np.abs(np.asarray(lam, np.float64)) @ sum(Ja[c].T @ MXa[:, c] for c in range(d)))
    count = int(np.max(np.sum(np.asarray(M, np.float64) != 0, axis=1))) + 3 * d + 4 + len(lam)
    return np.asarray(lam, dtype) @ g, count * terms


# ---------------------------------------------------------------------------------------------------------------
# (a) the closed forms against the definition
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,which", [("tiny", None), ("ladder2", 0), ("ladder2", 1), ("ladder2", 2)])
def test_closed_forms_are_the_mixed_second_derivative_of_the_edges_term(name, which):
    """(the ladder's lam^T g is a long-double product with a dense 1209 x 1209 matrix: one edge per case there)"""
    P, X, _ = instance(name)
    d, dof = P["d"], cr.dof_of(P["d"])
    lam = np.random.default_rng(5).standard_normal(dof * P["N"])
    closed = -sn.sens_edge(P, X, lam, LD)            # d phi / d theta
    worst = np.zeros(2)
    edges = seeded_edges(P, 0, 11)
    for e in (edges if which is None else [edges[which]]):
        for param in range(2 + dof):
            h = 2.0 ** -10
            D = []
            for step in (h, h / 2):
                (fp, tp), (fm, tm) = lam_g(sn.perturbed(P, e, param, step), X, lam), lam_g(sn.perturbed(P, e, param, -step), X, lam)
                D.append(((fp - fm) / (2 * LD(step)), ULD * (tp + tm) / (2 * step)))
            err = abs(closed[e, param] - D[1][0])
            if param < 2 + d:       # linear in kappa and tau, quadratic in t~: the difference is exact
                allow = D[1][1]
                worst[0] = max(worst[0], float(err / allow))
                assert abs(closed[e, param] - D[0][0]) <= D[0][1], (e, param)
            else:
                allow = abs(D[0][0] - D[1][0]) + D[1][1]
                worst[1] = max(worst[1], float(err / allow))
            assert err <= allow, (name, e, param, float(closed[e, param]), float(D[1][0]), float(allow))
            assert abs(closed[e, param]) > 1e6 * D[1][1]          # (the entry is there to be checked)
    print("%s: closed form against the central difference, worst error / allowance: exact parameters %.3g, eta %.3g" % (name, worst[0], worst[1]))


def test_a_wrong_sign_or_frame_fails_the_rule():
    """The rule has teeth: eta taken on the left of R~, or omega_i's terms dropped, miss the central difference by far."""
    P, X, _ = instance("tiny")
    lam = np.random.default_rng(5).standard_normal(6 * P["N"])
    e, h = 3, 2.0 ** -10
    closed = -sn.sens_edge(P, X, lam, LD)[e]
    for param in (2, 5, 6):
        D = [(lam_g(sn.perturbed(P, e, param, s), X, lam)[0] - lam_g(sn.perturbed(P, e, param, -s), X, lam)[0]) / (2 * LD(s)) for s in (h, h / 2)]
        assert abs(-closed[param] - D[1]) > 1e3 * (abs(D[0] - D[1]) + 1e-12)
    lam0 = lam.copy()
    lam0[6 * P["I"][e] + 3:6 * P["I"][e] + 6] = 0
    assert np.abs(sn.sens_edge(P, X, lam0, LD)[e] + closed).max() > 1e-3 * np.abs(closed).max()


# ---------------------------------------------------------------------------------------------------------------
# (b) end to end: dL/dtheta = -lam^T d_theta g against the re-solved X*(theta)
# ---------------------------------------------------------------------------------------------------------------
_chain = {}


def chain(name):
    """Once per input: W, the tangent gradient c of L = <W, X> with the anchor's rows struck out, lam = H^-1 c, the restated
    sensitivities and their margin (lam to C u kappa_2 |H^-1|_2 |c|_1 entrywise), lambda_min of H."""
    if name not in _chain:
        P, X, M = instance(name)
        d, dof = P["d"], cr.dof_of(P["d"])
        W = np.random.default_rng(17).standard_normal(X.shape)
        J = cr.tangent_basis(X, d)
        c = sum(J[k].T @ W[:, k] for k in range(d))
        c[:dof] = 0.0
        A = nr.anchored_hessian(M, X, d, 0)
        ev = np.linalg.eigvalsh(A)
        assert ev[0] > 0
        lam = np.linalg.solve(A, c)
        b_lam = cr.C * U * float(ev[-1] / ev[0]) / float(ev[0]) * float(np.abs(c).sum())
        _chain[name] = dict(W=W, c=c, lam=lam, lmin=float(ev[0]), sens=sn.sens_edge(P, X, lam, LD), margin=sn.margin_sens(P, X, lam, b_lam),
                            edges=seeded_edges(P, 0, 23))
    return _chain[name]


def resolved_L(P, X, W, c, lmin, e, param, step):
    """(L(X*(theta + step)), the bound of its error): the point is within (|g| + rounding of g) / lambda_min of a critical one."""
    d = P["d"]
    Q = sn.perturbed(P, e, param, step)
    Q = dict(Q, R=np.asarray(Q["R"], np.float64), t=np.asarray(Q["t"], np.float64), kappa=np.asarray(Q["kappa"], np.float64),
             tau=np.asarray(Q["tau"], np.float64))
    M = rr.weighted_matrix(Q, np.ones(len(Q["I"])))
    out = nr.polish_full(M, X, d, 0, max_steps=5, grad_tol=1e-10)
    Ja = np.abs(cr.tangent_basis(out["X"], d))
    MXa = np.abs(M) @ np.abs(out["X"])
    g_round = 64 * U * float(np.linalg.norm(sum(Ja[k].T @ MXa[:, k] for k in range(d))))
    err = float(np.linalg.norm(c)) * (out["grad_final"] + g_round) / lmin + 4 * U * float(np.sum(np.abs(W) * np.abs(out["X"])))
    return float(np.sum(np.asarray(W, LD) * np.asarray(out["X"], LD))), err


CHAIN_CASES = [("tiny", k, None) for k in range(3)] + [("ladder2", k, p) for k in range(3) for p in range(5)]


@pytest.mark.parametrize("name,which,only", CHAIN_CASES)
def test_the_chain_against_the_resolved_solution(name, which, only):
    """(the ladder's re-solves are dense 1209 x 1209 factorisations: one parameter per case there)"""
    P, X, _ = instance(name)
    R = chain(name)
    e = R["edges"][which]
    if which == 0:
        assert 0 in (P["I"][e], P["J"][e])
    worst, strong = 0.0, np.inf
    for param in (range(2 + cr.dof_of(P["d"])) if only is None else [only]):
        h = 2.0 ** -10 * (max(1.0, float(P["kappa"][e])) if param == 0 else max(1.0, float(P["tau"][e])) if param == 1 else 1.0)
        D = []
        for step in (h, h / 2):
            (Lp, ep), (Lm, em) = (resolved_L(P, X, R["W"], R["c"], R["lmin"], e, param, s) for s in (step, -step))
            D.append(((Lp - Lm) / (2 * step), (ep + em) / (2 * step)))
        closed = float(R["sens"][e, param])
        floor = D[1][1] + float(R["margin"][e, param]) + 4 * U * abs(closed) / h
        err, allow = abs(closed - D[1][0]), abs(D[0][0] - D[1][0]) + floor
        worst = max(worst, err / allow)
        assert err <= allow, (name, e, param, closed, D, floor)
        strong = min(strong, abs(closed) / allow)
    print("%s edge %d: dL/dtheta against the re-solved central difference, worst error / allowance %.3g; the smallest entry is %.3g "
          "allowances" % (name, e, worst, strong))
    assert strong > 2.0       # (a wrong sign would show on every entry)


# ---------------------------------------------------------------------------------------------------------------
# (c) exact identities
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "rand2_70", "rand3_70", "ladder2"])
def test_phi_sums_to_the_gradient_and_scaling_every_weight_moves_nothing(name):
    """sum_e phi_e = lam^T g, and sum_e (kappa_e d phi/d kappa_e + tau_e d phi/d tau_e) = lam^T g (phi_e is linear in its weights:
    scaling every weight scales g, which does not move a minimiser) -- at points that are NOT critical, in long double."""
    P, X = ri.named(name) if name != "ladder2" else (ladder2_problem(), None)
    if X is None:
        X = cr.random_rotations_point(instance("ladder2")[1], 2, 3)
    lam = np.random.default_rng(9).standard_normal(cr.dof_of(P["d"]) * P["N"])
    want, terms = lam_g(P, X, lam)
    s, ph = sn.sens_edge(P, X, lam, LD), sn.phi(P, X, lam, LD)
    m = len(P["I"])
    tol = ULD * (terms + (m + 4 * P["d"] + 6) * float(np.sum(np.abs(np.asarray(ph, np.float64)))))
    scaled = -np.sum(np.asarray(P["kappa"], LD) * s[:, 0] + np.asarray(P["tau"], LD) * s[:, 1])
    print("%s: lam'g %.6g, sum phi off by %.3g, the weight-scaling sum by %.3g, tolerance %.3g" %
          (name, float(want), float(abs(np.sum(ph) - want)), float(abs(scaled - want)), tol))
    assert abs(want) > 1e6 * tol
    assert abs(np.sum(ph) - want) <= tol
    tol_s = ULD * (terms + (m + 4 * P["d"] + 8) * float(np.sum(np.abs(np.asarray(P["kappa"] * s[:, 0], np.float64)) + np.abs(np.asarray(P["tau"] * s[:, 1], np.float64)))))
    assert abs(scaled - want) <= tol_s


# ---------------------------------------------------------------------------------------------------------------
# (d) sens_math.h against the long-double restatement
# ---------------------------------------------------------------------------------------------------------------
HOOK_INPUTS = ["tiny", "rand3_70", "rand3_160", "ladder3", "rand2_70", "rand2_160", "ladder2", "sens_ladder2"]


def hook_input(name):
    if name == "sens_ladder2":
        P, X, _ = instance("ladder2")
        return P, X
    return ri.named(name)


@pytest.mark.parametrize("name", HOOK_INPUTS)
def test_per_edge_arithmetic_against_the_restatement(name):
    P, X = hook_input(name)
    G = ri.graph(P)
    dof = cr.dof_of(P["d"])
    worst = np.zeros(3)
    for seed in (1, 2):
        lam = np.random.default_rng(seed).standard_normal(dof * P["N"]) * (1.0 if seed == 1 else 1e-3)
        if seed == 2:
            lam[dof:2 * dof] = 0.0                                  # a pose whose adjoint is zero
        sens, ph = dpgo_amd.sens_edge_debug(G, X, lam)
        want, want_phi = sn.sens_edge(P, X, lam, LD), sn.phi(P, X, lam, LD)
        m = sn.margin_sens(P, X, lam)
        assert sens.shape == want.shape == m.shape == (len(P["I"]), 2 + dof) and np.all(np.isfinite(m)) and np.all(m > 0)
        worst[0] = max(worst[0], float(np.max(np.abs(np.asarray(sens, LD) - want) / m)))
        worst[1] = max(worst[1], float(np.max(np.abs(np.asarray(sn.sens_edge(P, X, lam), LD) - want) / m)))
        # phi: tau (a . da) + kappa <B, dB>, the two sums' margins through the weights and three roundings more
        m_phi = np.asarray(P["tau"]) * m[:, 1] + np.asarray(P["kappa"]) * m[:, 0] + 3 * U * np.abs(np.asarray(want_phi, np.float64))
        worst[2] = max(worst[2], float(np.max(np.abs(np.asarray(ph, LD) - want_phi) / m_phi)))
    print("%s: error / margin_sens: library %.3f, fp64 numpy %.3f; phi %.3f" % (name, worst[0], worst[1], worst[2]))
    assert worst.max() < 1.0, worst
    # the margin is no blanket: each output scaled by 1 + 1e-9, or its sign flipped, falls outside on most edges
    assert np.mean(np.abs(np.asarray(sens * (1 + 1e-9), LD) - want) > m) > 0.5
    # zero adjoint: exact zeros
    z, zp = dpgo_amd.sens_edge_debug(G, X, np.zeros(dof * P["N"]))
    assert not z.any() and not zp.any()


# ---------------------------------------------------------------------------------------------------------------
# (e) the entry points
# ---------------------------------------------------------------------------------------------------------------
def test_symbols_and_argument_checks():
    import ctypes as C
    L = dpgo_amd.lib()
    header = open(os.path.join(ri.ROOT, "include", "dpgo_amd.h")).read()
    for sym in ("dpgo_group_sensitivity", "dpgo_debug_sens_edge_host"):
        assert sym + "(" in header and sym in dpgo_amd.SYMBOLS and hasattr(L, sym)
    for word in ("DPGO_SENS_OK 0", "DPGO_SENS_NOT_PD 1", "DPGO_SENS_SKIPPED 2", "dpgo_sens_result_t"):
        assert word in header
    assert (dpgo_amd.SENS_OK, dpgo_amd.SENS_NOT_PD, dpgo_amd.SENS_SKIPPED) == (0, 1, 2)
    assert C.sizeof(dpgo_amd.SensResult) == 8 * 4 + 8 + 7 * 8
    P, X = ri.named("rand2_70")
    G = ri.graph(P)
    lam = np.ones(3 * P["N"])
    with pytest.raises(ValueError):
        dpgo_amd.sens_edge_debug(G, X[:-1], lam)
    with pytest.raises(ValueError):
        dpgo_amd.sens_edge_debug(G, X, lam[:-1])
    Xf = np.asfortranarray(X)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    out = np.zeros((len(P["I"]), 5))
    assert L.dpgo_debug_sens_edge_host(None, dp(Xf), Xf.shape[0], dp(lam), dp(out), None) == -1
    assert L.dpgo_debug_sens_edge_host(G._h, dp(Xf), Xf.shape[0], None, dp(out), None) == -1
    assert L.dpgo_debug_sens_edge_host(G._h, dp(Xf), Xf.shape[0], dp(lam), None, None) == -1
    assert L.dpgo_debug_sens_edge_host(G._h, dp(Xf), Xf.shape[0], dp(lam), dp(out), None) == 0 and out.any()
    r = dpgo_amd.SensResult()
    assert L.dpgo_group_sensitivity(None, G._h, dp(Xf), Xf.shape[0], 0, 0, dp(lam), len(lam), 1, None, dp(out), C.byref(r)) == -1


def test_tangent_gradient_and_unit_upstream():
    """tangent_gradient is the derivative of <G, X> along the retraction; unit_upstream the unit columns of one pose."""
    for name in ("rand2_70", "rand3_70"):
        P, X = ri.named(name)
        d, dof = P["d"], cr.dof_of(P["d"])
        rng = np.random.default_rng(3)
        G, v = rng.standard_normal(X.shape), rng.standard_normal(dof * P["N"])
        c = dpgo_amd.tangent_gradient(X, G)
        J = cr.tangent_basis(X, d)
        want = sum(J[k].T @ G[:, k] for k in range(d))
        assert c.shape == want.shape and np.abs(c - want).max() <= 16 * U * np.abs(want).max()
        h = 1e-5
        fd = (np.sum(G * cr.retract(X, h * v, d)) - np.sum(G * cr.retract(X, -h * v, d))) / (2 * h)
        assert abs(fd - c @ v) <= 1e-8 * np.linalg.norm(c) * np.linalg.norm(v)
        Uu = dpgo_amd.unit_upstream(P["N"], d, 4)
        assert Uu.shape == (dof * P["N"], dof) and Uu.sum() == dof and np.array_equal(Uu[4 * dof:5 * dof], np.eye(dof))
        with pytest.raises(ValueError):
            dpgo_amd.unit_upstream(P["N"], d, P["N"])
        with pytest.raises(ValueError):
            dpgo_amd.tangent_gradient(X, G[:-1])
