"""The kernels of the maximum-likelihood objective on the device (dpgo_amd/csrc/ml.hip) against the long-double restatement
(tests/ml_restatement.py), each output within its derived rounding bound times the constant fixed on the CPU
(tests/test_ml_host.py: CONSTANTS): k_ml_edge through NodeGroup.ml_eval(full=True) on chains of 1, 63, 64, 65 and 297 edges,
k_ml_gather and k_ml_hessian through NodeGroup.ml_hessian on the fixtures and the ladders from three anchors, and the isotropic
consistency with k_cov_hessian on a noise-free graph.  Nothing in a bound comes from the device.
"""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_restatement as cr  # noqa: E402
import ml_inputs as mi  # noqa: E402
import ml_restatement as mr  # noqa: E402
import test_ml_host as tmh  # noqa: E402  (its constants, graphs and points; none of its tests is imported)

import dpgo_amd  # noqa: E402
from oracle.problem import LOSS_NONE  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = cr.LD
C = tmh.CONSTANTS


def group_of(E, nn, info=True):
    """A trivial-loss group that hosts every node of E's graph on nn nodes, built on the graph that keeps E's Omega."""
    G = tmh.graph_of(E, nn, info)
    return dpgo_amd.NodeGroup(G, range(nn), dpgo_amd.Options.driver(LOSS_NONE, True, max_iterations=0))


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 297])
def test_edge_pass_against_the_long_double_restatement(d, m):
    E, X, near = mi.chain(d, m)
    ref = mr.edges_all(E, X, LD)
    bnd = mr.edge_bounds(E, X, ref)
    held = tmh.held_edges(E, ref)
    assert int((~held).sum()) == near == ref["near_pi"]
    grp = group_of(E, 1)
    F, r, chi2, near_dev, more = grp.ml_eval(X, full=True)
    got = dict(more, r=r, chi2=chi2)
    # theta^2 on both sides of the series' threshold, and exactly zero
    th2 = (np.asarray(ref["r"], np.float64)[:, d:] ** 2).sum(axis=1)
    if d == 3 and m >= 3:
        assert np.any((th2 > 0) & (th2 < mr.SERIES_T2)) and np.any((th2 > mr.SERIES_T2) & (th2 < 1e-6)) and th2[m - 1] == 0.0
    if m >= 3:
        assert not r[m - 1].any() and chi2[m - 1] == 0.0 and not more["grad"][m - 1].any()
    for k in ("r", "wr", "chi2", "Ji", "Jj", "grad"):
        err = np.abs(np.asarray(got[k], LD) - ref[k]).astype(np.float64)[held]
        b = C[k] * bnd[k][held]
        worst = float((err[b > 0] / b[b > 0]).max()) if np.any(b > 0) else 0.0
        print("d = %d, m = %d: %s at %.3g of its bound" % (d, m, k, worst))
        assert np.all(err <= b), (k, worst)
    # W = Omega J: J's own bound through |Omega|, and a dot product of length dof
    dof = cr.dof_of(d)
    Om = np.abs(E["Om"])
    for k, j in (("Wi", "Ji"), ("Wj", "Jj")):
        want = np.asarray(E["Om"], LD) @ ref[j]
        b = Om @ (C[j] * bnd[j]) + dof * U * (Om @ np.abs(np.asarray(ref[j], np.float64)))
        assert np.all(np.abs(np.asarray(got[k], LD) - want).astype(np.float64)[held] <= b[held]), k
    assert near_dev == near
    # F_ml: 1/2 of the device's own chi2 in a fixed tree (an edge near pi has a value, whatever it is); the same bits again
    assert abs(F - 0.5 * chi2.sum()) <= U * (np.ceil(np.log2(max(m, 2))) + 6) * 0.5 * np.abs(chi2).sum()
    if near == 0:
        bF = mr.sum_bounds(E, E["N"], ref, bnd)[0]
        assert abs(float(LD(F) - ref["chi2"].sum() / 2)) <= C["F"] * bF
    again = grp.ml_eval(X, full=True)
    assert again[0] == F and np.array_equal(again[1], r) and np.array_equal(again[2], chi2)
    for k in more:
        assert np.array_equal(again[4][k], more[k])


CASES = [("tinyGrid3D", 1), ("tinyGrid3D", 2), ("smallGrid3D", 1), ("smallGrid3D", 2), ("smallGrid3D", 5), ("ladder2", 6), ("ladder3", 6)]
_in = {}


def case_input(fixtures_dir, name):
    if name not in _in:
        E = mi.ladder(int(name[-1])) if name.startswith("ladder") else mi.fixture(fixtures_dir, name)
        X = tmh.chordal_point(E)
        ref = mr.edges_all(E, X, LD)
        bnd = mr.edge_bounds(E, X, ref)
        # poses an edge near pi touches are not held (ml.h: its values are not specified)
        loose = np.zeros(E["N"], bool)
        for e in np.flatnonzero(~tmh.held_edges(E, ref)):
            loose[[E["I"][e], E["J"][e]]] = True
        _in[name] = (E, X, ref, bnd, loose)
    return _in[name]


@pytest.mark.parametrize("name,nn", CASES)
def test_gradient_and_hessian_against_the_long_double_restatement(fixtures_dir, name, nn):
    E, X, ref, bnd, loose = case_input(fixtures_dir, name)
    d, N = E["d"], E["N"]
    dof = cr.dof_of(d)
    n = dof * N
    grp = group_of(E, nn)
    bF, bg, bH = mr.sum_bounds(E, N, ref, bnd)
    lo = np.repeat(loose, dof)
    for a in (0, N // 2, N - 1):
        Fr, gr, Hr = mr.assemble(E, X, a, LD, per_edge=ref)
        ptr, col, val, g, F = grp.ml_hessian(X, anchor=a)
        assert ptr.shape == (n + 1,) and ptr[-1] == len(col) == len(val)
        stored = sp.csr_matrix((np.ones(len(col)), col, ptr), shape=(n, n)).toarray() > 0
        D = sp.csr_matrix((val, col, ptr), shape=(n, n)).toarray()
        assert np.all(np.asarray(Hr, np.float64)[~stored] == 0.0)   # every restatement entry has a place
        r = slice(dof * a, dof * a + dof)
        assert np.array_equal(D[r, r], np.eye(dof)) and not D[r, :r.start].any() and not D[r, r.stop:].any()
        assert not D[:r.start, r].any() and not D[r.stop:, r].any() and not g[r].any()
        assert np.array_equal(D, D.T)                                # symmetric to the bit
        keep = ~lo
        keep[r] = False
        eg = np.abs(np.asarray(g, LD) - gr).astype(np.float64)
        eH = np.abs(np.asarray(D, LD) - Hr).astype(np.float64)
        wg = float((eg[keep] / np.maximum(C["g"] * bg[keep], 1e-300)).max())
        kk = np.outer(keep, keep)
        wH = float((eH[kk] / np.maximum(C["H"] * bH[kk], 1e-300)).max())
        print("%s x %d, anchor %d: g at %.3g, H at %.3g of their bounds (%d poses not held)" % (name, nn, a, wg, wH, int(loose.sum())))
        assert np.all(eg[keep] <= C["g"] * bg[keep]) and np.all(eH[kk] <= C["H"] * bH[kk])
        if not loose.any():
            assert abs(float(LD(F) - Fr)) <= C["F"] * bF
        again = grp.ml_hessian(X, anchor=a)
        assert np.array_equal(again[2], val) and np.array_equal(again[3], g) and again[4] == F
        # k_ml_hessian on an array of sentinels with 64 more on either side: every value written, with the bits it has in the
        # factorisation's array, and no sentinel around them touched
        sentinel = -7.25e-300
        guards, v2 = grp.ml_hessian_guarded(X, len(val), anchor=a, pad=64, sentinel=sentinel)
        assert np.array_equal(guards.view(np.uint64), np.full((2, 64), sentinel).view(np.uint64))
        assert np.array_equal(v2.view(np.uint64), val.view(np.uint64)) and not np.any(v2 == sentinel)


@pytest.mark.parametrize("d", [2, 3])
def test_isotropic_consistency_on_a_noise_free_graph(d):
    """Omega_iso on a graph whose every residual is exactly zero: the Gauss-Newton Hessian is the Riemannian one, so ml_hessian
    equals cov_hessian within the sum of both bounds -- ml's from the restatement; k_cov_hessian's entry is a sum of at most
    4 d products of three factors over the terms of S_pq, which are those of H: 2 (4 d + 2) u times their absolute sum -- and
    ml_polish has nothing to do."""
    E, X = mi.noise_free(d)
    N, dof = E["N"], cr.dof_of(d)
    grp = group_of(E, 2, info=False)
    assert not grp.graph.edge_information()[1]
    ref = mr.edges_all(E, X, LD)
    bnd = mr.edge_bounds(E, X, ref)
    bH = mr.sum_bounds(E, N, ref, bnd)[2]
    absH = mr.assemble(dict(E), X, None, np.float64, per_edge={k: (np.abs(np.asarray(v, np.float64)) if k != "near_pi" else v)
                                                              for k, v in ref.items()})[2]
    n = dof * N
    for a in (0, N - 1):
        ptr, col, val, g, F = grp.ml_hessian(X, anchor=a)
        p2, c2, v2 = grp.cov_hessian(X, anchor=a)
        assert np.array_equal(ptr, p2) and np.array_equal(col, c2)
        Dm = sp.csr_matrix((val, col, ptr), shape=(n, n)).toarray()
        Dc = sp.csr_matrix((v2, c2, p2), shape=(n, n)).toarray()
        tol = C["H"] * bH + 2 * (4 * d + 2) * U * absH
        r = slice(dof * a, dof * a + dof)
        tol[r, :] = 0
        tol[:, r] = 0
        worst = float((np.abs(Dm - Dc) / np.maximum(tol, 1e-300))[tol > 0].max())
        print("d = %d, anchor %d: ml_hessian against cov_hessian at %.3g of the sum of both bounds" % (d, a, worst))
        assert np.all(np.abs(Dm - Dc) <= tol)
        assert F == 0.0 and not g.any()
    Xo, res, log = grp.ml_polish(X)
    assert res.outcome == dpgo_amd.POLISH_CONVERGED and res.steps == 0 and res.factorisations == 0 and np.array_equal(Xo, X)
    assert res.chi2_initial == 0.0 and res.chi2_final == 0.0 and res.near_pi == 0


def test_refusals(fixtures_dir):
    E, X, _, _, _ = case_input(fixtures_dir, "smallGrid3D")
    N = E["N"]
    G = tmh.graph_of(E, 2)
    calls = [lambda g, **kw: g.ml_polish(X, **kw), lambda g, **kw: g.ml_covariance(X, **kw), lambda g, **kw: g.ml_hessian(X, **kw),
             lambda g, **kw: g.ml_eval(X, **{k: v for k, v in kw.items() if k != "anchor"})]
    hub = dpgo_amd.NodeGroup(G, range(2), dpgo_amd.Options.driver(dpgo_amd.LOSS_HUBER, True, max_iterations=0))
    part = dpgo_amd.NodeGroup(G, [0], dpgo_amd.Options.driver(LOSS_NONE, True, max_iterations=0))
    grp = group_of(E, 2)
    other = tmh.graph_of(mi.fixture(fixtures_dir, "tinyGrid3D"), 2)
    bad = E["Om"].copy()
    bad[11, 2, 2] = -1.0
    notspd = tmh.graph_of(dict(E, Om=bad), 2)
    for call in calls:
        for g, kw in ((hub, {}), (part, {}), (grp, dict(graph=other)), (grp, dict(graph=notspd))):
            with pytest.raises(RuntimeError):
                call(g, **kw)
    for call in calls[:3]:
        for a in (N, -1):
            with pytest.raises(RuntimeError):
                call(grp, anchor=a)
    assert grp.ml_eval(X)[3] == 0
