"""Marginal covariances of the robust objective on the device (Group::robust_covariance: the covariance's factorisation,
selected inversion and read-out on the robust Hessian) against the dense long-double inverse of the restated H
(tests/robust_restatement.py: reference) at the device's polished point, within the bound of tests/test_gpu_covariance.py:
cov_restatement.C u kappa_2(H) / lambda_min + |bH|_2 / lambda_min^2, bH the restatement's bound of the matrix.

Inputs: smallGrid3D on 2 and 5 nodes with Huber 0.25 and random_graph(2, 160, N=40) on 4 nodes with Huber 5, each at the point
robust_polish reaches from the committed start; random_graph(2, 600, N=150) on 2 nodes of 75 poses (every node spans two
64-row segments) and random_graph(3, 40, N=5) on 4 nodes (three of them of one pose), Huber 5, likewise.  curvature 0 is held against covariance_reweighted (each side within its bound
of the same reference).  The indefinite case was found on the CPU: random_graph(2, 160, N=40) at its own X under
Geman-McClure with delta = 1 -- the restated anchored H has lambda_min = -6.2 with the curvature of the loss and is positive
definite without it.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_restatement as cr  # noqa: E402
import factor_restatement as fr  # noqa: E402
import robust_inputs as ri  # noqa: E402
import robust_restatement as rr  # noqa: E402

import dpgo_amd  # noqa: E402
from oracle.problem import LOSS_GM, LOSS_HUBER  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ROWS = {r["name"]: r for r in ri.trajectories()}
CASES = ["small2_huber", "small5_huber", "random2_huber5", "big2_huber5", "ones3_huber5"]

_pt = {}


def polished(name):
    """(P, graph, group, the device's polished point) of a trajectory row."""
    if name not in _pt:
        row = ROWS[name]
        P, X = ri.trajectory_problem(row)
        G = ri.graph(P)
        grp = ri.group(G)
        Xp, res, _, _ = grp.robust_polish(X, row["loss"], row["delta"], graph=G)
        assert res.outcome == dpgo_amd.POLISH_CONVERGED
        _pt[name] = (P, G, grp, Xp)
    return _pt[name]


def dense_reference(P, X, loss, dl, curvature, anchor):
    R = rr.reference(P, X, loss, dl, curvature, anchor)
    lam = np.linalg.eigvalsh(np.asarray(R["H"], np.float64))
    assert lam[0] > 0
    L, kstar, _ = fr.cholesky_ld(R["H"])
    assert kstar < 0
    Xi = fr.lower_inverse_ld(L)
    bSigma = cr.C * U * float(lam[-1] / lam[0]) / float(lam[0]) + float(np.linalg.norm(R["bH"], 2)) / float(lam[0]) ** 2
    return Xi.T @ Xi, bSigma


def blocks_of(Sigma, dof, pairs):
    return np.stack([Sigma[dof * p:dof * p + dof, dof * q:dof * q + dof] for p, q in pairs])


@pytest.mark.parametrize("name", CASES)
def test_marginals_and_edge_blocks_against_the_dense_inverse(name):
    row = ROWS[name]
    P, G, grp, Xp = polished(name)
    loss, dl, N = row["loss"], row["delta"], P["N"]
    dof = cr.dof_of(P["d"])
    edges = np.unique(np.stack([P["I"], P["J"]], axis=1), axis=0).astype(np.int32)
    for anchor in (0, N - 1):
        Sigma, bSigma = dense_reference(P, Xp, loss, dl, 1, anchor)
        marg, cross, res = grp.robust_covariance(Xp, loss, dl, curvature=1, anchor=anchor, pairs=edges, graph=G)
        assert res.outcome == dpgo_amd.COV_OK and res.unknowns == dof * N and res.pivot_min > 0 and res.numeric_ms > 0
        want_m, want_c = blocks_of(Sigma, dof, [(p, p) for p in range(N)]), blocks_of(Sigma, dof, edges)
        touch = (edges == anchor).any(axis=1)
        want_m[anchor] = 0
        want_c[touch] = 0
        assert not marg[anchor].any() and not cross[touch].any()
        em = float(np.abs(np.asarray(marg, fr.LD) - want_m).max()) / bSigma
        ec = float(np.abs(np.asarray(cross, fr.LD) - want_c).max()) / bSigma
        print("%s anchor %d: marginals %.3g, edge blocks %.3g of the bound; stationarity %.3g; max|Sigma| %.3g" %
              (name, anchor, em, ec, res.stationarity, np.abs(marg).max()))
        assert em < 1.0 and ec < 1.0
        # stationarity is |S_w X|_F, held against the restated product and its rounding floor (64 u | |M_w| |X| |_F)
        w = rr.weights(P, Xp, loss, dl)[2]
        M, S = rr.S_w(P, Xp, w)
        ref, floor = float(np.linalg.norm(S @ Xp)), 64 * U * float(np.linalg.norm(np.abs(M) @ np.abs(Xp)))
        assert abs(res.stationarity - ref) <= 1e-6 * ref + floor
        again = grp.robust_covariance(Xp, loss, dl, curvature=1, anchor=anchor, pairs=edges, graph=G)
        assert np.array_equal(again[0], marg) and np.array_equal(again[1], cross)


@pytest.mark.parametrize("name", CASES)
def test_curvature_0_is_the_reweighted_covariance(name):
    row = ROWS[name]
    P, G, grp, Xp = polished(name)
    loss, dl, N = row["loss"], row["delta"], P["N"]
    dof = cr.dof_of(P["d"])
    edges = np.unique(np.stack([P["I"], P["J"]], axis=1), axis=0).astype(np.int32)
    Sigma, bSigma = dense_reference(P, Xp, loss, dl, 0, 0)
    marg, cross, res = grp.robust_covariance(Xp, loss, dl, curvature=0, pairs=edges, graph=G)
    m2, c2, r2, _ = dpgo_amd.covariance_reweighted(G, Xp, loss, dl, pairs=edges)
    assert res.outcome == dpgo_amd.COV_OK and r2.outcome == dpgo_amd.COV_OK
    want_m = blocks_of(Sigma, dof, [(p, p) for p in range(N)])
    want_m[0] = 0
    for got in (marg, m2):
        assert float(np.abs(np.asarray(got, fr.LD) - want_m).max()) < bSigma
    print("%s: curvature 0 against covariance_reweighted: max difference %.3g (bound %.3g)" %
          (name, float(np.abs(marg - m2).max()), 2 * bSigma))
    assert np.abs(marg - m2).max() <= 2 * bSigma and np.abs(cross - c2).max() <= 2 * bSigma
    assert abs(res.stationarity - r2.stationarity) <= 1e-6 * max(res.stationarity, 1e-12) + 1e-9


def test_not_positive_definite_where_the_curvature_of_the_loss_wins():
    P, X = ri.named("rand2_160")
    lam1 = np.linalg.eigvalsh(rr.hessian(P, X, LOSS_GM, 1.0, 1, 0))
    lam0 = np.linalg.eigvalsh(rr.hessian(P, X, LOSS_GM, 1.0, 0, 0))
    assert lam1[0] < -1e-6 * lam1[-1] and lam0[0] > 1e-6 * lam0[-1]      # far from the threshold on both sides
    G = ri.graph(P)
    grp = ri.group(G)
    marg, _, res = grp.robust_covariance(X, LOSS_GM, 1.0, curvature=1, graph=G)
    assert res.outcome == dpgo_amd.COV_NOT_PD and not marg.any()
    marg0, _, res0 = grp.robust_covariance(X, LOSS_GM, 1.0, curvature=0, graph=G)
    assert res0.outcome == dpgo_amd.COV_OK and marg0[1:].any()
    skipped = grp.robust_covariance(X, LOSS_GM, 1.0, max_bytes=1, graph=G)[2]
    assert skipped.outcome == dpgo_amd.COV_SKIPPED and skipped.device_bytes > grp.covariance(X, max_bytes=1)[2].device_bytes
    for bad in (dict(loss=7), dict(loss_reg=-1.0), dict(curvature=3), dict(anchor=-1), dict(pairs=[[0, P["N"]]])):
        kw = dict(loss=LOSS_HUBER, loss_reg=1.0)
        kw.update(bad)
        with pytest.raises(RuntimeError):
            grp.robust_covariance(X, graph=G, **kw)
