"""The kernels of the robust objective (dpgo_amd/csrc/robust.hip: k_robust_edge, k_robust_gather, k_robust_mval,
k_robust_rank1 behind k_cov_hessian) through the debug calls robust_hessian / robust_matrix, entry by entry against the
long-double restatement (tests/robust_restatement.py: reference) within its first-order bounds, which
tests/test_robust_host.py holds the fp64 restatement to on the same inputs.

Inputs: tinyGrid3D on 2 nodes at its chordal point (fewer than 64 edges); edge_restatement.random_graph(d, 70, N=20) and
(d, 160, N=40) on 4 nodes (a partial last workgroup, parallel and reversed edges); the compacted synthetic.inter_ladder(d) on
4 nodes at its ground truth with delta = its kink 0.25 (a hub with 300 incidences, poses with 0 ... 40 incidences, 48 edges
within 10 % of the kink on both sides, none closer than 0.1 %, Welsch weights that reach exactly 0.0).  Compacting keeps every
incidence list but not the node sizes: the graph loader cuts the 200 poses into 4 nodes of 50.  What the uncompacted graph's
node sizes were for is covered by inputs of their own: the same ladder on 2 nodes of 100 poses and random_graph(d, 600, N=150)
on 2 nodes of 75 (every node spans the 64-row segment boundary, with a tail in its second segment, and the partial sums have
four segments), and random_graph(d, 40, N=5) on 4 nodes of 2, 1, 1, 1 poses (one-pose nodes, each a segment of one row).

The equalities -- loss 0 against cert_matrix / cov_hessian, curvature 0 against cov_hessian of the group built from
scale_edges(w) -- are held to the sum of the two sides' bounds against the same long-double reference.  s_rot, s_trans, rho
and w are compared with EdgeEval's bit for bit, and F within tests/test_gpu_edges.py's tolerance.
"""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_restatement as cr  # noqa: E402
import robust_inputs as ri  # noqa: E402
import robust_restatement as rr  # noqa: E402

import dpgo_amd  # noqa: E402
from oracle.problem import LOSS_GM, LOSS_HUBER, LOSS_NONE, LOSS_WELSCH  # noqa: E402

pytestmark = pytest.mark.gpu

LD = np.longdouble
INPUTS = ["tiny", "rand2_70", "rand3_70", "rand2_160", "rand3_160", "ladder2", "ladder3", "rand2_600", "rand3_600", "rand2_40", "rand3_40",
          "ladder2x2", "ladder3x2"]
DELTA = {n: (0.25 if n.startswith("ladder") else 5.0) for n in INPUTS}
LOSSES = (LOSS_HUBER, LOSS_GM, LOSS_WELSCH)

_groups = {}


def objects(name):
    """(P, X, graph, trivial-loss group) of an input, one group per process."""
    if name not in _groups:
        P, X = ri.named(name)
        G = ri.graph(P)
        _groups[name] = (P, X, G, ri.group(G))
    return _groups[name]


def dense(ptr, col, val):
    n = len(ptr) - 1
    return sp.csr_matrix((val, col, ptr), shape=(n, n)).toarray()


def ratio(got, want, bound):
    err = np.abs(np.asarray(np.asarray(got, LD) - want, np.float64))
    assert np.all(np.isfinite(bound))
    return float(np.max(err / np.maximum(bound, 1e-300))), bool(np.all(err <= bound))


@pytest.mark.parametrize("name", INPUTS)
def test_hessian_gradient_and_per_edge_values_against_the_restatement(name):
    P, X, G, grp = objects(name)
    d, N, dl = P["d"], P["N"], DELTA[name]
    dof = cr.dof_of(d)
    ev = dpgo_amd.EdgeEval(G)
    for loss in LOSSES:
        R = ri.reference(name, loss, dl)
        ptr, col, val, g, F, w, c, (s_rot, s_trans, rho) = grp.robust_hessian(X, loss, dl, curvature=1, anchor=0, edges=True)
        # the edge pass: EdgeEval's values bit for bit, F within its tolerance, c within its bound with no edge left out
        sr_e, st_e, rho_e, w_e, sm = ev.run(X, loss, dl)
        for got, want in ((s_rot, sr_e), (s_trans, st_e), (rho, rho_e), (w, w_e)):
            assert np.array_equal(got.view(np.int64), want.view(np.int64))
        assert abs(F - float(R["F"])) <= R["bF"] and abs(F - sm.F) <= R["bF"]
        assert np.all(np.isfinite(R["bc"]))
        rc, ok = ratio(c, R["c"], R["bc"])
        assert ok, rc
        assert np.all(c[~P["inter"]] == 0.0) and np.all(c <= 0.0) and np.all(c[w == 0.0] == 0.0)
        if loss == LOSS_HUBER:
            s = np.asarray(R["s"], np.float64)
            assert np.array_equal(c != 0.0, P["inter"] & (s > dl))     # (no edge within the bound of s of the kink)
        rg, ok = ratio(g, R["g"], R["bg"])
        assert ok, rg
        H = dense(ptr, col, val)
        rh, ok = ratio(H, R["H"], R["bH"])
        print("%s loss %d: error / bound of c %.3f, g %.3f, H %.3f; %d edges with curvature" % (name, loss, rc, rg, rh, int(np.sum(c != 0))))
        assert ok, rh
        # the same bits on a second call
        again = grp.robust_hessian(X, loss, dl, curvature=1, anchor=0)
        assert all(np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))
                   for a, b in zip((val, g, w, c), (again[2], again[3], again[5], again[6]))) and again[4] == F
    node_of = np.searchsorted(np.cumsum([G.node_sizes(a)[0] for a in range(G.num_nodes)]), np.arange(N), side="right")
    sizes = np.bincount(node_of, minlength=G.num_nodes)
    if name.endswith("_600") or name.endswith("x2"):
        assert sizes.min() > 64 and (sizes % 64).min() > 0      # every node: a full segment and a tail in the next
    if name.endswith("_40"):
        assert sorted(sizes.tolist()) == [1, 1, 1, 2]
    if name.startswith("ladder"):
        near = P["inter"] & (np.abs(np.asarray(ri.reference(name, LOSS_HUBER, dl)["s"], np.float64) / dl - 1.0) <= 0.1)
        s = np.asarray(ri.reference(name, LOSS_HUBER, dl)["s"], np.float64)
        print("%s: %d inter-node edges within 10 %% of the kink, %d below; Welsch weights that are exactly 0: %d" %
              (name, int(near.sum()), int((near & (s < dl)).sum()), int(np.sum(grp.robust_hessian(X, LOSS_WELSCH, dl)[5] == 0.0))))
        assert (near & (s < dl)).any() and (near & (s > dl)).any()
        assert np.sum(grp.robust_hessian(X, LOSS_WELSCH, dl)[5] == 0.0) > 0
        assert np.bincount(np.concatenate([P["I"], P["J"]])).max() >= 300


@pytest.mark.parametrize("name", INPUTS)
def test_matrix_against_the_restatement_and_symmetric_to_the_bit(name):
    P, X, G, grp = objects(name)
    d, N, dl = P["d"], P["N"], DELTA[name]
    for loss in LOSSES:
        R = ri.reference(name, loss, dl)
        ptr, col, val = grp.robust_matrix(X, loss, dl)
        M = dense(ptr, col, val)
        assert np.array_equal(M.view(np.int64), np.ascontiguousarray(M.T).view(np.int64))
        r, ok = ratio(M, rr.to_pose_major(R["M"], N, d), rr.to_pose_major(R["bM"], N, d))
        print("%s loss %d: error / bound of M_w %.3f" % (name, loss, r))
        assert ok, r
        again = grp.robust_matrix(X, loss, dl)[2]
        assert np.array_equal(val.view(np.int64), again.view(np.int64))


@pytest.mark.parametrize("name", ["tiny", "rand2_160", "rand3_70", "ladder3"])
def test_trivial_loss_is_the_certificate_matrix_and_the_covariance_hessian(name):
    P, X, G, grp = objects(name)
    d, N = P["d"], P["N"]
    R = ri.reference(name, LOSS_NONE, 1.0)
    Mr = dense(*grp.robust_matrix(X, LOSS_NONE))
    S = dense(*grp.cert_matrix(X, 0.0))
    Lam = grp.cert_lambda(X)
    B = d + 1
    for p in range(N):                                    # cert_matrix without Lambda: S + blkdiag(0, Lambda)
        S[B * p + 1:B * p + B, B * p + 1:B * p + B] += Lam[p]
    bM = rr.to_pose_major(R["bM"], N, d)
    bL = 8 * rr.U * np.abs(Lam).max()                     # (Lambda subtracted and added back: two roundings at its size, a few for its own sum)
    assert np.all(np.abs(Mr - S) <= 2 * bM + bL)
    r, ok = ratio(Mr, rr.to_pose_major(R["M"], N, d), bM)
    assert ok, r
    for curv in (0, 1):
        Hr = dense(*grp.robust_hessian(X, LOSS_NONE, curvature=curv)[:3])
        Hc = dense(*grp.cov_hessian(X))
        assert np.all(np.abs(Hr - Hc) <= 2 * R["bH"])
        r, ok = ratio(Hr, R["H"], R["bH"])
        assert ok, r


@pytest.mark.parametrize("name", ["tiny", "rand2_160", "rand3_70", "ladder2"])
def test_curvature_0_is_the_covariance_hessian_of_the_scaled_graph(name):
    P, X, G, grp = objects(name)
    dl = DELTA[name]
    for loss in LOSSES:
        R = ri.reference(name, loss, dl, curvature=0)
        ptr, col, val, g, F, w, c = grp.robust_hessian(X, loss, dl, curvature=0)
        H0 = dense(ptr, col, val)
        r, ok = ratio(H0, R["H"], R["bH"])
        assert ok, r
        Gw = G.scale_edges(w)
        Hs = dense(*ri.group(Gw).cov_hessian(X))
        assert np.all(np.abs(H0 - Hs) <= 2 * R["bH"])
        print("%s loss %d: curvature 0 against the restatement %.3f of the bound; against the scaled graph's cov_hessian max %.3g" %
              (name, loss, r, float(np.abs(H0 - Hs).max())))


@pytest.mark.parametrize("name", ["rand2_70", "rand3_160"])
def test_anchor_rows_and_columns_are_the_identity(name):
    P, X, G, grp = objects(name)
    d, N, dl = P["d"], P["N"], DELTA[name]
    dof = cr.dof_of(d)
    with_inter = int(P["I"][np.nonzero(P["inter"])[0][0]])
    for a in (0, N - 1, with_inter):
        R = ri.reference(name, LOSS_GM, dl, anchor=a)
        ptr, col, val, g, F, w, c = grp.robust_hessian(X, LOSS_GM, dl, curvature=1, anchor=a)
        H = dense(ptr, col, val)
        r = slice(dof * a, dof * a + dof)
        assert np.array_equal(H[r, r], np.eye(dof)) and not H[r, :r.start].any() and not H[r, r.stop:].any()
        assert not H[:r.start, r].any() and not H[r.stop:, r].any() and not g[r].any()
        q, ok = ratio(H, R["H"], R["bH"])
        assert ok, q
