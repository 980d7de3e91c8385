"""PCM host parts (no GPU): the max-clique solvers against networkx, the numpy restatement of PCM::update on a
hand-built case, and Graph.filter_edges."""
import os
import sys

import networkx as nx
import numpy as np
import pytest

import dpgo_amd
from dpgo_amd import synthetic

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pcm_restatement as pr  # noqa: E402


def _gnp(n, p, seed):
    rng = np.random.default_rng(seed)
    A = np.triu(rng.random((n, n)) < p, 1)
    return (A | A.T).astype(np.uint8)


def _nx_clique_number(A):
    if len(A) == 0:
        return 0
    G = nx.from_numpy_array(A - np.diag(np.diag(A)))
    return len(nx.max_weight_clique(G, weight=None)[0])


def _is_clique(A, sel):
    idx = np.nonzero(sel)[0]
    sub = A[np.ix_(idx, idx)] | np.eye(len(idx), dtype=A.dtype)
    return bool(np.all(sub))


def _check(A):
    ex, he = dpgo_amd.max_clique(A, True), dpgo_amd.max_clique(A, False)
    assert ex.shape == he.shape == (len(A),)
    assert _is_clique(A, ex) and _is_clique(A, he)
    assert ex.sum() == _nx_clique_number(A)
    assert he.sum() <= ex.sum()
    return ex, he


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("n,seed", [(12, 1), (33, 2), (60, 3), (64, 4), (65, 5)])
def test_max_clique_gnp_against_networkx(n, p, seed):
    if p == 0.9 and n > 60:
        n = 60
    _check(_gnp(n, p, seed))


@pytest.mark.parametrize("n,k,seed", [(60, 12, 7), (100, 30, 8), (130, 70, 9)])
def test_max_clique_planted(n, k, seed):
    A = _gnp(n, 0.2, seed)
    rng = np.random.default_rng(seed)
    members = rng.choice(n, k, replace=False)
    A[np.ix_(members, members)] = 1
    np.fill_diagonal(A, 0)
    ex, he = _check(A)
    assert ex.sum() == k
    np.testing.assert_array_equal(np.nonzero(ex)[0], np.sort(members))


def test_max_clique_trivial_graphs():
    assert dpgo_amd.max_clique(np.zeros((0, 0)), True).shape == (0,)
    assert dpgo_amd.max_clique(np.zeros((0, 0)), False).shape == (0,)
    for exact in (True, False):
        assert dpgo_amd.max_clique(np.zeros((1, 1)), exact).tolist() == [True]
        assert dpgo_amd.max_clique(np.ones((1, 1)), exact).tolist() == [True]
        e = dpgo_amd.max_clique(np.zeros((7, 7)), exact)        # empty graph: one vertex
        assert e.sum() == 1
        assert dpgo_amd.max_clique(np.ones((70, 70)), exact).all()   # complete graph (diagonal ignored)
    # asymmetric input: A | A^T
    A = np.zeros((3, 3), np.uint8)
    A[0, 1] = A[2, 0] = A[1, 2] = 1
    assert dpgo_amd.max_clique(A, True).all()


def _rot2(th):
    c, s = np.cos(th), np.sin(th)
    return np.array([[c, -s], [s, c]])


def _hand_case(delta):
    """Two nodes (poses 0,1 | 2,3), d = 2: poses at known positions, measurements 0->2 and 3->1 (the second
    reversed) exactly consistent with the poses, then the translation of the second perturbed by delta."""
    N, d = 4, 2
    Rs = [_rot2(a) for a in (0.3, -0.7, 1.1, 2.0)]
    ts = [np.array(v, float) for v in ((0, 0), (5, 1), (-2, 3), (7, -4))]
    X = np.zeros(((d + 1) * N, d))
    for i in range(N):
        X[i] = ts[i]
        X[N + d * i:N + d * i + d] = Rs[i].T
    rel = lambda i, j: (Rs[i].T @ Rs[j], Rs[i].T @ (ts[j] - ts[i]))
    I = np.array([0, 3, 0, 2])
    J = np.array([2, 1, 1, 3])
    R = np.stack([rel(i, j)[0] for i, j in zip(I, J)])
    t = np.stack([rel(i, j)[1] for i, j in zip(I, J)])
    t[1] = t[1] + delta
    node_of = np.array([0, 0, 1, 1])
    kap, tau = np.full(4, 3.0), np.full(4, 5.0)
    return I, J, R, t, kap, tau, node_of, X


@pytest.mark.parametrize("delta", [(0.0, 0.0), (0.01, 0.0), (-0.003, 0.004), (0.5, -1.2)])
def test_restatement_hand_case(delta):
    I, J, R, t, kap, tau, node_of, X = _hand_case(np.array(delta))
    meas, A, E = pr.update(0, 1, I, J, R, t, kap, tau, node_of, X, tolerance=0.2)
    np.testing.assert_array_equal(meas, [0, 1])            # intra-node edges are not measurements of the pair
    err = np.hypot(*delta)
    np.testing.assert_allclose(E[0, 1], err, atol=1e-12)    # the rotation cycle is exact; translation error |delta|
    assert E[0, 1] == E[1, 0]
    assert A[0, 1] == (err <= 0.2) and A[0, 0] == A[1, 1] == 1
    # weighted: sqrt(tau) |delta| (kappa, tau the pair's means)
    _, _, Ew = pr.update(0, 1, I, J, R, t, kap, tau, node_of, X, weighted=True)
    np.testing.assert_allclose(Ew[0, 1], np.sqrt(5.0) * err, atol=1e-12)
    # the scalar form agrees with the vectorised one; the order of alpha and beta does not change the error
    _, _, Eba = pr.update(1, 0, I, J, R, t, kap, tau, node_of, X)
    np.testing.assert_allclose(Eba[0, 1], err, atol=1e-12)


def test_restatement_scalar_matches_vectorised():
    g = synthetic.grid(4, 4, 4, 250, seed=3, sigma_t=0.05, sigma_r=0.02)
    N = g["num_poses"]
    X = np.zeros((4 * N, 3))
    X[:N] = np.stack([np.arange(N) % 4, (np.arange(N) // 4) % 4, np.arange(N) // 16], 1)
    X[N:] = np.tile(np.eye(3), (N, 1))
    node_of = np.arange(N) // (N // 2)
    meas, A, E = pr.update(0, 1, g["I"], g["J"], g["R"], g["t"], g["kappa"], g["tau"], node_of, X)
    assert len(meas) > 10
    rl = pr.roles(0, 1, g["I"], g["J"], g["R"], g["t"], node_of, meas)
    for p, q in [(0, 1), (2, 7), (3, len(meas) - 1)]:
        P, Q = rl[p], rl[q]
        poses = [pr.pose(X, N, 3, k) for k in (P[0], Q[0], P[1], Q[1])]
        e = pr.pair_error([poses[0][0], poses[1][0]], [poses[0][1], poses[1][1]], [poses[2][0], poses[3][0]],
                          [poses[2][1], poses[3][1]], P[2], P[3], Q[4], Q[5])
        np.testing.assert_allclose(E[p, q], e, rtol=1e-13, atol=1e-14)


def test_filter_edges_round_trip(fixtures_dir):
    G = dpgo_amd.read_g2o(os.path.join(fixtures_dir, "smallGrid3D.g2o"), 3)
    rng = np.random.default_rng(11)
    I, J, R, t, kap, tau = G.edges()
    # drop some non-chain edges (every pose keeps its odometry edge)
    keep = (np.abs(I - J) == 1) | (rng.random(G.num_edges) < 0.6)
    F = G.filter_edges(keep)
    assert (F.d, F.num_poses, F.num_nodes, F.num_edges) == (G.d, G.num_poses, G.num_nodes, int(keep.sum()))
    for a, b in zip(F.edges(), (I, J, R, t, kap, tau)):
        np.testing.assert_array_equal(a, b[keep])
    for n in range(3):
        assert F.node_offset(n) == G.node_offset(n)
    assert G.filter_edges(np.ones(G.num_edges, bool)).num_edges == G.num_edges
    with pytest.raises(ValueError):
        G.filter_edges(np.zeros(G.num_edges, bool))
    with pytest.raises(ValueError):
        G.filter_edges(keep[:-1])


def test_pose_nodes_matches_partition(fixtures_dir):
    G = dpgo_amd.read_g2o(os.path.join(fixtures_dir, "M3500.g2o"), 4)
    node = dpgo_amd.pose_nodes(G)
    for a in range(4):
        n0 = G.node_sizes(a)[0]
        assert (node == a).sum() == n0
