"""PCM on the GPU: the device consistency test against the numpy restatement of PCM::update (PCM.cpp:5-235), the
shape ladder of the bit rows, orientation, the argument checks, and outlier recovery on a lattice with planted
outliers, end to end through AMM-PGO#."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import dpgo_amd
from dpgo_amd import LOSS_NONE, synthetic

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pcm_restatement as pr  # noqa: E402

pytestmark = pytest.mark.gpu


def _ref(G, a, b, X, tol, weighted):
    I, J, R, t, kap, tau = G.edges()
    return pr.update(a, b, I, J, R, t, kap, tau, dpgo_amd.pose_nodes(G), X, tolerance=tol, weighted=weighted)


def _neighbour_pairs(G):
    I, J = G.edges()[:2]
    node = dpgo_amd.pose_nodes(G)
    ni, nj = node[I], node[J]
    inter = ni != nj
    return sorted(set(zip(np.minimum(ni, nj)[inter].tolist(), np.maximum(ni, nj)[inter].tolist())))


def _compare(pcm, G, a, b, X, tol, weighted):
    """Device errors and decisions against the restatement; returns the number of decisions checked."""
    m = pcm.update(G, a, b, X, tol, weighted)
    meas, A_ref, E_ref = _ref(G, a, b, X, tol, weighted)
    assert m == len(meas)
    np.testing.assert_array_equal(pcm.measurements(), meas)
    A, E = pcm.adjacency(), pcm.errors()
    scale = max(1.0, float(np.abs(X[:G.num_poses]).max()))
    floor = 1e-12 * scale * (np.sqrt(max(G.edges()[5].max(), 1.0)) if weighted else 1.0)
    np.testing.assert_allclose(E, E_ref, rtol=1e-10, atol=floor)
    assert (A == A.T).all() and (np.diag(A) == 1).all()
    clear = np.abs(E_ref - tol) > 1e-9 * max(1.0, tol)
    np.fill_diagonal(clear, True)
    np.testing.assert_array_equal(A[clear], A_ref[clear])
    # the kernel's bits drive the solvers: both return cliques of the dense matrix, exact = its maximum (exact search
    # is exponential on dense noisy matrices, so only at the smaller sizes)
    if m > 256:
        return int(clear.sum())
    ex, he = pcm.solve_exact(), pcm.solve_heuristic()
    for s in (ex, he):
        idx = np.nonzero(s)[0]
        assert A[np.ix_(idx, idx)].all()
    assert ex.sum() == dpgo_amd.max_clique(A, True).sum() >= he.sum()
    return int(clear.sum())


@pytest.mark.parametrize("name,nn", [("M3500", 4), ("smallGrid3D", 2), ("smallGrid3D", 3)])
@pytest.mark.parametrize("weighted", [False, True])
def test_device_matches_restatement(fixtures_dir, name, nn, weighted):
    G = dpgo_amd.read_g2o(os.path.join(fixtures_dir, name + ".g2o"), nn)
    X = G.chordal_initialization()
    pcm = dpgo_amd.PCM()
    pairs = _neighbour_pairs(G)
    assert pairs
    for a, b in pairs:
        _, _, E = _ref(G, a, b, X, 0.2, weighted)
        off = E[~np.eye(len(E), dtype=bool)]
        tol = float(np.median(off)) if off.size else 0.2     # both decisions occur
        _compare(pcm, G, a, b, X, tol, weighted)
        A = pcm.adjacency()
        if len(A) > 2:
            assert 0 < A.sum() - len(A) < len(A) * (len(A) - 1)
        # alpha and beta swapped: the same measurements in the other roles (the reference's error is not symmetric in
        # alpha and beta -- the cycle's translation depends on its base frame -- so it is compared, not equated)
        _compare(pcm, G, b, a, X, tol, weighted)


def _two_node_graph(g):
    return dpgo_amd.graph_from_edges(3, g["num_poses"], g["I"], g["J"], g["R"], g["t"], g["kappa"], g["tau"], 2)


@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 127, 128, 129, 1000])
def test_shape_ladder(m):
    g = synthetic.two_node(1000, seed=4)
    G0 = _two_node_graph(g)
    I, J = G0.edges()[:2]
    node = dpgo_amd.pose_nodes(G0)
    cross = np.nonzero(node[I] != node[J])[0]
    keep = node[I] == node[J]
    keep[cross[:m]] = True
    G = G0.filter_edges(keep)
    X = synthetic.global_X(g["Rg"], g["tg"])
    pcm = dpgo_amd.PCM()
    assert _compare(pcm, G, 0, 1, X, 0.2, False) >= m
    A = pcm.adjacency()
    assert A.shape == (m, m)
    if m >= 64:
        assert 0 < A.sum() - m < m * (m - 1)   # both decisions at the chunk edges


def test_orientation_reversal_keeps_decisions():
    g = synthetic.two_node(300, seed=6)
    X = synthetic.global_X(g["Rg"], g["tg"])
    G = _two_node_graph(g)
    rev = np.arange(len(g["I"])) % 3 == 0
    I2, J2 = np.where(rev, g["J"], g["I"]), np.where(rev, g["I"], g["J"])
    R2 = np.where(rev[:, None, None], np.swapaxes(g["R"], 1, 2), g["R"])
    t2 = np.where(rev[:, None], -np.einsum("eba,eb->ea", g["R"], g["t"]), g["t"])
    G2 = dpgo_amd.graph_from_edges(3, g["num_poses"], I2, J2, R2, t2, g["kappa"], g["tau"], 2)
    pcm = dpgo_amd.PCM()
    m = pcm.update(G, 0, 1, X)
    A, E = pcm.adjacency(), pcm.errors()
    assert pcm.update(G2, 0, 1, X) == m
    node = dpgo_amd.pose_nodes(G)
    np.testing.assert_array_equal(pcm.measurements(), np.nonzero(node[g["I"]] != node[g["J"]])[0])
    A2, E2 = pcm.adjacency(), pcm.errors()
    np.testing.assert_allclose(E2, E, rtol=1e-10, atol=1e-11)
    clear = np.abs(E - 0.2) > 1e-9
    np.testing.assert_array_equal(A2[clear], A[clear])
    assert 0 < A.sum() - m < m * (m - 1)


def _lattice():
    nx_, ny_, nz_, nn = 8, 8, 12, 4     # z-slabs of 3 layers: closures (Chebyshev distance <= 2) join neighbouring slabs
    N = nx_ * ny_ * nz_
    g = synthetic.grid(nx_, ny_, nz_, 3 * N + 1200, seed=5, outlier_frac=0.15, sigma_r=1e-3, sigma_t=1e-2)
    G = dpgo_amd.graph_from_edges(3, N, g["I"], g["J"], g["R"], g["t"], g["kappa"], g["tau"], nn)
    ids = np.arange(N)
    t = np.stack([ids % nx_, (ids // nx_) % ny_, ids // (nx_ * ny_)], 1).astype(float)
    X = synthetic.global_X(np.tile(np.eye(3), (N, 1, 1)), t)
    return g, G, X


def test_outlier_recovery():
    g, G, X = _lattice()
    node = dpgo_amd.pose_nodes(G)
    ni, nj = node[g["I"]], node[g["J"]]
    pairs = _neighbour_pairs(G)
    assert pairs == [(0, 1), (1, 2), (2, 3)]
    pcm = dpgo_amd.PCM()
    for a, b in pairs:
        m = pcm.update(G, a, b, X)
        ids = pcm.measurements()
        out = g["outlier"][ids]
        assert m == len(ids) and out.sum() >= 5 and (~out).sum() >= 5, (a, b, m, out.sum())
        np.testing.assert_array_equal(pcm.solve_exact(), ~out)
        np.testing.assert_array_equal(pcm.solve_heuristic(), ~out)
    keep = dpgo_amd.pcm_inliers(G, X)
    inter = ni != nj
    np.testing.assert_array_equal(keep[inter], ~g["outlier"][inter])
    assert keep[~inter].all()
    assert (keep == dpgo_amd.pcm_inliers(G, X, exact=False)).all()

    # AMM-PGO# from the ground truth, once on the filtered graph and once on the unfiltered one
    def rot_error(graph):
        run = dpgo_amd.DistPGO(graph, dpgo_amd.Options.driver(LOSS_NONE, True), X0=X)
        for _ in range(10):
            assert run.step() == 0
        Y = run.X()
        N = graph.num_poses
        R = np.swapaxes(Y[N:].reshape(N, 3, 3), 1, 2)
        R = np.einsum("ba,nbc->nac", R[0], R)       # gauge: R_0^T R_i
        return float(np.sqrt(np.mean(np.sum((R - np.eye(3)) ** 2, axis=(1, 2)))))

    # (the same start and iteration count on the CPU oracle give the same two numbers, 0.444 and 0.532)
    e_filtered, e_raw = rot_error(G.filter_edges(keep)), rot_error(G)
    assert np.isfinite(e_filtered) and e_filtered < 0.9 * e_raw, (e_filtered, e_raw)


def test_argument_checks():
    g, G, X = _lattice()
    pcm = dpgo_amd.PCM()
    for a, b in [(1, 1), (0, 4), (-1, 0), (0, 7)]:
        with pytest.raises(ValueError):
            pcm.update(G, a, b, X)
    L = dpgo_amd.lib()
    assert L.dpgo_pcm_update(pcm._h, G._h, 0, 1, None, X.shape[0], None) == -1
    Xf = np.asfortranarray(X)
    assert L.dpgo_pcm_update(pcm._h, G._h, 0, 1, Xf.ctypes.data_as(C.POINTER(C.c_double)), X.shape[0] - 1, None) == -1
    # nodes 0 and 2 share no edge: m = 0, empty results
    assert pcm.update(G, 0, 2, X) == 0
    assert pcm.measurements().shape == (0,) and pcm.adjacency().shape == (0, 0)
    assert pcm.solve_exact().shape == (0,) and pcm.errors().shape == (0, 0)
    # defaults through a NULL options pointer
    assert L.dpgo_pcm_update(pcm._h, G._h, 0, 1, Xf.ctypes.data_as(C.POINTER(C.c_double)), X.shape[0], None) > 0
