"""The kernels of the measurement sensitivities on the device (dpgo_amd/csrc/sens.hip: k_sens_rhs, k_sens_adjoint,
k_sens_edge), through NodeGroup.sensitivity with want_adjoint: tinyGrid3D x {1, 2} nodes, smallGrid3D x {1, 5} and the d = 2
ladder x 6, anchors 0 and N - 1, at the polished points and with the references of tests/test_gpu_pairs.py (the restated
anchored H, its long-double Cholesky factor, bSigma), k = 1, 16, 17 and 65 columns: the tile edge of the block solve and the
batch edge.  The 65 upstream columns are seeded dense ones (their anchor rows are not zero), one zero column, and the unit
columns of one pose.

Bounds; nothing in them comes from the device.
  lambda   bSigma |c|_1 entrywise against the long-double solve (an entry of H^-1 is within bSigma)
  sens     tests/sens_restatement.py: margin_sens with that bound of lambda, against the long-double restatement at the
           long-double lambda; and, the edge kernel alone, margin_sens with b = 0 against the restatement at the DEVICE's lambda
  the weight-scaling identity  sum_e (kappa_e sens_kappa + tau_e sens_tau) = -lambda^T g for the device's own lambda, within
           sum_e (kappa_e m_kappa + tau_e m_tau) of margin_sens with b = 0
The device's worst figure per case is printed and held below 1.  Bit for bit: a column alone, in a call of 1, 16, 17 columns
and in the reversed call; anchor rows zeroed; the call repeated; a zero column gives zeros.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import newton_restatement as nr  # noqa: E402
import robust_restatement as rr  # noqa: E402
import sens_restatement as sn  # noqa: E402
import solve_restatement as sr  # noqa: E402
import test_gpu_covariance as tgc  # noqa: E402  (its groups; none of its tests is imported)
import test_gpu_pairs as tgp  # noqa: E402  (its polished points and references; none of its tests is imported)

import dpgo_amd  # noqa: E402

pytestmark = pytest.mark.gpu

LD, U = sn.LD, sn.U
CASES = tgp.CASES
K = 65
ZERO_COL = 5

_up = {}


def problem_of(grp):
    """robust_restatement's dict from the group's own graph: the edge order of NodeGroup.sensitivity."""
    G = grp.graph
    return rr.problem(G.d, G.num_poses, *G.edges(), G.num_nodes)


def upstream(fixtures_dir, name, anchor):
    """Once per (fixture, anchor): the 65 columns, the long-double adjoints of the columns with the anchor's rows struck out,
    and bSigma |c|_1 per column."""
    key = (name, anchor)
    if key not in _up:
        R = tgp.reference(fixtures_dir, name, anchor)
        N, d, dof = R["N"], R["d"], R["dof"]
        rng = np.random.default_rng(100 + anchor)
        C = np.asfortranarray(rng.standard_normal((dof * N, K)))
        C[:, ZERO_COL] = 0.0
        pose = (anchor + 1 + int(rng.integers(0, N - 1))) % N
        C[:, K - dof:] = dpgo_amd.unit_upstream(N, d, pose)
        assert np.abs(C[dof * anchor:dof * anchor + dof]).min(axis=0).max() > 0
        Cz = np.array(C)
        Cz[dof * anchor:dof * anchor + dof] = 0.0
        lam = sr.solve_cholesky_ld(R["A"], Cz, R["L"])
        assert not lam[dof * anchor:dof * anchor + dof].any()
        _up[key] = dict(C=C, Cz=np.asfortranarray(Cz), lam=lam, b_lam=R["bSigma"] * np.abs(Cz).sum(axis=0), pose=pose)
    return _up[key]


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name,nn", CASES)
def test_adjoints_and_sensitivities_against_the_restatement(fixtures_dir, name, nn):
    grp = tgc.make_group(fixtures_dir, name, nn)
    P = problem_of(grp)
    N, m = P["N"], len(P["I"])
    for a in (0, N - 1):
        R = tgp.reference(fixtures_dir, name, a)
        Up = upstream(fixtures_dir, name, a)
        X, dof = R["X"], R["dof"]
        res, sens, lam = grp.sensitivity(X, Up["C"], anchor=a, want_adjoint=True)
        assert res.outcome == dpgo_amd.SENS_OK and res.unknowns == dof * N and res.fronts >= 1 and res.device_bytes > 0
        assert (res.columns, res.batches, res.edges) == (K, 2, m) and res.pivot_min > 0 and res.stationarity < 1e-5
        assert sens.shape == (K, m, 2 + dof) and lam.shape == (dof * N, K)
        assert not lam[dof * a:dof * a + dof].any() and not lam[:, ZERO_COL].any() and not sens[ZERO_COL].any()
        worst = np.zeros(4)
        worst[0] = float(np.max(np.abs(np.asarray(lam, LD) - Up["lam"]) / (Up["b_lam"][None, :] + 1e-300)))
        want = np.moveaxis(sn.sens_edge(P, X, Up["lam"], LD), 1, 0)
        margin = np.moveaxis(sn.margin_sens(P, X, np.asarray(Up["lam"], np.float64), Up["b_lam"]), 1, 0)
        live = np.arange(K) != ZERO_COL
        worst[1] = float(np.max(np.abs(np.asarray(sens, LD) - want)[live] / (margin[live] + 1e-300)))
        # the edge kernel alone: at the device's own adjoints
        own = np.moveaxis(sn.sens_edge(P, X, lam, LD), 1, 0)
        m0 = np.moveaxis(sn.margin_sens(P, X, lam), 1, 0)
        worst[2] = float(np.max(np.abs(np.asarray(sens, LD) - own)[live] / (m0[live] + 1e-300)))
        # scaling every weight moves nothing: -sum (kappa sens_kappa + tau sens_tau) = lambda^T g, g the gradient at X
        g = nr.grad(rr.weighted_matrix(P, np.ones(m), LD), np.asarray(X, LD), P["d"])
        kap, tau = np.asarray(P["kappa"], LD), np.asarray(P["tau"], LD)
        got = -np.sum(kap[None] * np.asarray(sens[..., 0], LD) + tau[None] * np.asarray(sens[..., 1], LD), axis=1)
        m_id = np.sum(P["kappa"][None] * m0[..., 0] + P["tau"][None] * m0[..., 1], axis=1)
        worst[3] = float(np.max(np.abs(got - np.asarray(lam, LD).T @ g)[live] / (m_id[live] + 1e-300)))
        print("%s x %d, anchor %d: lambda %.3g, sens %.3g, the edge kernel alone %.3g, the weight-scaling identity %.3g of their bounds"
              % ((name, nn, a) + tuple(worst)))
        assert worst.max() < 1.0, worst
        # the sensitivities are there to be checked: far above the edge kernel's margin on most entries
        assert np.median(np.abs(sens[live]) / m0[live]) > 1e6
        # the unit columns: lambda is a column of H^-1
        tgp.need(R, [(Up["pose"], Up["pose"])])
        cols = np.arange(dof * Up["pose"], dof * Up["pose"] + dof)
        assert np.abs(np.asarray(lam[:, K - dof:], LD) - R["Sigma"][:, cols]).max() <= R["bSigma"]


@pytest.mark.parametrize("name,nn", CASES)
def test_a_columns_bits_do_not_depend_on_its_companions(fixtures_dir, name, nn):
    grp = tgc.make_group(fixtures_dir, name, nn)
    N = grp.graph.num_poses
    for a in (0, N - 1):
        R = tgp.reference(fixtures_dir, name, a)
        Up = upstream(fixtures_dir, name, a)
        X, C = R["X"], Up["C"]
        _, sens, lam = grp.sensitivity(X, C, anchor=a, want_adjoint=True)
        # 1, 16, 17 columns: the first columns of the 65
        for k in (1, 16, 17):
            res, s, l = grp.sensitivity(X, C[:, :k], anchor=a, want_adjoint=True)
            assert (res.columns, res.batches) == (k, 1)
            assert np.array_equal(s, sens[:k]) and np.array_equal(l, lam[:, :k]), k
        # a column of each batch alone (a 1-D upstream), and without the adjoint asked for
        for col in (40, 64):
            res, s = grp.sensitivity(X, C[:, col], anchor=a)
            assert s.shape == sens[:1].shape and np.array_equal(s[0], sens[col]), col
        # the columns reversed
        _, s, l = grp.sensitivity(X, C[:, ::-1], anchor=a, want_adjoint=True)
        assert np.array_equal(s[::-1], sens) and np.array_equal(l[:, ::-1], lam)
        # the anchor's rows zeroed; the call repeated
        assert same(grp.sensitivity(X, Up["Cz"], anchor=a, want_adjoint=True)[1:], (sens, lam))
        assert same(grp.sensitivity(X, C, anchor=a, want_adjoint=True)[1:], (sens, lam))
        # linear in the column: twice the column, twice the bits
        _, s2 = grp.sensitivity(X, 2.0 * C[:, 7], anchor=a)
        assert np.array_equal(s2[0], 2.0 * sens[7])


def test_another_graph_of_the_same_poses_gives_its_own_edge_order(fixtures_dir):
    """graph=: the edges of the argument, in its order -- here the group's graph with two edges dropped."""
    grp = tgc.make_group(fixtures_dir, "smallGrid3D", 2)
    R = tgp.reference(fixtures_dir, "smallGrid3D", 0)
    Up = upstream(fixtures_dir, "smallGrid3D", 0)
    keep = np.ones(grp.graph.num_edges, bool)
    keep[[3, 50]] = False
    _, full = grp.sensitivity(R["X"], Up["C"][:, :3])
    _, part = grp.sensitivity(R["X"], Up["C"][:, :3], graph=grp.graph.filter_edges(keep))
    assert part.shape[1] == keep.sum() and np.array_equal(part, full[:, keep])
