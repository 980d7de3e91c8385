"""NodeGroup.sensitivity / dpgo_group_sensitivity on the device (dpgo_amd/csrc/sens.h): the outcomes SKIPPED and NOT_PD, every
refusal, the unit columns of a pose against NodeGroup.pair_covariance, and the front ends (dist_pgo --sensitivity_pose, the C++
facade).  Points and references are those of tests/test_gpu_pairs.py; the arithmetic is held to the restatement in
tests/test_gpu_sens_ops.py.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cert_restatement as cert  # noqa: E402
import cov_restatement as cr  # noqa: E402
import test_gpu_certify as tc  # noqa: E402
import test_gpu_covariance as tgc  # noqa: E402  (its groups; none of its tests is imported)
import test_gpu_cert_proof as tp  # noqa: E402
import test_gpu_pairs as tgp  # noqa: E402  (its polished points and references; none of its tests is imported)

import dpgo_amd  # noqa: E402
from oracle.problem import LOSS_NONE  # noqa: E402

pytestmark = pytest.mark.gpu


def columns(R, k, seed=3):
    return np.asfortranarray(np.random.default_rng(seed).standard_normal((R["dof"] * R["N"], k)))


def raw_call(grp, graph, X, Uc, k, adjoint, sens, res, anchor=0, max_bytes=0, ldu=None):
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    return dpgo_amd.lib().dpgo_group_sensitivity(grp._h if grp else None, graph._h if graph else None, dp(X), X.shape[0], anchor, max_bytes,
                                                 dp(Uc), Uc.shape[0] if ldu is None else ldu, k, dp(adjoint), dp(sens),
                                                 C.byref(res) if res is not None else None)


def test_skipped_leaves_the_outputs_alone_and_allocates_nothing(fixtures_dir):
    R = tgp.reference(fixtures_dir, "smallGrid3D", 0)
    grp = tgc.make_group(fixtures_dir, "smallGrid3D", 2)
    X, Uc = np.asfortranarray(R["X"]), columns(R, 3)
    m, dof, n = grp.graph.num_edges, R["dof"], R["dof"] * R["N"]
    res = dpgo_amd.SensResult()
    sens, adj = np.full((3, m, 2 + dof), 7.0), np.full((n, 3), 7.0, order="F")
    assert raw_call(grp, grp.graph, X, Uc, 3, adj, sens, res, max_bytes=1) == 0   # (the certificate's buffers and M's values come here)
    free0 = tgp.device_free_bytes()
    assert raw_call(grp, grp.graph, X, Uc, 3, adj, sens, res, max_bytes=1) == 0
    assert tgp.device_free_bytes() == free0
    assert res.outcome == dpgo_amd.SENS_SKIPPED and np.all(sens == 7.0) and np.all(adj == 7.0)
    assert res.unknowns == n and res.fronts >= 4 and res.levels >= 1 and res.max_front > 0 and res.device_bytes > 1
    assert (res.columns, res.batches, res.edges) == (3, 1, m) and res.stationarity > 0
    # the prediction is the threshold: one byte less is refused, the prediction itself runs
    assert grp.sensitivity(X, Uc, max_bytes=res.device_bytes - 1)[0].outcome == dpgo_amd.SENS_SKIPPED
    ok, s = grp.sensitivity(X, Uc, max_bytes=res.device_bytes)
    assert ok.outcome == dpgo_amd.SENS_OK and ok.device_bytes == res.device_bytes and s.any()
    # the call's own buffers are counted: more columns, more edges' worth of output
    more = grp.sensitivity(X, columns(R, 64), max_bytes=1)[0]
    assert more.device_bytes >= res.device_bytes + 8 * (64 - 16) * n + 8 * (64 - 3) * (n + m * (2 + dof))
    assert grp.sensitivity(X, columns(R, 200), max_bytes=1)[0].device_bytes == more.device_bytes   # (a batch at a time)


def test_a_point_that_is_no_minimum(fixtures_dir):
    R = tgp.reference(fixtures_dir, "smallGrid3D", 0)
    grp = tgc.make_group(fixtures_dir, "smallGrid3D", 2)
    N, mm, gp, _, _ = tp.instance(fixtures_dir, "smallGrid3D")
    Z = cr.random_rotations_point(R["X"], R["d"], 5)
    A = cr.anchored(cr.hessian(cert.S_matrix(gp.M, Z, R["d"]).toarray(), Z, R["d"]), 0, R["dof"])
    assert np.linalg.eigvalsh(A)[0] < -1e-6 * np.abs(A).max()       # the restated anchored H has a negative eigenvalue there
    Uc = columns(R, 5)
    before = grp.sensitivity(R["X"], Uc, want_adjoint=True)
    Xz = np.asfortranarray(Z)
    m, dof, n = grp.graph.num_edges, R["dof"], R["dof"] * N
    res = dpgo_amd.SensResult()
    sens, adj = np.full((5, m, 2 + dof), 7.0), np.full((n, 5), 7.0, order="F")
    assert raw_call(grp, grp.graph, Xz, Uc, 5, adj, sens, res) == 0
    assert res.outcome == dpgo_amd.SENS_NOT_PD and not sens.any() and not adj.any() and res.stationarity > 1.0
    after = grp.sensitivity(R["X"], Uc, want_adjoint=True)
    assert after[0].outcome == dpgo_amd.SENS_OK and np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])


def test_refusals(fixtures_dir):
    path, N, mm, gp, X0 = tc.problem(fixtures_dir, "smallGrid3D")
    R = tgp.reference(fixtures_dir, "smallGrid3D", 0)
    X, Uc = np.asfortranarray(R["X"]), columns(R, 2)
    G = dpgo_amd.read_g2o(path, 2)
    hub = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(dpgo_amd.LOSS_HUBER, True), X0=X0)
    with pytest.raises(RuntimeError):
        hub.group.sensitivity(X, Uc)                                 # a robust loss
    part = dpgo_amd.NodeGroup(G, [0], dpgo_amd.Options.driver(LOSS_NONE, True))
    with pytest.raises(RuntimeError):
        part.sensitivity(X, Uc)                                      # a group that does not host every node
    grp = tgc.make_group(fixtures_dir, "smallGrid3D", 2)
    for anchor in (N, -1):
        with pytest.raises(RuntimeError):
            grp.sensitivity(X, Uc, anchor=anchor)
    with pytest.raises(RuntimeError):
        grp.sensitivity(X[:-1], Uc)
    # a graph that does not match the group: other poses, another dimension, an edge that is no block of the pattern
    tiny = dpgo_amd.read_g2o(os.path.join(fixtures_dir, "tinyGrid3D.g2o"), 2)
    I, J, Rm, t, kappa, tau = G.edges()
    have = {(int(a), int(b)) for a, b in zip(I, J)} | {(int(b), int(a)) for a, b in zip(I, J)}
    p, q = next((a, b) for a in range(N) for b in range(a + 2, N) if (a, b) not in have)
    stranger = dpgo_amd.graph_from_edges(3, N, np.append(I, p), np.append(J, q), np.concatenate([Rm, Rm[:1]]), np.concatenate([t, t[:1]]),
                                         np.append(kappa, 1.0), np.append(tau, 1.0), 2)
    for bad in (tiny, stranger):
        with pytest.raises(RuntimeError):
            grp.sensitivity(X, Uc, graph=bad)
    # a non-finite upstream entry, anywhere (the anchor's rows included)
    for where, value in (((7, 1), np.nan), ((0, 0), np.inf), ((6 * N - 1, 1), -np.inf)):
        Ub = np.array(Uc, order="F")
        Ub[where] = value
        with pytest.raises(RuntimeError):
            grp.sensitivity(X, Ub)
    with pytest.raises(ValueError):
        grp.sensitivity(X, Uc[:-1])
    # the C ABI: k < 1, ldu < dof N, null upstream / sens / result / graph / group
    m, n = grp.graph.num_edges, 6 * N
    sens, res = np.zeros((2, m, 8)), dpgo_amd.SensResult()
    assert raw_call(grp, grp.graph, X, Uc, 2, None, sens, res) == 0 and res.outcome == dpgo_amd.SENS_OK
    assert raw_call(grp, grp.graph, X, Uc, 0, None, sens, res) == -1 and raw_call(grp, grp.graph, X, Uc, -3, None, sens, res) == -1
    assert raw_call(grp, grp.graph, X, Uc, 2, None, sens, res, ldu=n - 1) == -1
    assert raw_call(grp, grp.graph, X, None, 2, None, sens, res, ldu=n) == -1
    assert raw_call(grp, grp.graph, X, Uc, 2, None, None, res) == -1 and raw_call(grp, grp.graph, X, Uc, 2, None, sens, None) == -1
    assert raw_call(grp, None, X, Uc, 2, None, sens, res) == -1 and raw_call(None, grp.graph, X, Uc, 2, None, sens, res) == -1
    # a wider leading dimension is the same call
    wide = np.zeros((n + 5, 2), order="F")
    wide[:n] = Uc
    s2 = np.zeros_like(sens)
    assert raw_call(grp, grp.graph, X, wide, 2, None, s2, res) == 0 and np.array_equal(s2, sens)
    assert grp.sensitivity(X, Uc)[0].outcome == dpgo_amd.SENS_OK


@pytest.mark.parametrize("name,nn", [("tinyGrid3D", 2), ("smallGrid3D", 5), ("ladder2", 6)])
def test_unit_columns_are_the_columns_of_the_pair_covariance(fixtures_dir, name, nn):
    """lambda of pose p's unit columns is Sigma's columns of p: at the rows of p and q the blocks of pair_covariance (p, q),
    each side within bSigma of the same inverse."""
    grp = tgc.make_group(fixtures_dir, name, nn)
    R = tgp.reference(fixtures_dir, name, 0)
    N, d, dof = R["N"], R["d"], R["dof"]
    for p, q in tgp.non_edge_pairs(R, 0, 41)[:3]:
        res, sens, lam = grp.sensitivity(R["X"], dpgo_amd.unit_upstream(N, d, p), want_adjoint=True)
        joint = grp.pair_covariance(R["X"], [(p, q)])["joint"][0]
        assert res.outcome == dpgo_amd.SENS_OK and res.columns == dof
        rp, rq = slice(dof * p, dof * p + dof), slice(dof * q, dof * q + dof)
        assert np.abs(lam[rp] - joint[0]).max() <= 2 * R["bSigma"]           # S_pp: rows of p, columns of p
        assert np.abs(lam[rq] - joint[1].T).max() <= 2 * R["bSigma"]         # S_pq has the rows of p: its transpose the rows of q
        assert np.abs(joint[0]).max() > 100 * R["bSigma"] and sens.any()


def test_sensitivity_does_not_disturb_the_optimiser(fixtures_dir):
    """30 AMM-PGO# iterations with a call on a sibling trivial-loss group after every fifth: bit for bit the run without."""
    path = tc.problem(fixtures_dir, "smallGrid3D")[0]
    runs = []
    for with_call in (False, True):
        drv = dpgo_amd.DistPGO(dpgo_amd.read_g2o(path, 2), dpgo_amd.Options.driver(LOSS_NONE, True))
        sib = tc.group(path, 2)[0] if with_call else None
        for it in range(30):
            assert drv.step() == 0
            if with_call and it % 5 == 4:
                assert sib.sensitivity(drv.X(), dpgo_amd.unit_upstream(125, 3, 7))[0].outcome in (dpgo_amd.SENS_OK, dpgo_amd.SENS_NOT_PD)
        runs.append((np.array(drv.X()), [drv.group[a].Xk() for a in range(2)]))
    assert np.array_equal(runs[0][0], runs[1][0]) and all(np.array_equal(runs[0][1][a], runs[1][1][a]) for a in range(2))


# ---------------------------------------------------------------------------------------------------------------
# the front ends
# ---------------------------------------------------------------------------------------------------------------
_py = {}


def python_run(fixtures_dir, pose):
    """What the drivers do on tinyGrid3D x 2: 30 iterations, the polish, the unit columns of `pose`."""
    if pose not in _py:
        drv = dpgo_amd.DistPGO(dpgo_amd.read_g2o(os.path.join(fixtures_dir, "tinyGrid3D.g2o"), 2), dpgo_amd.Options.driver(LOSS_NONE, True))
        for _ in range(30):
            assert drv.step() == 0
        Xp, pres, _ = drv.group.polish(drv.X())
        assert pres.outcome == dpgo_amd.POLISH_CONVERGED
        res, sens = drv.group.sensitivity(Xp, dpgo_amd.unit_upstream(drv.graph.num_poses, 3, pose))
        assert res.outcome == dpgo_amd.SENS_OK
        I, J = drv.graph.edges()[:2]
        off = drv.graph.node_offset(1)
        _py[pose] = (res, sens, I, J, (I < off) != (J < off))
    return _py[pose]


def test_dist_pgo_sensitivity_flags(fixtures_dir, tmp_path):
    """--polish --sensitivity_pose P --sensitivity_report FILE adds the report and one line after the summary; the report holds
    NodeGroup.sensitivity's numbers bit for bit."""
    exe = os.path.join(tc.ROOT, "dpgo_amd", "dist_pgo")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    path = os.path.join(fixtures_dir, "tinyGrid3D.g2o")
    base = [exe, "--dataset", path, "--num_nodes", "2", "--iters", "30", "--dist_init", "false", "--save", "false"]
    run = subprocess.run(base + ["--polish", "--sensitivity_pose", "5", "--sensitivity_report", "sens.txt"], capture_output=True, text=True,
                         cwd=tmp_path, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = [l for l in run.stdout.splitlines() if l.startswith("sensitivity: ")]
    assert len(lines) == 1 and run.stdout.rstrip().splitlines()[-1] == lines[0]
    res, sens, I, J, inter = python_run(fixtures_dir, 5)
    f = lines[0].split()
    assert f[1] == "OK" and [int(v) for v in f[2:6]] == [5, res.edges, res.columns, res.batches] and int(f[6]) == res.device_bytes
    rows = np.loadtxt(tmp_path / "sens.txt")
    m = res.edges
    assert rows.shape == (m, 4 + 6 * 8) and np.array_equal(rows[:, 0], np.arange(m))
    assert np.array_equal(rows[:, 1], I) and np.array_equal(rows[:, 2], J) and np.array_equal(rows[:, 3], inter.astype(float))
    assert np.array_equal(rows[:, 4:].reshape(m, 6, 8), np.moveaxis(sens, 0, 1))
    # without --polish, or with a robust loss: the line says why; one flag without the other is an error
    raw = subprocess.run(base + ["--sensitivity_pose", "5", "--sensitivity_report", "s2.txt"], capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert raw.returncode == 0 and "sensitivity: not computed" in raw.stdout and not (tmp_path / "s2.txt").exists()
    hub = subprocess.run(base + ["--loss", "huber", "--polish", "--sensitivity_pose", "5", "--sensitivity_report", "s3.txt"], capture_output=True,
                         text=True, cwd=tmp_path, timeout=300)
    assert hub.returncode == 0 and "sensitivity: not computed" in hub.stdout and not (tmp_path / "s3.txt").exists()
    one = subprocess.run(base + ["--polish", "--sensitivity_pose", "5"], capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert one.returncode != 0
    far = subprocess.run(base + ["--polish", "--sensitivity_pose", "9", "--sensitivity_report", "s4.txt"], capture_output=True, text=True,
                         cwd=tmp_path, timeout=300)
    assert far.returncode != 0


def test_cpp_facade_measurement_sensitivities(fixtures_dir):
    """examples/facade_mm.cpp with `sensitivity P`: DPGOHashGroup::newton_polish and ::measurement_sensitivities after the loop,
    on stderr; stdout the same trace as without; the numbers those of NodeGroup.sensitivity bit for bit; an upstream of the
    wrong length refused."""
    exe = os.path.join(tc.ROOT, "dpgo_amd", "facade_mm")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    args = [exe, os.path.join(fixtures_dir, "tinyGrid3D.g2o"), "2", "30", "trivial", "1"]
    plain = subprocess.run(args, check=True, capture_output=True, text=True, timeout=300)
    out = subprocess.run(args + ["sensitivity", "5"], check=True, capture_output=True, text=True, timeout=300)
    assert out.stdout == plain.stdout and "sensitivity" not in plain.stderr
    lines = [l.split() for l in out.stderr.splitlines() if l.startswith("sensitivity: ")]
    res, sens, _, _, _ = python_run(fixtures_dir, 5)
    m = res.edges
    assert len(lines) == m + 2 and lines[-2][1:] == ["OK", str(m), str(res.columns), str(res.batches)]
    assert [int(l[2]) for l in lines[:m]] == list(range(m))
    got = np.array([[float(v) for v in l[3:]] for l in lines[:m]])
    assert np.array_equal(got.reshape(m, 6, 8), np.moveaxis(sens, 0, 1))
    assert lines[-1][1:] == ["short", "upstream", "-1", "0"]
