"""NodeGroup.robust_sensitivity / dpgo_group_robust_sensitivity on the device (dpgo_amd/csrc/rsens.h): the outcomes SKIPPED and
NOT_PD, every refusal, the trivial loss against NodeGroup.sensitivity, the optimiser left alone, and the front ends (dist_pgo
--robust_polish --sensitivity_pose, the C++ facade).  The arithmetic is held to the restatement in tests/test_gpu_rsens_ops.py.

The trivial loss "equals sensitivity in value" as far as two factorisations of two roundings of one matrix can: the robust call
writes H from M_w = sum_e 1 M_e (k_robust_mval), sensitivity from the assembled M, and the two differ in the order of their sums
(tests/test_gpu_robust_ops.py holds them to 2 bH of each other).  So each side is held to the long-double restatement at the
long-double adjoint within its own margin (margin_rsens, margin_sens, lambda to bSigma |c|_1 with the bound of H in bSigma), and
the two to each other within the sum.  The indefinite point is tests/test_gpu_robust_covariance.py's: random_graph(2, 160, N=40)
at its own X under Geman-McClure with delta = 1.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_restatement as cr  # noqa: E402
import factor_restatement as fr  # noqa: E402
import robust_inputs as ri  # noqa: E402
import robust_restatement as rr  # noqa: E402
import rsens_restatement as rs  # noqa: E402
import sens_restatement as sn  # noqa: E402
import solve_restatement as sr  # noqa: E402
import test_gpu_pairs as tgp  # noqa: E402  (device_free_bytes; none of its tests is imported)
import test_gpu_robust_polish as trp  # noqa: E402  (the drivers' run through Python; none of its tests is imported)

import dpgo_amd  # noqa: E402
from oracle.problem import LOSS_GM, LOSS_HUBER, LOSS_NONE  # noqa: E402

pytestmark = pytest.mark.gpu

LD, U = rs.LD, rs.U
ROWS = {r["name"]: r for r in ri.trajectories()}
_pt = {}


def small():
    """(P, graph, group, the robust-polished point) of smallGrid3D on 2 nodes under Huber 0.25."""
    if not _pt:
        row = ROWS["small2_huber"]
        P, X = ri.trajectory_problem(row)
        G = ri.graph(P)
        grp = ri.group(G)
        Xp, res, _, _ = grp.robust_polish(X, LOSS_HUBER, 0.25, graph=G)
        assert res.outcome == dpgo_amd.POLISH_CONVERGED
        _pt["v"] = (P, G, grp, np.asfortranarray(Xp))
    return _pt["v"]


def columns(P, k, seed=3):
    return np.asfortranarray(np.random.default_rng(seed).standard_normal((cr.dof_of(P["d"]) * P["N"], k)))


def raw_call(grp, graph, X, Uc, k, adjoint, sens, dreg, res, loss=LOSS_HUBER, loss_reg=0.25, anchor=0, max_bytes=0, ldu=None):
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    return dpgo_amd.lib().dpgo_group_robust_sensitivity(grp._h if grp else None, graph._h if graph else None, dp(X), X.shape[0], loss,
                                                        loss_reg, anchor, max_bytes, dp(Uc), Uc.shape[0] if ldu is None else ldu, k,
                                                        dp(adjoint), dp(sens), dp(dreg), C.byref(res) if res is not None else None)


def test_skipped_leaves_the_outputs_alone_and_allocates_nothing():
    row = ROWS["small2_huber"]
    P, X = ri.trajectory_problem(row)
    X = np.asfortranarray(X)
    G = ri.graph(P)
    grp = ri.group(G)                                       # a fresh group: nothing of the robust objective is on the device
    Uc = columns(P, 3)
    m, dof = len(P["I"]), 6
    n = dof * P["N"]
    res = dpgo_amd.SensResult()
    sens, dreg, adj = np.full((3, m, 3 + dof), 7.0), np.full(3, 7.0), np.full((n, 3), 7.0, order="F")
    assert raw_call(grp, G, X, Uc, 3, adj, sens, dreg, res, max_bytes=1) == 0   # (the certificate's buffers and M's values come here)
    free0 = tgp.device_free_bytes()
    assert raw_call(grp, G, X, Uc, 3, adj, sens, dreg, res, max_bytes=1) == 0
    assert tgp.device_free_bytes() == free0
    assert res.outcome == dpgo_amd.SENS_SKIPPED and np.all(sens == 7.0) and np.all(adj == 7.0) and np.all(dreg == 7.0)
    assert res.unknowns == n and res.fronts >= 4 and res.levels >= 1 and res.max_front > 0 and res.device_bytes > 1
    assert (res.columns, res.batches, res.edges) == (3, 1, m)
    # the robust buffers are counted in: more than the plain call on the same sizes predicts
    plain = grp.sensitivity(X, Uc, max_bytes=1)[0]
    assert res.device_bytes > plain.device_bytes
    # the prediction is the threshold: one byte less is refused, the prediction itself runs -- and predicts the same once the
    # robust buffers are on the device
    assert grp.robust_sensitivity(X, Uc, LOSS_HUBER, 0.25, max_bytes=res.device_bytes - 1, graph=G)[0].outcome == dpgo_amd.SENS_SKIPPED
    ok, s, dr = grp.robust_sensitivity(X, Uc, LOSS_HUBER, 0.25, max_bytes=res.device_bytes, graph=G)
    assert ok.outcome in (dpgo_amd.SENS_OK, dpgo_amd.SENS_NOT_PD) and ok.device_bytes == res.device_bytes
    again = grp.robust_sensitivity(X, Uc, LOSS_HUBER, 0.25, max_bytes=res.device_bytes - 1, graph=G)[0]
    assert again.outcome == dpgo_amd.SENS_SKIPPED and again.device_bytes == res.device_bytes
    # the call's own buffers are counted: more columns, more edges' worth of output
    more = grp.robust_sensitivity(X, columns(P, 64), LOSS_HUBER, 0.25, max_bytes=1, graph=G)[0]
    assert more.device_bytes >= res.device_bytes + 8 * (64 - 16) * n + 8 * (64 - 3) * (n + m * (3 + dof))
    assert grp.robust_sensitivity(X, columns(P, 200), LOSS_HUBER, 0.25, max_bytes=1, graph=G)[0].device_bytes == more.device_bytes


def test_not_positive_definite_where_the_curvature_of_the_loss_wins():
    P, X = ri.named("rand2_160")
    lam1 = np.linalg.eigvalsh(rr.hessian(P, X, LOSS_GM, 1.0, 1, 0))
    assert lam1[0] < -1e-6 * lam1[-1]                       # the restated anchored H has a negative eigenvalue there
    G = ri.graph(P)
    grp = ri.group(G)
    Uc = columns(P, 5)
    m, n = len(P["I"]), 3 * P["N"]
    res = dpgo_amd.SensResult()
    sens, dreg, adj = np.full((5, m, 6), 7.0), np.full(5, 7.0), np.full((n, 5), 7.0, order="F")
    assert raw_call(grp, G, np.asfortranarray(X), Uc, 5, adj, sens, dreg, res, loss=LOSS_GM, loss_reg=1.0) == 0
    assert res.outcome == dpgo_amd.SENS_NOT_PD and not sens.any() and not adj.any() and not dreg.any() and res.stationarity > 1.0
    # the same point without the loss: a verdict of its own, and the group goes on
    assert grp.robust_sensitivity(X, Uc, LOSS_NONE, graph=G)[0].outcome in (dpgo_amd.SENS_OK, dpgo_amd.SENS_NOT_PD)


def test_refusals(fixtures_dir):
    P, G, grp, X = small()
    N = P["N"]
    Uc = columns(P, 2)
    with pytest.raises(RuntimeError):
        ri.group(G, loss=LOSS_HUBER).robust_sensitivity(X, Uc, LOSS_HUBER, 0.25)    # a group created with a robust loss
    part = dpgo_amd.NodeGroup(G, [0], dpgo_amd.Options.driver(LOSS_NONE, True, max_iterations=0))
    with pytest.raises(RuntimeError):
        part.robust_sensitivity(X, Uc, LOSS_HUBER, 0.25)                            # a group that hosts one of two nodes
    for bad in (dict(loss=4), dict(loss=-1), dict(loss_reg=0.0), dict(loss_reg=-1.0), dict(loss_reg=float("nan")),
                dict(loss_reg=float("inf")), dict(anchor=N), dict(anchor=-1)):
        kw = dict(loss=LOSS_HUBER, loss_reg=0.25)
        kw.update(bad)
        with pytest.raises(RuntimeError):
            grp.robust_sensitivity(X, Uc, graph=G, **kw)
    with pytest.raises(RuntimeError):
        grp.robust_sensitivity(X[:-1], Uc, LOSS_HUBER, 0.25, graph=G)
    # a graph that does not match the group: other poses, edges its pattern does not hold
    foreign = ri.graph(ri.fixture("tinyGrid3D", 2)[0])
    Pr, _ = ri.random(3, 160, 125, 2)
    for bad in (foreign, ri.graph(Pr)):
        with pytest.raises(RuntimeError):
            grp.robust_sensitivity(X, Uc, LOSS_HUBER, 0.25, graph=bad)
    # a non-finite upstream entry, anywhere (the anchor's rows included)
    for where, value in (((7, 1), np.nan), ((0, 0), np.inf), ((6 * N - 1, 1), -np.inf)):
        Ub = np.array(Uc, order="F")
        Ub[where] = value
        with pytest.raises(RuntimeError):
            grp.robust_sensitivity(X, Ub, LOSS_HUBER, 0.25, graph=G)
    with pytest.raises(ValueError):
        grp.robust_sensitivity(X, Uc[:-1], LOSS_HUBER, 0.25, graph=G)
    # the C ABI: k < 1, ldu < dof N, null upstream / sens / dloss_reg / result / graph / group
    m, n = len(P["I"]), 6 * N
    sens, dreg, res = np.zeros((2, m, 9)), np.zeros(2), dpgo_amd.SensResult()
    assert raw_call(grp, G, X, Uc, 2, None, sens, dreg, res) == 0 and res.outcome == dpgo_amd.SENS_OK
    assert raw_call(grp, G, X, Uc, 0, None, sens, dreg, res) == -1 and raw_call(grp, G, X, Uc, -3, None, sens, dreg, res) == -1
    assert raw_call(grp, G, X, Uc, 2, None, sens, dreg, res, ldu=n - 1) == -1
    assert raw_call(grp, G, X, None, 2, None, sens, dreg, res, ldu=n) == -1
    assert raw_call(grp, G, X, Uc, 2, None, None, dreg, res) == -1 and raw_call(grp, G, X, Uc, 2, None, sens, None, res) == -1
    assert raw_call(grp, G, X, Uc, 2, None, sens, dreg, None) == -1
    assert raw_call(grp, None, X, Uc, 2, None, sens, dreg, res) == -1 and raw_call(None, G, X, Uc, 2, None, sens, dreg, res) == -1
    # a wider leading dimension is the same call
    wide = np.zeros((n + 5, 2), order="F")
    wide[:n] = Uc
    s2, d2 = np.zeros_like(sens), np.zeros_like(dreg)
    assert raw_call(grp, G, X, wide, 2, None, s2, d2, res) == 0 and np.array_equal(s2, sens) and np.array_equal(d2, dreg)
    assert sens.any() and dreg.all()


@pytest.mark.parametrize("name", ["tiny", "rand2_70", "rand3_70"])
def test_the_trivial_loss_equals_sensitivity_in_value(name):
    P, X0 = ri.named(name)
    G = ri.graph(P)
    grp = ri.group(G)
    X, pres, _ = grp.polish(X0, max_steps=60)
    assert pres.outcome == dpgo_amd.POLISH_CONVERGED
    X = np.asfortranarray(X)
    dof, N = cr.dof_of(P["d"]), P["N"]
    R = rr.reference(P, X, LOSS_NONE, 1.0, 1, 0)
    ev = np.linalg.eigvalsh(np.asarray(R["H"], np.float64))
    assert ev[0] > 0
    bSigma = cr.C * U * float(ev[-1] / ev[0]) / float(ev[0]) + float(np.linalg.norm(R["bH"], 2)) / float(ev[0]) ** 2
    Cc = columns(P, 17)
    Cz = np.array(Cc)
    Cz[:dof] = 0.0
    lam = sr.solve_cholesky_ld(R["H"], Cz)
    b_lam = bSigma * np.abs(Cz).sum(axis=0)
    res, sens, dreg, adj = grp.robust_sensitivity(X, Cc, LOSS_NONE, graph=G, want_adjoint=True)
    res0, plain, adj0 = grp.sensitivity(X, Cc, graph=G, want_adjoint=True)
    assert res.outcome == dpgo_amd.SENS_OK and res0.outcome == dpgo_amd.SENS_OK and not sens[..., -1].any() and not dreg.any()
    want = np.moveaxis(sn.sens_edge(P, X, lam, LD), 1, 0)
    m_r = np.moveaxis(rs.margin_rsens(P, X, np.asarray(lam, np.float64), LOSS_NONE, 1.0, b_lam), 1, 0)[..., :-1]
    m_p = np.moveaxis(sn.margin_sens(P, X, np.asarray(lam, np.float64), b_lam), 1, 0)
    worst = (float(np.max(np.abs(np.asarray(sens[..., :-1], LD) - want) / m_r)), float(np.max(np.abs(np.asarray(plain, LD) - want) / m_p)),
             float(np.max(np.abs(sens[..., :-1] - plain) / (m_r + m_p))), float(np.max(np.abs(adj - adj0) / (2 * b_lam[None, :]))))
    print("%s, trivial loss: robust_sensitivity %.3g, sensitivity %.3g of their margins; their difference %.3g, the adjoints' %.3g of the sums"
          % ((name,) + worst))
    assert max(worst) < 1.0
    # tighter, with nothing of bSigma in it: every edge against sens_math.h on the host at each call's own adjoint -- two fp64
    # evaluations of one formula (under the trivial loss rsens_combine returns sens_one's numbers), each within margin_sens (b = 0)
    for col in (0, 8, 16):
        for got, lam_dev in ((sens[col][:, :-1], adj[:, col]), (plain[col], adj0[:, col])):
            host = dpgo_amd.sens_edge_debug(G, X, np.ascontiguousarray(lam_dev))[0]
            assert np.all(np.abs(got - host) <= 2 * sn.margin_sens(P, X, lam_dev))
    # the margins are no blanket, loose as bSigma's model of the factorisation makes them: the typical entry is well above them
    assert np.median(np.abs(plain) / (m_r + m_p)) > 10


def test_robust_sensitivity_does_not_disturb_the_optimiser(fixtures_dir):
    """20 AMM-PGO# iterations of a trivial-loss driver whose OWN group takes a robust sensitivity call (Huber) after every fifth:
    bit for bit the run without."""
    path = os.path.join(fixtures_dir, "smallGrid3D.g2o")
    runs = []
    for with_call in (False, True):
        G = dpgo_amd.read_g2o(path, 2)
        drv = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(LOSS_NONE, True))
        trace = []
        for it in range(20):
            assert drv.step() == 0
            if with_call and it % 5 == 4:
                out = drv.group.robust_sensitivity(drv.X(), dpgo_amd.unit_upstream(125, 3, 7), LOSS_HUBER, 0.25)
                assert out[0].outcome in (dpgo_amd.SENS_OK, dpgo_amd.SENS_NOT_PD)
            trace.append([getattr(drv.group.results(a), f) for a in range(2) for f in ("fobj", "gamma", "gradFnorm", "Gk")])
        runs.append((np.array(drv.X()), [drv.group[a].Xk() for a in range(2)], np.array(trace)))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][2], runs[1][2])
    for a in range(2):
        assert np.array_equal(runs[0][1][a], runs[1][1][a])


# ---------------------------------------------------------------------------------------------------------------
# the front ends
# ---------------------------------------------------------------------------------------------------------------
_py = {}


def python_run(fixtures_dir, pose):
    """What the drivers do on smallGrid3D x 2 under Huber: 20 iterations, the robust polish on a trivial-loss group, the unit
    columns of `pose` through robust_sensitivity on that group at that point."""
    if pose not in _py:
        Xp = trp.python_run(fixtures_dir)[0]
        G = dpgo_amd.read_g2o(os.path.join(fixtures_dir, "smallGrid3D.g2o"), 2)
        opt = dpgo_amd.Options.driver(LOSS_HUBER, True)
        res, sens, dreg = ri.group(G).robust_sensitivity(Xp, dpgo_amd.unit_upstream(G.num_poses, 3, pose), LOSS_HUBER, opt.loss_reg)
        assert res.outcome == dpgo_amd.SENS_OK
        I, J = G.edges()[:2]
        off = G.node_offset(1)
        _py[pose] = (res, sens, dreg, I, J, (I < off) != (J < off))
    return _py[pose]


def test_dist_pgo_robust_sensitivity_flags(fixtures_dir, tmp_path):
    """--loss huber --robust_polish --sensitivity_pose P --sensitivity_report FILE: one line after the summary, the report with
    one more value per row and the delta line, NodeGroup.robust_sensitivity's numbers bit for bit.  Without --robust_polish the
    line still says why there are no sensitivities, as it did."""
    exe = os.path.join(ri.ROOT, "dpgo_amd", "dist_pgo")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    base = [exe, "--dataset", os.path.join(fixtures_dir, "smallGrid3D.g2o"), "--num_nodes", "2", "--iters", "20", "--dist_init", "false",
            "--save", "false", "--loss", "huber"]
    run = subprocess.run(base + ["--robust_polish", "--sensitivity_pose", "5", "--sensitivity_report", "rsens.txt"], capture_output=True,
                         text=True, cwd=tmp_path, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = [l for l in run.stdout.splitlines() if l.startswith("robust sensitivity: ")]
    assert len(lines) == 1 and run.stdout.rstrip().splitlines()[-1] == lines[0] and "\nsensitivity: " not in run.stdout
    res, sens, dreg, I, J, inter = python_run(fixtures_dir, 5)
    f = lines[0][len("robust sensitivity: "):].split()
    assert f[0] == "OK" and [int(v) for v in f[1:5]] == [5, res.edges, res.columns, res.batches] and int(f[5]) == res.device_bytes
    text = (tmp_path / "rsens.txt").read_text().splitlines()
    m = res.edges
    assert len(text) == m + 1 and text[-1].split()[0] == "delta"
    assert np.array_equal(np.array([float(v) for v in text[-1].split()[1:]]), dreg)
    rows = np.array([[float(v) for v in l.split()] for l in text[:-1]])
    assert rows.shape == (m, 4 + 6 * 9) and np.array_equal(rows[:, 0], np.arange(m))
    assert np.array_equal(rows[:, 1], I) and np.array_equal(rows[:, 2], J) and np.array_equal(rows[:, 3], inter.astype(float))
    assert np.array_equal(rows[:, 4:].reshape(m, 6, 9), np.moveaxis(sens, 0, 1))
    assert dreg.all() and sens[:, inter, -1].any()
    # without --robust_polish: the line of before; one flag without the other is an error
    hub = subprocess.run(base + ["--polish", "--sensitivity_pose", "5", "--sensitivity_report", "s3.txt"], capture_output=True, text=True,
                         cwd=tmp_path, timeout=300)
    assert hub.returncode == 0 and "sensitivity: not computed (the Hessian is that of the trivial loss; --loss huber)" in hub.stdout
    assert "robust sensitivity" not in hub.stdout and not (tmp_path / "s3.txt").exists()
    one = subprocess.run(base + ["--robust_polish", "--sensitivity_pose", "5"], capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert one.returncode != 0


def test_cpp_facade_robust_measurement_sensitivities(fixtures_dir):
    """examples/facade_mm.cpp with `robust_sensitivity P`: DPGOHashGroup::robust_newton_polish and
    ::robust_measurement_sensitivities after the loop, on stderr; stdout the same trace as without; the numbers those of
    NodeGroup.robust_sensitivity bit for bit."""
    exe = os.path.join(ri.ROOT, "dpgo_amd", "facade_mm")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    args = [exe, os.path.join(fixtures_dir, "smallGrid3D.g2o"), "2", "20", "huber", "1"]
    plain = subprocess.run(args, check=True, capture_output=True, text=True, timeout=300)
    out = subprocess.run(args + ["robust_sensitivity", "5"], check=True, capture_output=True, text=True, timeout=300)
    assert out.stdout == plain.stdout and "sensitivity" not in plain.stderr
    lines = [l[len("robust sensitivity: "):].split() for l in out.stderr.splitlines() if l.startswith("robust sensitivity: ")]
    res, sens, dreg, _, _, _ = python_run(fixtures_dir, 5)
    m = res.edges
    assert len(lines) == m + 2 and lines[-1] == ["OK", str(m), str(res.columns), str(res.batches)]
    assert [int(l[1]) for l in lines[:m]] == list(range(m)) and lines[m][0] == "delta"
    got = np.array([[float(v) for v in l[2:]] for l in lines[:m]])
    assert np.array_equal(got.reshape(m, 6, 9), np.moveaxis(sens, 0, 1))
    assert np.array_equal(np.array([float(v) for v in lines[m][1:]]), dreg)
