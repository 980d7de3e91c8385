"""The Newton polish of the robust objective on the device (Group::robust_polish: polish.cpp's loop with k_robust_edge's F,
k_robust_gather's M_w X and k_robust_mval + k_cov_hessian + k_robust_rank1's H) against its numpy restatement
(tests/robust_restatement.py: polish_full) on the committed trajectory rows (tests/golden/robust_trajectories.json, made on
the CPU by tests/golden/make_robust_trajectories.py; tests/test_robust_host.py checks the file against the restatement).

Only rows whose restated curvature-1 run CONVERGED with at most 12 factorisations are device trajectory cases.  Held exactly:
the outcome, the accepted steps, the factorisations, `indefinite`, the tries of every iteration.  F_k is held within the
tolerance tests/test_gpu_polish.py derives: 1000 times the worst relative difference of F_k between the restatement and the
restatement started from X (1 + 1e-13 xi), xi seeded Gaussians.  The final point is held by the restated gradient and the
smallest eigenvalue of the restated anchored robust Hessian at the restatement's end point; nothing comes from the code under
test.  The facade example and the driver reproduce NodeGroup.robust_polish bit for bit.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import robust_inputs as ri  # noqa: E402
import robust_restatement as rr  # noqa: E402
import test_gpu_polish as tpol  # noqa: E402  (device_free_bytes; none of its tests is imported)

import dpgo_amd  # noqa: E402
from oracle.problem import LOSS_HUBER, LOSS_NONE  # noqa: E402

pytestmark = pytest.mark.gpu

REL_TOL = 1e-9
ROWS = {r["name"]: r for r in ri.trajectories()}
DEVICE_ROWS = [n for n, r in ROWS.items() if r["device"]]
FIELDS = ("outcome", "steps", "factorisations", "indefinite", "F_initial", "F_final", "grad_initial", "grad_final", "hmax", "mu_final",
          "pivot_min", "pivot_max")

_ref, _grp = {}, {}


def objects(row):
    key = (row["input"], row["nodes"])
    if key not in _grp:
        P, _ = ri.trajectory_problem(row)
        G = ri.graph(P)
        _grp[key] = (G, ri.group(G))
    return _grp[key]


def reference(name):
    if name not in _ref:
        row = ROWS[name]
        P, X = ri.trajectory_problem(row)
        loss, dl = row["loss"], row["delta"]
        r = rr.polish_full(P, X, loss, dl, 1)
        xi = np.random.default_rng(41).standard_normal(X.shape)
        rp = rr.polish_full(P, X * (1.0 + 1e-13 * xi), loss, dl, 1)
        k = min(len(r["log"]), len(rp["log"]))
        dF = float(np.max(np.abs(r["log"][:k, 0] - rp["log"][:k, 0]) / np.abs(r["log"][:k, 0])))
        lam_min = float(np.linalg.eigvalsh(rr.hessian(P, r["X"], loss, dl, 1, 0))[0])
        _ref[name] = dict(P=P, X=X, run=r, tolF=1000.0 * dF, lam_min=lam_min,
                          g_ref=float(np.linalg.norm(rr.grad(P, r["X"], loss, dl, 0))))
        print("%s: restatement %d steps, %d factorisations, worst relative difference of F_k under a 1e-13 perturbation %.3g, "
              "lambda_min %.4g" % (name, r["steps"], r["factorisations"], dF, lam_min))
    return _ref[name]


@pytest.mark.parametrize("name", DEVICE_ROWS)
def test_trajectory_and_final_point_against_the_restatement(name):
    row, R = ROWS[name], reference(name)
    P, X, want = R["P"], R["X"], R["run"]
    loss, dl = row["loss"], row["delta"]
    if row["delta_rule"] == "median":   # (computed, not hard-coded: the committed number is this one)
        assert dl == float(np.median(rr.weights(P, X, 0, 1.0)[0][P["inter"]]))
    G, grp = objects(row)
    Xd, res, log, sm = grp.robust_polish(X, loss, dl, curvature=1, graph=G)
    print("%s: %s, %d steps, %d factorisations, %d indefinite, tries %s" %
          (name, dpgo_amd.POLISH_NAMES[res.outcome], res.steps, res.factorisations, res.indefinite, log[:, 4].astype(int).tolist()))
    assert (res.outcome, res.steps, res.factorisations, res.indefinite) == (want["outcome"], want["steps"], want["factorisations"], want["indefinite"])
    assert len(log) == len(want["log"]) and np.array_equal(log[:, 4], want["log"][:, 4])
    c1 = row["curvature1"]   # the committed table says the same
    assert (res.outcome, res.steps, res.factorisations, res.indefinite, log[:, 4].astype(int).tolist()) == \
        (c1["outcome"], c1["steps"], c1["factorisations"], c1["indefinite"], c1["tries"])
    rel = np.abs(log[:, 0] - want["log"][:, 0]) / np.abs(want["log"][:, 0])
    print("    F_k: worst relative difference %.3g, tolerance %.3g" % (rel.max(), R["tolF"]))
    assert np.all(rel <= R["tolF"]), (rel, R["tolF"])
    assert res.F_initial == log[0, 0] and res.F_final == log[-1, 0] and res.grad_initial == log[0, 1] and res.grad_final == log[-1, 1]
    # the final point
    floor = REL_TOL * want["hmax"]
    g_dev = float(np.linalg.norm(rr.grad(P, Xd, loss, dl, 0)))
    dist = float(np.linalg.norm(Xd - want["X"]))
    bound = 2.0 * (g_dev + R["g_ref"]) / R["lam_min"]
    print("    restated |g(X_dev)| %.3g (2 rel_tol hmax = %.3g), |X_dev - X_ref| %.3g (bound %.3g)" % (g_dev, 2 * floor, dist, bound))
    assert R["lam_min"] > 0 and g_dev <= 2.0 * floor and dist <= bound
    F_dev = float(rr.objective(P, Xd, loss, dl))
    assert abs(res.F_final - F_dev) <= 1e-12 * abs(F_dev)
    # the summary describes the final point; the anchor's record is X's bit for bit
    ev = dpgo_amd.EdgeEval(G).run(Xd, loss, dl)[4]
    assert (sm.F, sm.F_intra, sm.F_inter, sm.weight_min, sm.num_inter, sm.num_downweighted) == \
        (ev.F, ev.F_intra, ev.F_inter, ev.weight_min, ev.num_inter, ev.num_downweighted) and sm.F == res.F_final
    d, N = P["d"], P["N"]
    assert np.array_equal(Xd[0], X[0]) and np.array_equal(Xd[N:N + d], X[N:N + d])


def test_the_curvature_of_the_loss_pays(fixtures_dir):
    """On smallGrid3D / Huber 0.25 the re-weighted Hessian needs strictly more steps than the true one, as the restatement
    says it does."""
    row = ROWS["small2_huber"]
    P, X = ri.trajectory_problem(row)
    G, grp = objects(row)
    r1 = grp.robust_polish(X, LOSS_HUBER, row["delta"], curvature=1, graph=G)[1]
    r0 = grp.robust_polish(X, LOSS_HUBER, row["delta"], curvature=0, graph=G)[1]
    print("curvature 1: %d steps, curvature 0: %d steps" % (r1.steps, r0.steps))
    assert r1.outcome == dpgo_amd.POLISH_CONVERGED and r0.steps > r1.steps
    assert (r0.outcome, r0.steps, r0.factorisations) == tuple(row["curvature0"][k] for k in ("outcome", "steps", "factorisations"))


def test_what_it_is_for():
    """verify_reweighted's stationarity -- the robust gradient norm -- is at least 1e3 lower at the polished point."""
    row = ROWS["small2_huber"]
    P, X = ri.trajectory_problem(row)
    G, grp = objects(row)
    Xp, res, _, _ = grp.robust_polish(X, LOSS_HUBER, row["delta"], graph=G)
    before = dpgo_amd.verify_reweighted(G, X, LOSS_HUBER, row["delta"])[0]
    after = dpgo_amd.verify_reweighted(G, Xp, LOSS_HUBER, row["delta"])[0]
    print("stationarity %.3g -> %.3g" % (before.stationarity, after.stationarity))
    assert res.outcome == dpgo_amd.POLISH_CONVERGED and after.stationarity <= 1e-3 * before.stationarity


def test_skipped_allocates_nothing():
    row = ROWS["small2_huber"]
    P, X = ri.trajectory_problem(row)
    G = ri.graph(P)
    grp = ri.group(G)
    grp.robust_polish(X, LOSS_HUBER, 0.25, max_bytes=1, graph=G)   # (the certificate's buffers and M's values come here)
    free0 = tpol.device_free_bytes()
    Xo, res, log, sm = grp.robust_polish(X, LOSS_HUBER, 0.25, max_bytes=1, graph=G)
    assert tpol.device_free_bytes() == free0
    assert res.outcome == dpgo_amd.POLISH_SKIPPED and np.array_equal(Xo, X) and len(log) == 0 and res.steps == 0 and res.factorisations == 0
    plain = grp.polish(X, max_bytes=1)[1]
    assert res.device_bytes > plain.device_bytes > 1          # the per-edge arrays, M_w and the lists are counted in
    assert grp.robust_polish(X, LOSS_HUBER, 0.25, max_bytes=res.device_bytes - 1, graph=G)[1].outcome == dpgo_amd.POLISH_SKIPPED
    ok = grp.robust_polish(X, LOSS_HUBER, 0.25, max_bytes=res.device_bytes, graph=G)[1]
    assert ok.outcome == dpgo_amd.POLISH_CONVERGED and ok.device_bytes == res.device_bytes


def test_refusals():
    row = ROWS["small2_huber"]
    P, X = ri.trajectory_problem(row)
    G = ri.graph(P)
    with pytest.raises(RuntimeError):
        ri.group(G, loss=LOSS_HUBER).robust_polish(X, LOSS_HUBER, 0.25)          # a group created with a robust loss
    part = dpgo_amd.NodeGroup(G, [0], dpgo_amd.Options.driver(LOSS_NONE, True, max_iterations=0))
    with pytest.raises(RuntimeError):
        part.robust_polish(X, LOSS_HUBER, 0.25)                                  # a group that hosts one of two nodes
    grp = ri.group(G)
    foreign = ri.graph(ri.fixture("tinyGrid3D", 2)[0])                           # another pose count
    with pytest.raises(RuntimeError):
        grp.robust_polish(X, LOSS_HUBER, 0.25, graph=foreign)
    Pr, _ = ri.random(3, 160, 125, 2)                                            # the group's poses, edges its pattern does not hold
    with pytest.raises(RuntimeError):
        grp.robust_polish(X, LOSS_HUBER, 0.25, graph=ri.graph(Pr))
    for bad in (dict(loss=4), dict(loss=-1), dict(loss_reg=0.0), dict(loss_reg=float("nan")), dict(loss_reg=float("inf")),
                dict(curvature=2), dict(curvature=-1), dict(anchor=P["N"]), dict(max_tries=0)):
        kw = dict(loss=LOSS_HUBER, loss_reg=0.25)
        kw.update(bad)
        with pytest.raises(RuntimeError):
            grp.robust_polish(X, graph=G, **kw)
    assert grp.robust_polish(X, LOSS_NONE, float("nan"), graph=G)[1].outcome == dpgo_amd.POLISH_CONVERGED   # (loss 0 ignores loss_reg)
    assert grp.robust_polish(X, LOSS_HUBER, 0.25, graph=G)[1].outcome == dpgo_amd.POLISH_CONVERGED


def test_robust_polish_does_not_disturb_the_optimiser(fixtures_dir):
    """20 AMM-PGO# iterations of a trivial-loss driver whose OWN group takes a robust polish (Huber, both curvatures) and a
    robust covariance after every fifth: bit for bit the run without.  (The calls need a trivial-loss group, so the optimiser
    that shares the group runs the trivial loss; the loss of the polish is an argument.)"""
    path = os.path.join(fixtures_dir, "smallGrid3D.g2o")
    runs = []
    for with_polish in (False, True):
        G = dpgo_amd.read_g2o(path, 2)
        drv = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(LOSS_NONE, True))
        trace = []
        for it in range(20):
            assert drv.step() == 0
            if with_polish and it % 5 == 4:
                X = drv.X()
                assert drv.group.robust_polish(X, LOSS_HUBER, 0.25, curvature=it % 2)[1].outcome != dpgo_amd.POLISH_SKIPPED
                assert drv.group.robust_covariance(X, LOSS_HUBER, 0.25)[2].outcome != dpgo_amd.COV_SKIPPED
            trace.append([getattr(drv.group.results(a), f) for a in range(2) for f in ("fobj", "gamma", "gradFnorm", "Gk")])
        runs.append((np.array(drv.X()), [drv.group[a].Xk() for a in range(2)], np.array(trace)))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][2], runs[1][2])
    for a in range(2):
        assert np.array_equal(runs[0][1][a], runs[1][1][a])


def test_several_calls_on_one_group():
    """robust_polish, then polish, then covariance on one group give the bits fresh groups give; a second robust_polish the
    same bits as the first."""
    row = ROWS["small2_huber"]
    P, X = ri.trajectory_problem(row)
    G = ri.graph(P)
    fresh_r = ri.group(G).robust_polish(X, LOSS_HUBER, 0.25, graph=G)
    fresh_p = ri.group(G).polish(X)
    fresh_c = ri.group(G).covariance(fresh_p[0])
    grp = ri.group(G)
    first = grp.robust_polish(X, LOSS_HUBER, 0.25, graph=G)
    pol = grp.polish(X)
    cov = grp.covariance(pol[0])
    second = grp.robust_polish(X, LOSS_HUBER, 0.25, graph=G)
    for a, b in ((first, fresh_r), (second, fresh_r), (pol, fresh_p)):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
        for f in FIELDS:
            assert getattr(a[1], f) == getattr(b[1], f), f
    assert cov[2].outcome == dpgo_amd.COV_OK and np.array_equal(cov[0], fresh_c[0])


# ---------------------------------------------------------------------------------------------------------------
# the facade and the driver
# ---------------------------------------------------------------------------------------------------------------
_py = {}


def python_run(fixtures_dir):
    """What the driver and the facade example do, through Python: chordal point, 20 Huber AMM-PGO# iterations on 2 nodes, the
    robust polish on a trivial-loss group of the same graph."""
    if not _py:
        G = dpgo_amd.read_g2o(os.path.join(fixtures_dir, "smallGrid3D.g2o"), 2)
        opt = dpgo_amd.Options.driver(LOSS_HUBER, True)
        drv = dpgo_amd.DistPGO(G, opt)
        for _ in range(20):
            assert drv.step() == 0
        _py["v"] = ri.group(G).robust_polish(drv.X(), LOSS_HUBER, opt.loss_reg)
        assert _py["v"][1].outcome != dpgo_amd.POLISH_SKIPPED and _py["v"][1].steps >= 1
    return _py["v"]


def check_line(fields, res):
    assert fields[0] == dpgo_amd.POLISH_NAMES[res.outcome]
    assert [int(v) for v in fields[1:4]] == [res.steps, res.factorisations, res.indefinite]
    assert [float(v) for v in fields[4:8]] == [res.F_initial, res.F_final, res.grad_initial, res.grad_final]


def test_cpp_facade_robust_newton_polish(fixtures_dir):
    exe = os.path.join(ri.ROOT, "dpgo_amd", "facade_mm")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    args = [exe, os.path.join(fixtures_dir, "smallGrid3D.g2o"), "2", "20", "huber", "1"]
    plain = subprocess.run(args, check=True, capture_output=True, text=True, timeout=300)
    out = subprocess.run(args + ["robust_polish"], check=True, capture_output=True, text=True, timeout=300)
    assert out.stdout == plain.stdout and "polish" not in plain.stderr
    lines = [l[len("robust polish: "):].split() for l in out.stderr.splitlines() if l.startswith("robust polish: ")]
    Xp, res, _, _ = python_run(fixtures_dir)
    check_line(lines[-1], res)
    assert [int(l[1]) for l in lines[:-1]] == list(range(Xp.shape[0]))
    assert np.array_equal(np.array([[float(v) for v in l[2:]] for l in lines[:-1]]), Xp)


def test_dist_pgo_robust_flags(fixtures_dir, tmp_path):
    """--robust_polish adds one line after the summary and --verify_reweighted behind it acts on the polished point;
    --robust_covariance writes --covariance's format; --loss huber --polish still says why there is no polish; with the
    trivial loss the robust flags say so."""
    exe = os.path.join(ri.ROOT, "dpgo_amd", "dist_pgo")
    base = [exe, "--dataset", os.path.join(fixtures_dir, "smallGrid3D.g2o"), "--num_nodes", "2", "--iters", "20", "--dist_init", "false",
            "--save", "false", "--loss", "huber"]
    cov_file = tmp_path / "rcov.txt"
    plain = subprocess.run(base + ["--verify_reweighted", "--polish"], capture_output=True, text=True, cwd=tmp_path, timeout=300)
    rob = subprocess.run(base + ["--verify_reweighted", "--polish", "--robust_polish", "--robust_covariance", str(cov_file)],
                         capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert plain.returncode == 0 and rob.returncode == 0, rob.stderr[-2000:]
    assert "polish: not computed" in plain.stdout and "robust" not in plain.stdout
    assert "\npolish: not computed" in rob.stdout

    def steady(text):
        return [l for l in text.splitlines() if not l.startswith(("time: ", "robust ", "reweighted verification: "))]

    assert steady(plain.stdout) == steady(rob.stdout)
    line = [l for l in rob.stdout.splitlines() if l.startswith("robust polish: ")]
    Xp, res, _, _ = python_run(fixtures_dir)
    assert len(line) == 1
    check_line(line[0][len("robust polish: "):].split(), res)
    stat = {k: float([l for l in o.stdout.splitlines() if l.startswith("reweighted verification: ")][0].split()[8]) for k, o in
            (("plain", plain), ("rob", rob))}
    assert stat["rob"] <= 1e-3 * stat["plain"]
    cov = [l for l in rob.stdout.splitlines() if l.startswith("robust covariance: ")]
    assert len(cov) == 1 and cov[0].split()[2] == "OK"
    got = np.loadtxt(cov_file)
    G = dpgo_amd.read_g2o(os.path.join(fixtures_dir, "smallGrid3D.g2o"), 2)
    marg = ri.group(G).robust_covariance(Xp, LOSS_HUBER, 0.25)[0]
    iu = np.triu_indices(6)
    assert got.shape == (125, 22) and np.array_equal(got[:, 1:], np.stack([m[iu] for m in marg]))
    triv = subprocess.run(base[:-1] + ["trivial", "--robust_polish", "--robust_covariance", str(tmp_path / "no.txt")],
                          capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert triv.returncode == 0 and "robust polish: not computed" in triv.stdout and "robust covariance: not computed" in triv.stdout
    assert not (tmp_path / "no.txt").exists()
