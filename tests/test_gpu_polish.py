"""The Newton polish on the device (Group::polish: k_polish_grad, k_cov_hessian, k_polish_shift, spd_refactor_device,
spd_vsolve_device, k_polish_retract) against the numpy restatement of its rule (tests/newton_restatement.py) on the small
fixtures and the d = 2 ladder, from chordal and from converged points.

Held exactly to the restatement: the outcome, the accepted steps, the factorisations, `indefinite`, the tries of every
iteration.  F_k is held within a relative tolerance the test computes itself: 1000 times the worst relative difference of
F_k between the restatement and the restatement started from X (1 + 1e-13 xi), xi seeded Gaussians -- how far rounding-size
changes of the input move the trajectory, times a factor for the device's other summation orders over a few hundred terms.
|g| is not compared step by step (its relative difference grows as it falls).  The final point is held by bounds derived from
the restated gradient and the smallest eigenvalue of the restated anchored Hessian; nothing comes from the code under test.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cert_restatement as cert  # noqa: E402
import cov_restatement as cr  # noqa: E402
import newton_restatement as nr  # noqa: E402
import test_gpu_certify as tc  # noqa: E402  (its inputs and caches; none of its tests is imported)
import test_gpu_cert_proof as tp  # noqa: E402  (likewise: the d = 2 graph)
import test_gpu_covariance as tcov  # noqa: E402  (likewise: the converged points)

import dpgo_amd  # noqa: E402
from oracle.problem import LOSS_NONE  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ROOT = tc.ROOT
REL_TOL = 1e-9
CASES = [("tinyGrid3D", 1, "chordal"), ("tinyGrid3D", 2, "chordal"), ("tinyGrid3D", 1, "converged"), ("tinyGrid3D", 2, "converged"),
         ("smallGrid3D", 1, "chordal"), ("smallGrid3D", 5, "chordal"), ("smallGrid3D", 1, "converged"),
         ("smallGrid3D", 5, "converged"), ("ladder2", 6, "converged")]

_ref = {}


def start(fixtures_dir, name, which):
    return tp.instance(fixtures_dir, name)[3] if which == "chordal" else tcov.converged(fixtures_dir, name)


def reference(fixtures_dir, name, which):
    """Once per (input, start): the restatement's run, the tolerance of F_k, and at its final point the smallest eigenvalue of
    the restated anchored Hessian and the restated gradient's norm."""
    key = (name, which)
    if key not in _ref:
        N, mm, gp, _, _ = tp.instance(fixtures_dir, name)
        d = mm.d
        X = np.array(start(fixtures_dir, name, which))
        r = nr.polish_full(gp.M, X, d, anchor=0)
        xi = np.random.default_rng(41).standard_normal(X.shape)
        rp = nr.polish_full(gp.M, X * (1.0 + 1e-13 * xi), d, anchor=0)
        k = min(len(r["log"]), len(rp["log"]))
        dF = float(np.max(np.abs(r["log"][:k, 0] - rp["log"][:k, 0]) / np.abs(r["log"][:k, 0])))
        lam_min = float(np.linalg.eigvalsh(nr.anchored_hessian(gp.M, r["X"], d, 0))[0])
        _ref[key] = dict(N=N, d=d, M=gp.M, X=X, run=r, tolF=1000.0 * dF, lam_min=lam_min,
                         g_ref=float(np.linalg.norm(nr.grad(gp.M, r["X"], d, 0))))
        print("%s %s: restatement %d steps, %d factorisations, worst relative difference of F_k under a 1e-13 perturbation %.3g, "
              "lambda_min %.4g, hmax %.5g" % (name, which, r["steps"], r["factorisations"], dF, lam_min, r["hmax"]))
    return _ref[key]


def make_group(fixtures_dir, name, nn):
    return tp.instance(fixtures_dir, name)[4](nn)[0]


_runs = {}


def device_run(fixtures_dir, name, nn, which):
    key = (name, nn, which)
    if key not in _runs:
        R = reference(fixtures_dir, name, which)
        _runs[key] = make_group(fixtures_dir, name, nn).polish(R["X"])
    return _runs[key]


def orthogonality(X, d):
    N = X.shape[0] // (d + 1)
    Y = X[N:].reshape(N, d, d)
    return float(np.abs(Y @ np.transpose(Y, (0, 2, 1)) - np.eye(d)).max())


@pytest.mark.parametrize("name,nn,which", CASES)
def test_trajectory_against_the_restatement(fixtures_dir, name, nn, which):
    R = reference(fixtures_dir, name, which)
    want = R["run"]
    Xd, res, log = device_run(fixtures_dir, name, nn, which)
    print("%s x %d %s: %s, %d steps, %d factorisations, %d indefinite, tries %s" %
          (name, nn, which, dpgo_amd.POLISH_NAMES[res.outcome], res.steps, res.factorisations, res.indefinite, log[:, 4].astype(int).tolist()))
    assert (res.outcome, res.steps, res.factorisations, res.indefinite) == (want["outcome"], want["steps"], want["factorisations"], want["indefinite"])
    assert len(log) == len(want["log"]) and np.array_equal(log[:, 4], want["log"][:, 4])
    rel = np.abs(log[:, 0] - want["log"][:, 0]) / np.abs(want["log"][:, 0])
    print("    F_k: worst relative difference %.3g, tolerance %.3g" % (rel.max(), R["tolF"]))
    assert np.all(rel <= R["tolF"]), (rel, R["tolF"])
    assert res.F_initial == log[0, 0] and res.F_final == log[-1, 0] and res.grad_initial == log[0, 1] and res.grad_final == log[-1, 1]
    assert res.unknowns == cr.dof_of(R["d"]) * R["N"] and res.fronts >= 1 and res.device_bytes > 0 and res.total_ms > 0


@pytest.mark.parametrize("name,nn,which", CASES)
def test_final_point(fixtures_dir, name, nn, which):
    R = reference(fixtures_dir, name, which)
    d, N, M, want = R["d"], R["N"], R["M"], R["run"]
    Xd, res, log = device_run(fixtures_dir, name, nn, which)
    floor = REL_TOL * want["hmax"]
    g_dev = float(np.linalg.norm(nr.grad(M, Xd, d, 0)))
    dist = float(np.linalg.norm(Xd - want["X"]))
    bound = 2.0 * (g_dev + R["g_ref"]) / R["lam_min"]
    print("%s x %d %s: restated |g(X_dev)| %.3g (2 rel_tol hmax = %.3g), |X_dev - X_ref| %.3g (bound %.3g)" %
          (name, nn, which, g_dev, 2 * floor, dist, bound))
    assert g_dev <= 2.0 * floor
    assert dist <= bound
    assert abs(res.F_final - nr.objective(M, Xd)) <= 1e-12 * abs(res.F_final)
    assert abs(res.grad_final - g_dev) <= 1e-12 * g_dev + 1e-3 * floor
    # (mu_final is not held bit for bit: the rule's floor is a tie by construction -- 1e-3 hmax divided by ten five times IS
    # 1e-8 hmax -- so the last mu is 0 or 1e-8 hmax as rounding has it)
    assert abs(res.hmax - want["hmax"]) <= 1e-9 * want["hmax"]
    assert abs(res.mu_final - want["mu_final"]) <= 1e-8 * want["hmax"] * (1 + 1e-9)
    # the anchor's record bit for bit, the rotations orthogonal
    X = R["X"]
    assert np.array_equal(Xd[0], X[0]) and np.array_equal(Xd[N:N + d], X[N:N + d])
    assert orthogonality(Xd, d) <= 64 * U


@pytest.mark.parametrize("name,which", sorted({(c[0], c[2]) for c in CASES if c[0] != "ladder2"}))
def test_every_partition_ends_at_the_same_point(fixtures_dir, name, which):
    R = reference(fixtures_dir, name, which)
    ends = [device_run(fixtures_dir, c[0], c[1], c[2])[0] for c in CASES if (c[0], c[2]) == (name, which)]
    assert len(ends) == 2
    g = [float(np.linalg.norm(nr.grad(R["M"], Z, R["d"], 0))) for Z in ends]
    assert float(np.linalg.norm(ends[0] - ends[1])) <= 2.0 * (g[0] + g[1]) / R["lam_min"]


def test_convexity_report_and_max_steps(fixtures_dir):
    """From the chordal point of tinyGrid3D the first factorisation meets a non-positive pivot.  From the point with random
    rotations the run has many near-threshold not-positive-definite decisions and is not compared step by step."""
    assert device_run(fixtures_dir, "tinyGrid3D", 2, "chordal")[1].indefinite == 1
    N, mm, gp, X0, make = tp.instance(fixtures_dir, "tinyGrid3D")
    Z = cr.random_rotations_point(X0, mm.d, 5)
    Xd, res, log = make(2)[0].polish(Z)
    print("random rotations: %s, %d steps, %d factorisations, %d indefinite, F %.6g -> %.6g, |g| %.3g -> %.3g" %
          (dpgo_amd.POLISH_NAMES[res.outcome], res.steps, res.factorisations, res.indefinite, res.F_initial, res.F_final,
           res.grad_initial, res.grad_final))
    assert res.outcome in (dpgo_amd.POLISH_MAX_STEPS, dpgo_amd.POLISH_CONVERGED)
    assert np.all(np.diff(log[:, 0]) <= 0)
    assert abs(res.F_final - nr.objective(gp.M, Xd)) <= 1e-12 * abs(res.F_final)
    assert res.F_final < 0.1 * res.F_initial
    assert res.indefinite >= 1 and res.factorisations > res.steps


def test_what_it_is_for(fixtures_dir):
    """The certificate and the covariance at a critical point: verify is PROVEN on smallGrid3D with a stationarity at least
    1e3 below the unpolished point's; tinyGrid3D is a local minimum -- covariance OK, certify NEGATIVE -- and polishing does
    not change that."""
    X = tcov.converged(fixtures_dir, "smallGrid3D")
    grp = make_group(fixtures_dir, "smallGrid3D", 2)
    before = grp.verify(X)[0]
    Xp, res, _ = grp.polish(X)
    after = grp.verify(Xp)[0]
    print("smallGrid3D: stationarity %.3g -> %.3g" % (before.stationarity, after.stationarity))
    assert res.outcome == dpgo_amd.POLISH_CONVERGED and after.status == dpgo_amd.CERT_PROVEN
    assert after.stationarity <= 1e-3 * before.stationarity
    X = tcov.converged(fixtures_dir, "tinyGrid3D")
    grp = make_group(fixtures_dir, "tinyGrid3D", 2)
    before = grp.certify(X)[0]
    Xp, res, _ = grp.polish(X)
    cov = grp.covariance(Xp)[2]
    after = grp.certify(Xp)[0]
    print("tinyGrid3D: stationarity %.3g -> %.3g" % (before.stationarity, after.stationarity))
    assert res.outcome == dpgo_amd.POLISH_CONVERGED and cov.outcome == dpgo_amd.COV_OK
    assert before.status == dpgo_amd.CERT_NEGATIVE and after.status == dpgo_amd.CERT_NEGATIVE
    assert after.stationarity <= 1e-3 * before.stationarity and cov.stationarity == after.stationarity


def device_free_bytes():
    """hipMemGetInfo of the HIP runtime the library itself is linked against (resolved through the library's handle), behind a
    device synchronise."""
    import ctypes as C
    L = dpgo_amd.lib()
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert L.hipDeviceSynchronize() == 0 and L.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_skipped_allocates_nothing(fixtures_dir):
    X = tcov.converged(fixtures_dir, "smallGrid3D")
    grp = make_group(fixtures_dir, "smallGrid3D", 2)
    grp.polish(X, max_bytes=1)          # (the certificate's buffers and M's values come here)
    free0 = device_free_bytes()
    Xo, res, log = grp.polish(X, max_bytes=1)
    assert device_free_bytes() == free0
    assert res.outcome == dpgo_amd.POLISH_SKIPPED and np.array_equal(Xo, X) and len(log) == 0
    assert res.unknowns == 6 * (X.shape[0] // 4) and res.fronts >= 4 and res.levels >= 3 and res.max_front > 0 and res.device_bytes > 1
    assert res.steps == 0 and res.factorisations == 0
    assert grp.polish(X, max_bytes=res.device_bytes - 1)[1].outcome == dpgo_amd.POLISH_SKIPPED
    ok = grp.polish(X, max_bytes=res.device_bytes)[1]
    assert ok.outcome == dpgo_amd.POLISH_CONVERGED and ok.device_bytes == res.device_bytes and ok.symbolic_s == 0.0
    # what polish counts is less than what covariance counts: it may run where covariance is SKIPPED
    cov = grp.covariance(X, max_bytes=res.device_bytes)[2]
    assert cov.device_bytes > res.device_bytes and cov.outcome == dpgo_amd.COV_SKIPPED


def test_refusals(fixtures_dir):
    path, N, mm, gp, X0 = tc.problem(fixtures_dir, "smallGrid3D")
    X = tcov.converged(fixtures_dir, "smallGrid3D")
    G = dpgo_amd.read_g2o(path, 2)
    hub = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(dpgo_amd.LOSS_HUBER, True), X0=X0)
    with pytest.raises(RuntimeError):
        hub.group.polish(X)                      # a robust loss
    part = dpgo_amd.NodeGroup(G, [0], dpgo_amd.Options.driver(LOSS_NONE, True))
    with pytest.raises(RuntimeError):
        part.polish(X)                           # a group that hosts one of two nodes
    grp = make_group(fixtures_dir, "smallGrid3D", 2)
    for bad in (dict(anchor=N), dict(anchor=-1), dict(max_steps=-1), dict(max_tries=0), dict(rel_tol=-1.0)):
        with pytest.raises(RuntimeError):
            grp.polish(X, **bad)
    with pytest.raises(RuntimeError):
        grp.polish(X[:-1])
    assert grp.polish(X)[1].outcome == dpgo_amd.POLISH_CONVERGED


def test_polish_does_not_disturb_the_optimiser(fixtures_dir):
    """30 AMM-PGO# iterations with a polish on a sibling trivial-loss group after every fifth: bit for bit the run without."""
    path = tc.problem(fixtures_dir, "smallGrid3D")[0]
    runs = []
    for with_polish in (False, True):
        drv = dpgo_amd.DistPGO(dpgo_amd.read_g2o(path, 2), dpgo_amd.Options.driver(LOSS_NONE, True))
        sib = tc.group(path, 2)[0] if with_polish else None
        trace = []
        for it in range(30):
            assert drv.step() == 0
            if with_polish and it % 5 == 4:
                assert sib.polish(drv.X())[1].outcome == dpgo_amd.POLISH_CONVERGED
            trace.append([getattr(drv.group.results(a), f) for a in range(2) for f in ("fobj", "gamma", "gradFnorm", "Gk")])
        runs.append((np.array(drv.X()), [drv.group[a].Xk() for a in range(2)], np.array(trace)))
    assert np.array_equal(runs[0][0], runs[1][0])
    for a in range(2):
        assert np.array_equal(runs[0][1][a], runs[1][1][a])
    assert np.array_equal(runs[0][2], runs[1][2])


def test_several_calls_on_one_group(fixtures_dir):
    """A covariance call behind a polish gives the bits it gives on a fresh group; a second polish from the same X gives the
    same bits; a polish from another anchor ends at a critical point too."""
    X = tcov.converged(fixtures_dir, "smallGrid3D")
    fresh = make_group(fixtures_dir, "smallGrid3D", 2).covariance(X)
    grp = make_group(fixtures_dir, "smallGrid3D", 2)
    first = grp.polish(X)
    cov = grp.covariance(X)
    assert cov[2].outcome == dpgo_amd.COV_OK and np.array_equal(cov[0], fresh[0])
    second = grp.polish(X)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[2], second[2])
    for f in ("outcome", "steps", "factorisations", "indefinite", "F_initial", "F_final", "grad_initial", "grad_final", "hmax",
              "mu_final", "pivot_min", "pivot_max"):
        assert getattr(first[1], f) == getattr(second[1], f), f
    other = grp.polish(X, anchor=7)
    N = X.shape[0] // 4
    assert other[1].outcome == dpgo_amd.POLISH_CONVERGED
    assert np.array_equal(other[0][7], X[7]) and np.array_equal(other[0][N + 21:N + 24], X[N + 21:N + 24])


# ---------------------------------------------------------------------------------------------------------------
# the facade and the driver
# ---------------------------------------------------------------------------------------------------------------
_py = {}
FIELDS = ("steps", "factorisations", "indefinite", "F_initial", "F_final", "grad_initial", "grad_final")


def python_run(fixtures_dir):
    """What the driver and the facade example do, through Python: chordal point, 20 AMM-PGO# iterations on 2 nodes, the polish
    call on the group that iterated."""
    if not _py:
        path = tc.problem(fixtures_dir, "smallGrid3D")[0]
        drv = dpgo_amd.DistPGO(dpgo_amd.read_g2o(path, 2), dpgo_amd.Options.driver(LOSS_NONE, True))
        for _ in range(20):
            assert drv.step() == 0
        _py["v"] = drv.group.polish(drv.X())
        assert _py["v"][1].outcome == dpgo_amd.POLISH_CONVERGED and _py["v"][1].steps >= 2
    return _py["v"]


def check_line(fields, res):
    assert fields[1] == "CONVERGED"
    assert [int(v) for v in fields[2:5]] == [res.steps, res.factorisations, res.indefinite]
    assert [float(v) for v in fields[5:9]] == [res.F_initial, res.F_final, res.grad_initial, res.grad_final]


def test_cpp_facade_newton_polish(fixtures_dir):
    """examples/facade_mm.cpp with `polish`: DPGOHashGroup::newton_polish after the loop, on stderr; stdout the same trace as
    without; the point and the counts those of NodeGroup.polish bit for bit."""
    exe = os.path.join(ROOT, "dpgo_amd", "facade_mm")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    args = [exe, os.path.join(fixtures_dir, "smallGrid3D.g2o"), "2", "20", "trivial", "1"]
    plain = subprocess.run(args, check=True, capture_output=True, text=True, timeout=300)
    out = subprocess.run(args + ["polish"], check=True, capture_output=True, text=True, timeout=300)
    assert out.stdout == plain.stdout and "polish" not in plain.stderr
    lines = [l.split() for l in out.stderr.splitlines() if l.startswith("polish: ")]
    Xp, res, _ = python_run(fixtures_dir)
    check_line(lines[-1], res)
    assert [int(l[2]) for l in lines[:-1]] == list(range(Xp.shape[0]))
    assert np.array_equal(np.array([[float(v) for v in l[3:]] for l in lines[:-1]]), Xp)


def test_dist_pgo_polish_flag(fixtures_dir, tmp_path):
    """--polish adds one line after the summary and puts the polished point into the result files; without it stdout and the
    files are what they were.  --verify behind it acts on the polished point."""
    exe = os.path.join(ROOT, "dpgo_amd", "dist_pgo")
    base = [exe, "--dataset", os.path.join(fixtures_dir, "smallGrid3D.g2o"), "--num_nodes", "2", "--iters", "20", "--dist_init", "false"]
    outs = {}
    for tag, extra in (("plain", ["--verify"]), ("polish", ["--polish", "--verify"])):
        cwd = tmp_path / tag
        cwd.mkdir()
        outs[tag] = (subprocess.run(base + extra, capture_output=True, text=True, cwd=cwd, timeout=300), cwd)
        assert outs[tag][0].returncode == 0, outs[tag][0].stderr[-2000:]

    def steady(text):   # (the summary's wall time differs from run to run)
        return [l for l in text.splitlines() if not l.startswith(("time: ", "polish: ", "verification: "))]

    assert steady(outs["plain"][0].stdout) == steady(outs["polish"][0].stdout)
    assert "polish" not in outs["plain"][0].stdout
    assert sorted(os.listdir(outs["plain"][1])) == sorted(os.listdir(outs["polish"][1]))
    tail = outs["polish"][0].stdout.rstrip().splitlines()[-2:]
    assert tail[0].startswith("polish: ") and tail[1].startswith("verification: ")
    Xp, res, _ = python_run(fixtures_dir)
    check_line(tail[0].split(), res)
    # the certificate's stationarity is that of the polished point
    stat = {tag: float(outs[tag][0].stdout.rstrip().splitlines()[-1].split()[-1]) for tag in outs}
    assert stat["polish"] <= 1e-3 * stat["plain"]
    # estimates_trivial.txt (six digits, gauge-fixed: t - t_0, X R_0) holds the polished point
    N, d = Xp.shape[0] // 4, 3
    want = Xp.copy()
    want[:N] -= Xp[0]
    want = want @ Xp[N:N + d].T
    got = np.loadtxt(outs["polish"][1] / "estimates_trivial.txt")
    old = np.loadtxt(outs["plain"][1] / "estimates_trivial.txt")
    assert np.max(np.abs(got - want)) <= 1e-5 * np.max(np.abs(want))
    assert np.max(np.abs(old - want)) > 1e-4 * np.max(np.abs(want))   # (20 iterations are visibly short of the critical point)
    assert open(outs["plain"][1] / "results_chordal_2_amm.txt").read().split()[2::4] == \
        open(outs["polish"][1] / "results_chordal_2_amm.txt").read().split()[2::4]
    # a robust loss: the line says why there is no polish
    hub = subprocess.run(base[:-4] + ["--iters", "5", "--dist_init", "false", "--loss", "huber", "--polish", "--save", "false"],
                         capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert hub.returncode == 0 and "polish: not computed" in hub.stdout
