"""The maximum-likelihood refinement on the device (Group::ml_polish: polish_loop under the hooks of ml.cpp) against the numpy
restatement of its rule (tests/ml_restatement.py: polish_full), from the isotropic model's polished point, on tinyGrid3D x
{1, 2} nodes, smallGrid3D x {1, 2, 5}, the d = 2 ladder x 6 and the d = 2 grid x {1, 3} (tests/test_ml_host.py: WHOLE, whose decisions were shown on
the CPU to sit at least 4 rounding bounds from their alternatives).

Held exactly to the restatement: the outcome, the accepted steps, the factorisations, the tries of every iteration.  F_k is
held within a relative tolerance the test computes itself, as tests/test_gpu_polish.py does: 1000 times the worst relative
difference of F_k between the restatement and the restatement started from X (1 + 1e-13 xi).  The final point is held by the
bound from the restated gradient and the smallest eigenvalue of the restated anchored Hessian -- where the refinement converges:
the ladder's cannot (its measurements are random, F_ml jumps where an angle residual wraps), so its six replayed steps end at
MAX_STEPS and have no final-point bound; the d = 2 grid is the converging d = 2 input.  Nothing comes from the device.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ml_restatement as mr  # noqa: E402
import newton_restatement as nr  # noqa: E402
import test_gpu_ml_ops as ops  # noqa: E402  (its groups; none of its tests is imported)
import test_gpu_polish as tgp  # noqa: E402  (device_free_bytes; none of its tests is imported)
import test_ml_host as tmh  # noqa: E402  (the whole-call inputs and their trajectories; none of its tests is imported)

import dpgo_amd  # noqa: E402
from oracle.problem import LOSS_NONE  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [("tinyGrid3D", 1), ("tinyGrid3D", 2), ("smallGrid3D", 1), ("smallGrid3D", 2), ("smallGrid3D", 5), ("ladder2", 6),
         ("grid2", 1), ("grid2", 3)]
_ref, _runs = {}, {}


def reference(fixtures_dir, name):
    if name not in _ref:
        E, X = tmh.iso_point(fixtures_dir, name)
        r = tmh.trajectory(fixtures_dir, name)
        ms = tmh.WHOLE[name][1]
        xi = np.random.default_rng(41).standard_normal(X.shape)
        rp = mr.polish_full(E, X * (1.0 + 1e-13 * xi), anchor=0, max_steps=ms)
        k = min(len(r["log"]), len(rp["log"]))
        dF = float(np.max(np.abs(r["log"][:k, 0] - rp["log"][:k, 0]) / np.abs(r["log"][:k, 0])))
        F, g, H = mr.assemble(E, r["X"], 0)
        _ref[name] = dict(E=E, X=X, run=r, tolF=1000.0 * dF, max_steps=ms, lam_min=float(np.linalg.eigvalsh(0.5 * (H + H.T))[0]),
                          g_ref=float(np.linalg.norm(g)))
        print("%s: restatement %d steps, %d factorisations, F_k moves %.3g under a 1e-13 perturbation, lambda_min %.4g" %
              (name, r["steps"], r["factorisations"], dF, _ref[name]["lam_min"]))
    return _ref[name]


def device_run(fixtures_dir, name, nn):
    if (name, nn) not in _runs:
        R = reference(fixtures_dir, name)
        grp = ops.group_of(R["E"], nn)
        _runs[(name, nn)] = (grp,) + grp.ml_polish(R["X"], max_steps=R["max_steps"])
    return _runs[(name, nn)]


@pytest.mark.parametrize("name,nn", CASES)
def test_trajectory_against_the_restatement(fixtures_dir, name, nn):
    R = reference(fixtures_dir, name)
    want = R["run"]
    grp, Xd, res, log = device_run(fixtures_dir, name, nn)
    print("%s x %d: %s, %d steps, %d factorisations, F_ml %.9g -> %.9g, tries %s" %
          (name, nn, dpgo_amd.POLISH_NAMES[res.outcome], res.steps, res.factorisations, res.F_initial, res.F_final,
           log[:, 4].astype(int).tolist()))
    assert (res.outcome, res.steps, res.factorisations, res.indefinite) == (want["outcome"], want["steps"], want["factorisations"], 0)
    assert len(log) == len(want["log"]) and np.array_equal(log[:, 4], want["log"][:, 4])
    rel = np.abs(log[:, 0] - want["log"][:, 0]) / np.abs(want["log"][:, 0])
    print("    F_k: worst relative difference %.3g, tolerance %.3g" % (rel.max(), R["tolF"]))
    assert np.all(rel <= R["tolF"]), (rel, R["tolF"])
    assert res.F_initial == log[0, 0] and res.F_final == log[-1, 0] and res.F_final <= res.F_initial
    assert res.chi2_initial == 2 * res.F_initial and res.chi2_final == 2 * res.F_final and res.near_pi == 0
    # ml_eval's chi2 sums to 2 F_ml, and F_ml is the log's
    F, r, chi2, near = grp.ml_eval(Xd)
    assert abs(chi2.sum() - 2 * F) <= 1e-13 * abs(2 * F) and abs(F - res.F_final) <= 1e-13 * abs(F) and near == 0
    assert abs(F - float(mr.objective(R["E"], Xd))) <= 1e-12 * abs(F)


@pytest.mark.parametrize("name,nn", [c for c in CASES if c[0] != "ladder2"])
def test_final_point(fixtures_dir, name, nn):
    R = reference(fixtures_dir, name)
    E, want = R["E"], R["run"]
    d, N = E["d"], E["N"]
    grp, Xd, res, log = device_run(fixtures_dir, name, nn)
    floor = 1e-9 * want["hmax"]
    g_dev = float(np.linalg.norm(mr.assemble(E, Xd, 0)[1]))
    dist = float(np.linalg.norm(Xd - want["X"]))
    bound = 2.0 * (g_dev + R["g_ref"]) / R["lam_min"]
    print("%s x %d: restated |g(X_dev)| %.3g (2 rel_tol hmax = %.3g), |X_dev - X_ref| %.3g (bound %.3g)" %
          (name, nn, g_dev, 2 * floor, dist, bound))
    assert g_dev <= 2.0 * floor and dist <= bound
    assert abs(res.hmax - want["hmax"]) <= 1e-9 * want["hmax"]
    X = R["X"]
    assert np.array_equal(Xd[0], X[0]) and np.array_equal(Xd[N:N + d], X[N:N + d])   # the anchor's record bit for bit
    assert tgp.orthogonality(Xd, d) <= 64 * tgp.U


def test_skipped_allocates_nothing(fixtures_dir):
    R = reference(fixtures_dir, "smallGrid3D")
    grp = ops.group_of(R["E"], 2)
    grp.ml_polish(R["X"], max_bytes=1)          # (the certificate's buffers come here)
    free0 = tgp.device_free_bytes()
    Xo, res, log = grp.ml_polish(R["X"], max_bytes=1)
    assert tgp.device_free_bytes() == free0
    assert res.outcome == dpgo_amd.POLISH_SKIPPED and np.array_equal(Xo, R["X"]) and len(log) == 0
    assert res.unknowns == 6 * R["E"]["N"] and res.fronts >= 4 and res.max_front > 0 and res.device_bytes > 1
    plain = grp.polish(R["X"], max_bytes=1)[1]
    assert res.device_bytes > plain.device_bytes          # the arrays of the edge pass are counted in
    assert grp.ml_polish(R["X"], max_bytes=res.device_bytes - 1)[1].outcome == dpgo_amd.POLISH_SKIPPED
    ok = grp.ml_polish(R["X"], max_bytes=res.device_bytes)[1]
    assert ok.outcome == dpgo_amd.POLISH_CONVERGED and ok.device_bytes == res.device_bytes
    cov = grp.ml_covariance(R["X"], max_bytes=1)[2]
    assert cov.outcome == dpgo_amd.COV_SKIPPED and cov.device_bytes > 1


def test_ml_calls_do_not_disturb_the_optimiser(fixtures_dir):
    """20 AMM-PGO# iterations with the four calls on the iterating group after every fifth: bit for bit the run without."""
    R = reference(fixtures_dir, "smallGrid3D")
    runs = []
    for with_ml in (False, True):
        G = tmh.graph_of(R["E"], 2)
        drv = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(LOSS_NONE, True))
        trace = []
        for it in range(20):
            assert drv.step() == 0
            if with_ml and it % 5 == 4:
                Z = drv.X()
                assert drv.group.ml_polish(Z, max_steps=3)[1].steps >= 1
                assert drv.group.ml_covariance(Z)[2].outcome == dpgo_amd.COV_OK
                drv.group.ml_hessian(Z)
                drv.group.ml_eval(Z)
            trace.append([getattr(drv.group.results(a), f) for a in range(2) for f in ("fobj", "gamma", "gradFnorm", "Gk")])
        runs.append((np.array(drv.X()), np.array(trace)))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


def test_several_calls_on_one_group(fixtures_dir):
    """A second refinement from the same X gives the same bits; the isotropic polish and covariance behind it give the bits
    they give on a fresh group (the factor is shared, the certificate's M is never written)."""
    R = reference(fixtures_dir, "smallGrid3D")
    fresh = ops.group_of(R["E"], 2)
    p0, c0 = fresh.polish(R["X"]), fresh.covariance(R["X"])
    grp, Xd, res, log = device_run(fixtures_dir, "smallGrid3D", 2)
    second = grp.ml_polish(R["X"], max_steps=R["max_steps"])
    assert np.array_equal(second[0], Xd) and np.array_equal(second[2], log)
    p1, c1 = grp.polish(R["X"]), grp.covariance(R["X"])
    assert np.array_equal(p0[0], p1[0]) and np.array_equal(c0[0], c1[0])


# ---------------------------------------------------------------------------------------------------------------
# the facade and the driver
# ---------------------------------------------------------------------------------------------------------------
_py = {}


def python_run(fixtures_dir):
    """What the driver and the facade example do, through Python: chordal point, 20 AMM-PGO# iterations on 2 nodes, the polish
    and from its point the refinement on the file's own information matrices, on the group that iterated."""
    if not _py:
        path = os.path.join(fixtures_dir, "smallGrid3D.g2o")
        drv = dpgo_amd.DistPGO(dpgo_amd.read_g2o(path, 2), dpgo_amd.Options.driver(LOSS_NONE, True))
        for _ in range(20):
            assert drv.step() == 0
        Xp = drv.group.polish(drv.X())[0]
        Xm, res, log = drv.group.ml_polish(Xp)
        assert res.outcome == dpgo_amd.POLISH_CONVERGED
        _py["v"] = (Xm, res, drv.group.ml_eval(Xm), drv.group.ml_covariance(Xm))
        assert _py["v"][3][2].outcome == dpgo_amd.COV_OK
    return _py["v"]


def check_line(fields, res):
    assert fields[2] == "CONVERGED"
    assert [int(v) for v in fields[3:6]] == [res.steps, res.factorisations, res.indefinite]
    assert [float(v) for v in fields[6:10]] == [res.F_initial, res.F_final, res.grad_initial, res.grad_final]


def test_cpp_facade_ml_polish(fixtures_dir):
    """examples/facade_mm.cpp with `ml_polish`: DPGOHashGroup::newton_polish, then DPGOHashGroup::ml_polish, on stderr; stdout
    the same trace as without; the point and the counts those of NodeGroup.ml_polish bit for bit."""
    import subprocess
    exe = os.path.join(tgp.ROOT, "dpgo_amd", "facade_mm")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    args = [exe, os.path.join(fixtures_dir, "smallGrid3D.g2o"), "2", "20", "trivial", "1"]
    plain = subprocess.run(args, check=True, capture_output=True, text=True, timeout=300)
    out = subprocess.run(args + ["ml_polish"], check=True, capture_output=True, text=True, timeout=300)
    assert out.stdout == plain.stdout and "ml polish" not in plain.stderr
    lines = [l.split() for l in out.stderr.splitlines() if l.startswith("ml polish: ")]
    Xm, res, _, _ = python_run(fixtures_dir)
    check_line(lines[-1], res)
    assert [int(l[3]) for l in lines[:-1]] == list(range(Xm.shape[0]))
    assert np.array_equal(np.array([[float(v) for v in l[4:]] for l in lines[:-1]]), Xm)
    # DPGOHashGroup::ml_marginal_covariances at that point: the upper triangles of NodeGroup.ml_covariance bit for bit
    cl = [l.split() for l in out.stderr.splitlines() if l.startswith("ml covariance: ")]
    marg, cres = python_run(fixtures_dir)[3][0], python_run(fixtures_dir)[3][2]
    assert cl[-1][2] == "OK" and [int(v) for v in cl[-1][3:5]] == [cres.fronts, cres.levels]
    iu = np.triu_indices(6)
    assert [int(l[2]) for l in cl[:-1]] == list(range(len(marg)))
    assert np.array_equal(np.array([[float(v) for v in l[3:]] for l in cl[:-1]]), np.array([m[iu] for m in marg]))


def test_dist_pgo_ml_flags(fixtures_dir, tmp_path):
    """--ml_polish behind --polish adds one line and puts the refined point into the result files; --ml_report and
    --ml_covariance act on it; all three agree bit for bit with the Python calls.  Without them stdout is what it was."""
    import subprocess
    exe = os.path.join(tgp.ROOT, "dpgo_amd", "dist_pgo")
    base = [exe, "--dataset", os.path.join(fixtures_dir, "smallGrid3D.g2o"), "--num_nodes", "2", "--iters", "20", "--dist_init", "false",
            "--polish"]
    plain = subprocess.run(base, capture_output=True, text=True, cwd=tmp_path, timeout=300)
    ml = subprocess.run(base + ["--ml_polish", "--ml_report", "chi2.txt", "--ml_covariance", "mlcov.txt"], capture_output=True, text=True,
                        cwd=tmp_path, timeout=300)
    assert plain.returncode == 0 and ml.returncode == 0, ml.stderr[-2000:]
    steady = lambda text: [l for l in text.splitlines() if not l.startswith(("time: ", "ml polish: ", "ml covariance: "))]
    assert steady(plain.stdout) == steady(ml.stdout) and "ml " not in plain.stdout
    Xm, res, ev, cov = python_run(fixtures_dir)
    line = [l for l in ml.stdout.splitlines() if l.startswith("ml polish: ")][0].split()
    check_line(line, res)
    assert [float(v) for v in line[10:12]] == [res.chi2_initial, res.chi2_final] and int(line[12]) == res.near_pi
    rep = open(tmp_path / "chi2.txt").read().splitlines()
    head = rep[0].split()
    assert head[:2] == ["#", "F_ml"] and float(head[2]) == ev[0] and float(head[4]) == 2 * ev[0] and int(head[6]) == len(ev[2])
    assert np.array_equal(np.array([float(l.split()[2]) for l in rep[1:]]), ev[2])
    I, J = dpgo_amd.read_g2o(os.path.join(fixtures_dir, "smallGrid3D.g2o"), 2).edges()[:2]
    assert [[int(v) for v in l.split()[:2]] for l in rep[1:]] == np.stack([I, J], axis=1).tolist()
    got = np.loadtxt(tmp_path / "mlcov.txt")
    iu = np.triu_indices(6)
    assert np.array_equal(got[:, 0], np.arange(len(got))) and np.array_equal(got[:, 1:], np.array([m[iu] for m in cov[0]]))
    assert [l for l in ml.stdout.splitlines() if l.startswith("ml covariance: ")][0].split()[2] == "OK"
