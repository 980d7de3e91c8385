"""Hessian modes on the device (dpgo_amd/csrc/modes.h): NodeGroup.hessian_modes against numpy.linalg.eigvalsh of the restated
anchored Hessian (tests/cov_restatement.py) with the anchor's rows struck out, on the inputs of tests/test_modes_host.py --
tinyGrid3D x {1, 2} nodes, smallGrid3D x {1, 2, 5}, the twisted rings x {1, 3}, the d = 2 ladder x 6 and the indefinite
tinyGrid3D point x {1, 2} -- with k in {1, 4, 8}.

Bounds (u = 2^-53); nothing in them comes from the device.
  values      |values[j] - lambda_j| <= residuals[j] + C n u hmax, index by index (a missed mode fails this): the matrix is
              symmetric, so a Ritz value lies within its residual of an eigenvalue; C = 1 was fixed on the CPU
              (tests/test_modes_host.py: 4 x the largest gap between the fp64 and the long-double restatement)
  residuals   the true |H v_j - lambda_j v_j|, in long double with the restated H, is at most residuals[j] plus the same allowance
  vectors     |V V' - I| <= 8 (n + b^2) u: the entries of the two Gram matrices carry the rounding of sums of n products, and
              C'GC = I holds to b^2 u kappa with kappa, the condition of the scaled G, near 1 once the block has settled on the
              eigenvectors; rows sum: |sum_p energy[j][p] - 1| <= 2 (n + 8) u (n squares of a vector normalised in fp64)
  escape      F_escape <= F - 0.1 pred(alpha), both F re-evaluated by the restatement, within what two fp64 evaluations of F may
              differ by (tests/test_gpu_staircase.py: value_bound)
  E-optimum   1 / lambda_0 is the largest eigenvalue of the covariance and dominates its diagonal; the device's marginals carry
              cov_restatement's C u kappa_2 / lambda_0, the device's lambda_0 its residual and allowance
The facade example and the driver are held bit for bit to the Python call on the group that iterated.
The iteration count is compared with the restatement's where the CPU check (modes_restatement.decisive) shows every decisive
residual a factor 4 from rel_tol hmax on either side of the stopping iteration; the other inputs are left out of THAT assertion.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_restatement as cr  # noqa: E402
import modes_restatement as mr  # noqa: E402
import newton_restatement as nr  # noqa: E402
import test_gpu_certify as tc  # noqa: E402  (its inputs; none of its tests is imported)
import test_gpu_cert_proof as tp  # noqa: E402  (likewise: the groups)
import test_gpu_polish as tpol  # noqa: E402  (likewise: device_free_bytes)
import test_gpu_staircase as tgs  # noqa: E402  (likewise: the rings' groups, value_bound)
import test_modes_host as tmh  # noqa: E402  (likewise: the points, the dense references, the restatement's runs, C)

import dpgo_amd  # noqa: E402
from oracle.problem import LOSS_NONE  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ROOT = tc.ROOT
KS = tmh.KS
CASES = [("tinyGrid3D", 1), ("tinyGrid3D", 2), ("smallGrid3D", 1), ("smallGrid3D", 2), ("smallGrid3D", 5), ("ring2", 1), ("ring2", 3),
         ("ring3", 1), ("ring3", 3), ("ladder2", 6), ("tinyGrid3D-indefinite", 1), ("tinyGrid3D-indefinite", 2)]


def make_group(fixtures_dir, name, nn):
    if name.startswith("ring"):
        return tgs.ring_group(int(name[-1]), nn)
    return tp.instance(fixtures_dir, name.split("-")[0])[4](nn)[0]


_runs = {}


def device_run(fixtures_dir, name, nn, k):
    key = (name, nn, k)
    if key not in _runs:
        grp = _runs.setdefault(("group", name, nn), make_group(fixtures_dir, name, nn))
        _runs[key] = grp.hessian_modes(tmh.point(fixtures_dir, name)[1], k)
    return _runs[key]


def show(tag, out):
    r = out["result"]
    print("%s: %s, %d iterations, %d factorisations (%d shifted), mu %.4g, block %d, negative %d, lambda %.6g ... %.6g, worst "
          "residual %.3g; %d unknowns, %d fronts, %d bytes; factor %.2f solve %.2f gram %.2f ritz %.2f update %.2f total %.2f ms" %
          (tag, dpgo_amd.MODES_NAMES[r.outcome], r.iterations, r.factorisations, r.shift_tries, r.mu, r.block, r.negative,
           out["values"][0], out["values"][-1], out["residuals"].max(), r.unknowns, r.fronts, r.device_bytes, r.factor_ms, r.solve_ms,
           r.gram_ms, r.ritz_ms, r.update_ms, r.total_ms))


@pytest.mark.parametrize("name,nn", CASES)
def test_modes_against_the_dense_spectrum(fixtures_dir, name, nn):
    D = tmh.dense(fixtures_dir, name)
    n, dof, hmax, lam = D["n"], D["dof"], D["hmax"], D["lam"]
    N = n // dof
    allow = tmh.allowance(D)
    for k in KS:
        out = device_run(fixtures_dir, name, nn, k)
        r = out["result"]
        show("%s x %d, k = %d" % (name, nn, k), out)
        assert r.outcome == dpgo_amd.MODES_CONVERGED
        assert r.unknowns == n and r.block == 16 and r.fronts >= 1 and r.device_bytes > 0 and r.iterations >= 1
        assert abs(r.hmax - hmax) <= 1e-9 * hmax
        vals, res, V = out["values"], out["residuals"], out["vectors"]
        assert np.all(res <= 1e-8 * r.hmax)
        err = np.abs(vals - lam[:k])
        true = mr.true_residuals(D["A"], vals, V)
        print("    worst |value - eigenvalue| / (residual + allowance) %.3g, worst (true residual - residual) / allowance %.3g, "
              "|VV' - I| %.3g of its bound" % (float((err / (res + allow)).max()), float(((true - res) / allow).max()),
                                              np.abs(V @ V.T - np.eye(k)).max() / (8 * (n + 256) * U)))
        assert np.all(err <= res + allow)
        assert np.all(true <= res + allow)
        assert np.abs(V @ V.T - np.eye(k)).max() <= 8 * (n + 16 * 16) * U
        assert not V[:, :dof].any()                                  # the anchor's rows: exact zeros
        E = out["energy"]
        assert E.shape == (k, N) and np.all(E >= 0) and np.abs(E.sum(axis=1) - 1.0).max() <= 2 * (n + 8) * U
        assert np.abs(E - (V.reshape(k, N, dof) ** 2).sum(axis=2)).max() <= 4 * dof * U
        assert r.negative == int(np.sum(lam[:k] < 0))
        ref = tmh.restated(fixtures_dir, name, k)
        if name.endswith("indefinite"):
            assert r.shift_tries >= 1 and r.negative >= 1 and r.mu > 0
            assert r.shift_tries == ref["shift_tries"] and r.factorisations == ref["factorisations"]
            assert abs(r.mu - ref["mu"]) <= 1e-9 * ref["mu"]
        else:
            assert r.shift_tries == 0 and r.negative == 0 and r.mu == 0.0 and r.factorisations == 1
        if mr.decisive(ref["history"], k, 1e-8 * hmax):
            print("    iterations compared with the restatement's: %d" % ref["iterations"])
            assert r.iterations == ref["iterations"]
        # every partition: another ordering, other fronts, the same pairs
        first = _runs.setdefault(("first", name, k), out)
        assert np.all(np.abs(vals - first["values"]) <= res + first["residuals"] + 2 * allow)
        # ... and the same bits on a second call
        again = _runs[("group", name, nn)].hessian_modes(D["X"], k)
        assert np.array_equal(again["values"], vals) and np.array_equal(again["vectors"], V) and np.array_equal(again["residuals"], res)
        assert again["result"].iterations == r.iterations and again["X_escape"] is None


def test_another_anchor(fixtures_dir):
    name = "tinyGrid3D"
    N = tmh.dense(fixtures_dir, name)["n"] // 6
    D = tmh.dense(fixtures_dir, name, anchor=N - 1)
    out = make_group(fixtures_dir, name, 2).hessian_modes(D["X"], 4, anchor=N - 1)
    assert out["result"].outcome == dpgo_amd.MODES_CONVERGED
    assert np.all(np.abs(out["values"] - D["lam"][:4]) <= out["residuals"] + tmh.allowance(D))
    assert not out["vectors"][:, 6 * (N - 1):].any() and not out["energy"][:, N - 1].any()
    assert np.all(mr.true_residuals(D["A"], out["values"], out["vectors"]) <= out["residuals"] + tmh.allowance(D))


@pytest.mark.parametrize("nn", [1, 2])
def test_escape_from_the_indefinite_point(fixtures_dir, nn):
    name = "tinyGrid3D-indefinite"
    D = tmh.dense(fixtures_dir, name)
    M, X, d = D["M"], D["X"], D["d"]
    grp = make_group(fixtures_dir, name, nn)
    out = grp.hessian_modes(X, 1, want_escape=1)
    r = out["result"]
    assert r.outcome == dpgo_amd.MODES_CONVERGED and r.negative == 1 and r.escaped == 1 and r.escape_alpha > 0
    v0, lam0, alpha = out["vectors"][0], out["values"][0], r.escape_alpha
    g = nr.grad(M, X, d, 0)
    gv = float(g @ v0)
    pred = alpha * abs(gv) + 0.5 * alpha * alpha * abs(lam0)
    F0, F1 = nr.objective(M, X), nr.objective(M, out["X_escape"])
    floor = tgs.value_bound(M, X) + tgs.value_bound(M, out["X_escape"])
    print("x %d: lambda_0 %.6g, g'v_0 %.4g, alpha %.4g (alpha_0 %.4g), F %.8g -> %.8g, predicted decrease %.4g, floor %.3g" %
          (nn, lam0, gv, alpha, 0.5 / np.abs(v0).max(), F0, F1, pred, floor))
    assert F1 <= F0 - 0.1 * pred + floor
    assert abs(r.F - F0) <= floor and abs(r.F_escape - F1) <= floor
    # the point is the retraction along s v_0, alpha one of the 31 halvings of 0.5 / |v_0|_inf
    s = -1.0 if gv > 0 else 1.0
    want = nr.retract(X, alpha * s * v0, d, 0)
    assert np.abs(out["X_escape"] - want).max() <= 1e-12 * max(1.0, np.abs(X).max())
    ratio = (0.5 / np.abs(v0).max()) / alpha
    assert abs(ratio - 2.0 ** round(np.log2(ratio))) <= 1e-9 * ratio and 0 <= round(np.log2(ratio)) <= 30
    # at a minimum there is nothing to escape: X itself
    Dp = tmh.dense(fixtures_dir, "tinyGrid3D")
    op = grp.hessian_modes(Dp["X"], 1, want_escape=1)
    assert op["result"].escaped == 0 and op["result"].negative == 0 and np.array_equal(op["X_escape"], np.asfortranarray(Dp["X"]))
    assert op["result"].F_escape == op["result"].F


@pytest.mark.parametrize("name,nn", [("tinyGrid3D", 2), ("smallGrid3D", 5), ("ladder2", 6)])
def test_e_optimality_dominates_the_marginals(fixtures_dir, name, nn):
    D = tmh.dense(fixtures_dir, name)
    out = device_run(fixtures_dir, name, nn, 1)
    marg, _, cres = _runs[("group", name, nn)].covariance(D["X"])
    assert cres.outcome == dpgo_amd.COV_OK and out["result"].negative == 0
    top = max(float(np.diag(m).max()) for m in marg)
    lam = D["lam"]
    slack = cr.C * U * float(lam[-1] / lam[0]) / float(lam[0])
    lo = out["values"][0] - out["residuals"][0] - tmh.allowance(D)
    print("%s x %d: 1 / lambda_0 = %.6g, largest marginal variance %.6g" % (name, nn, 1.0 / out["values"][0], top))
    assert lo > 0 and 1.0 / lo >= top - slack
    assert 1.0 / out["values"][0] >= top          # (and plainly: the gap is not at rounding level on these graphs)


@pytest.mark.parametrize("k,block", [(13, 32), (29, 48), (45, 64)])
def test_wider_blocks(fixtures_dir, k, block):
    """The three wider blocks through the whole call (the restatement converges in 21, 35 and 52 iterations)."""
    D = tmh.dense(fixtures_dir, "smallGrid3D")
    grp = _runs.setdefault(("group", "smallGrid3D", 2), make_group(fixtures_dir, "smallGrid3D", 2))
    out = grp.hessian_modes(D["X"], k)
    show("smallGrid3D x 2, k = %d" % k, out)
    r = out["result"]
    assert r.outcome == dpgo_amd.MODES_CONVERGED and r.block == block and r.negative == 0
    assert np.all(np.abs(out["values"] - D["lam"][:k]) <= out["residuals"] + tmh.allowance(D))
    assert np.all(mr.true_residuals(D["A"], out["values"], out["vectors"]) <= out["residuals"] + tmh.allowance(D))
    assert np.abs(out["vectors"] @ out["vectors"].T - np.eye(k)).max() <= 8 * (D["n"] + block * block) * U


def test_skipped_allocates_nothing(fixtures_dir):
    D = tmh.dense(fixtures_dir, "smallGrid3D")
    grp = make_group(fixtures_dir, "smallGrid3D", 2)
    grp.hessian_modes(D["X"], 8, max_bytes=1)    # (the certificate's buffers and M's values come here)
    free0 = tpol.device_free_bytes()
    out = grp.hessian_modes(D["X"], 8, max_bytes=1)
    assert tpol.device_free_bytes() == free0
    r = out["result"]
    assert r.outcome == dpgo_amd.MODES_SKIPPED and not out["values"].any() and not out["vectors"].any()
    assert r.unknowns == D["n"] and r.fronts >= 4 and r.levels >= 3 and r.max_front > 0 and r.device_bytes > 1 and r.block == 16
    assert r.stationarity >= 0 and r.iterations == 0 and r.factorisations == 0
    assert grp.hessian_modes(D["X"], 8, max_bytes=r.device_bytes - 1)["result"].outcome == dpgo_amd.MODES_SKIPPED
    ok = grp.hessian_modes(D["X"], 8, max_bytes=r.device_bytes)["result"]
    assert ok.outcome == dpgo_amd.MODES_CONVERGED and ok.device_bytes == r.device_bytes
    # a wider block predicts more
    assert grp.hessian_modes(D["X"], 13, max_bytes=1)["result"].device_bytes > r.device_bytes


def test_max_iters_still_delivers(fixtures_dir):
    D = tmh.dense(fixtures_dir, "smallGrid3D")
    out = make_group(fixtures_dir, "smallGrid3D", 2).hessian_modes(D["X"], 8, max_iters=3)
    r = out["result"]
    assert r.outcome == dpgo_amd.MODES_MAX_ITERS and r.iterations == 3 and r.negative == 0
    assert out["residuals"].max() > 1e-8 * r.hmax
    # the pairs of the last iteration: every value within its (large) residual of SOME eigenvalue
    for v, res in zip(out["values"], out["residuals"]):
        assert np.abs(D["lam"] - v).min() <= res + tmh.allowance(D)
    assert np.all(mr.true_residuals(D["A"], out["values"], out["vectors"]) <= out["residuals"] + tmh.allowance(D))


def test_refusals(fixtures_dir):
    path, N, mm, gp, X0 = tc.problem(fixtures_dir, "tinyGrid3D")
    X = tmh.dense(fixtures_dir, "tinyGrid3D")["X"]
    G = dpgo_amd.read_g2o(path, 2)
    hub = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(dpgo_amd.LOSS_HUBER, True), X0=X0)
    with pytest.raises(RuntimeError):
        hub.group.hessian_modes(X, 1)             # a robust loss
    part = dpgo_amd.NodeGroup(G, [0], dpgo_amd.Options.driver(LOSS_NONE, True))
    with pytest.raises(RuntimeError):
        part.hessian_modes(X, 1)                  # a group that does not host every node
    grp = make_group(fixtures_dir, "tinyGrid3D", 2)
    n = 6 * N
    for bad in (dict(k=0), dict(k=-1), dict(k=61), dict(k=n - 6 + 1), dict(k=1, anchor=N), dict(k=1, anchor=-1), dict(k=1, guard=3),
                dict(k=60, guard=5), dict(k=1, max_iters=0), dict(k=1, max_tries=0), dict(k=1, rel_tol=-1.0), dict(k=1, shift=-1.0)):
        with pytest.raises(RuntimeError):
            grp.hessian_modes(X, **bad)
    with pytest.raises(RuntimeError):
        grp.hessian_modes(X[:-1], 1)
    ok = grp.hessian_modes(X, n - 6 if n - 6 <= 60 else 60)     # the most that may be asked for: here every eigenpair
    assert ok["result"].outcome in (dpgo_amd.MODES_CONVERGED, dpgo_amd.MODES_MAX_ITERS) and ok["result"].block == 64


# ---------------------------------------------------------------------------------------------------------------
# the facade and the driver
# ---------------------------------------------------------------------------------------------------------------
_py = {}


def python_run(fixtures_dir):
    """What the driver and the facade example do, through Python: chordal point, 20 AMM-PGO# iterations on 2 nodes, the polish
    and then four modes on the group that iterated."""
    if not _py:
        path = tc.problem(fixtures_dir, "smallGrid3D")[0]
        drv = dpgo_amd.DistPGO(dpgo_amd.read_g2o(path, 2), dpgo_amd.Options.driver(LOSS_NONE, True))
        for _ in range(20):
            assert drv.step() == 0
        Xp, pres, _ = drv.group.polish(drv.X())
        assert pres.outcome == dpgo_amd.POLISH_CONVERGED
        _py["v"] = drv.group.hessian_modes(Xp, 4)
        assert _py["v"]["result"].outcome == dpgo_amd.MODES_CONVERGED
    return _py["v"]


def test_cpp_facade_hessian_modes(fixtures_dir):
    """examples/facade_mm.cpp with `modes 4`: DPGOHashGroup::newton_polish and DPGOHashGroup::hessian_modes after the loop, on
    stderr; stdout the same trace as without; the pairs those of NodeGroup.hessian_modes bit for bit; k = 61 refused."""
    exe = os.path.join(ROOT, "dpgo_amd", "facade_mm")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    args = [exe, os.path.join(fixtures_dir, "smallGrid3D.g2o"), "2", "20", "trivial", "1"]
    plain = subprocess.run(args, check=True, capture_output=True, text=True, timeout=300)
    out = subprocess.run(args + ["modes", "4"], check=True, capture_output=True, text=True, timeout=300)
    assert out.stdout == plain.stdout and "modes" not in plain.stderr
    lines = [l.split() for l in out.stderr.splitlines() if l.startswith("modes: ")]
    want = python_run(fixtures_dir)
    r = want["result"]
    pairs = [l for l in lines if l[1] == "v"]
    assert [int(l[2]) for l in pairs] == [0, 1, 2, 3]
    assert np.array_equal(np.array([float(l[3]) for l in pairs]), want["values"])
    assert np.array_equal(np.array([float(l[4]) for l in pairs]), want["residuals"])
    assert np.array_equal(np.array([[float(v) for v in l[5:]] for l in pairs]), want["vectors"])
    summary = lines[len(pairs)]
    assert summary[1] == "CONVERGED" and [int(v) for v in summary[2:7]] == [r.iterations, r.factorisations, r.shift_tries, r.block, r.negative]
    assert [float(v) for v in summary[7:9]] == [r.mu, r.hmax]
    assert lines[-1][1:] == ["k", "=", "61", "-1"]


def test_dist_pgo_hessian_modes_flags(fixtures_dir, tmp_path):
    """--hessian_modes K --modes_report FILE behind --polish: one line after polish's and the report; without them stdout and the
    result files are what they were.  One flag without the other, and K out of range, are errors; a robust loss says why not."""
    exe = os.path.join(ROOT, "dpgo_amd", "dist_pgo")
    base = [exe, "--dataset", os.path.join(fixtures_dir, "smallGrid3D.g2o"), "--num_nodes", "2", "--iters", "20", "--dist_init", "false"]
    outs = {}
    for tag, extra in (("plain", ["--polish"]), ("modes", ["--polish", "--hessian_modes", "4", "--modes_report", "modes.txt", "--modes_escape"])):
        cwd = tmp_path / tag
        cwd.mkdir()
        outs[tag] = (subprocess.run(base + extra, capture_output=True, text=True, cwd=cwd, timeout=300), cwd)
        assert outs[tag][0].returncode == 0, outs[tag][0].stderr[-2000:]

    def steady(text):   # (the summary's wall time differs from run to run)
        return [l for l in text.splitlines() if not l.startswith(("time: ", "modes: "))]

    assert steady(outs["plain"][0].stdout) == steady(outs["modes"][0].stdout)
    assert "modes" not in outs["plain"][0].stdout and not (outs["plain"][1] / "modes.txt").exists()
    assert sorted(os.listdir(outs["plain"][1])) == sorted(f for f in os.listdir(outs["modes"][1]) if f != "modes.txt")
    tail = outs["modes"][0].stdout.rstrip().splitlines()[-2:]
    assert tail[0].startswith("polish: ") and tail[1].startswith("modes: ")
    want = python_run(fixtures_dir)
    r = want["result"]
    f = tail[1].split()
    assert f[1] == "CONVERGED" and [int(v) for v in f[2:7]] == [r.iterations, r.factorisations, r.shift_tries, r.block, r.negative]
    assert float(f[7]) == want["values"][0] and float(f[8]) == r.mu and int(f[9]) == r.device_bytes
    assert int(f[10]) == 0 and float(f[11]) == float(f[12]) == r.F                 # a minimum: nothing to escape from
    rows = open(outs["modes"][1] / "modes.txt").read().splitlines()
    head = rows[0].split()
    assert head[0::2] == ["k", "n", "mu", "hmax"] and int(head[1]) == 4 and int(head[3]) == r.unknowns and float(head[7]) == r.hmax
    assert len(rows) == 1 + 2 * 4
    for j in range(4):
        a = rows[1 + 2 * j].split()
        assert int(a[0]) == j and float(a[1]) == want["values"][j] and float(a[2]) == want["residuals"][j]
        assert int(a[3]) == int(np.argmax(want["energy"][j])) and float(a[4]) == want["energy"][j].max()
        assert np.array_equal(np.array([float(v) for v in rows[2 + 2 * j].split()]), want["vectors"][j])
    # the result files are the polished point's, escape flag or not (nothing escaped)
    assert open(outs["plain"][1] / "estimates_trivial.txt").read() == open(outs["modes"][1] / "estimates_trivial.txt").read()
    quick = base[:-4] + ["--iters", "5", "--dist_init", "false", "--save", "false"]
    for bad in (["--hessian_modes", "4"], ["--modes_report", "m.txt"], ["--hessian_modes", "61", "--modes_report", "m.txt"]):
        res = subprocess.run(quick + bad, capture_output=True, text=True, cwd=tmp_path, timeout=300)
        assert res.returncode != 0 and not (tmp_path / "m.txt").exists()
    hub = subprocess.run(quick + ["--loss", "huber", "--hessian_modes", "4", "--modes_report", "m.txt"], capture_output=True, text=True,
                         cwd=tmp_path, timeout=300)
    assert hub.returncode == 0 and "modes: not computed" in hub.stdout and not (tmp_path / "m.txt").exists()
