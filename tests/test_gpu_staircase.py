"""The Riemannian staircase on the device (Group::staircase: the kernels of stair.hip, the certificate's products, verify on the
Lambda of the lifted point, the rounding, the polish) on the inputs the feature was asked for on: the twisted ring, which it
takes from a local minimum to the certified global one; tinyGrid3D, where it solves the relaxation and reports that it is not
tight; smallGrid3D, where there is nothing to escape.

Intermediate levels are printed, not asserted: two correct runs may leave a level by different doors.  The certified optimum
has one value, and that value is what is held.  With the restated S = S(Y_dev) and its dense lambda_min on the CPU
(staircase_restatement.weak_duality_interval) every feasible X has F(X) >= 1/2 sum tr Lambda_p + 1/2 min(lambda_min, 0) |X|_F^2,
and F(Y_dev) = 1/2 sum tr Lambda_p + 1/2 <Y_dev, S Y_dev>: F_sdp and F_final must lie within that interval's width of the CPU's
certified optimum F*, plus the evaluation's rounding floor u |X|_F |M X|_F and the interval's own rounding (its `err`).
The TNT runs with the tight options of the host tests (the absolute gradient test at 1e-8 alone).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import newton_restatement as nr  # noqa: E402
import staircase_restatement as st  # noqa: E402
import test_gpu_certify as tc  # noqa: E402  (its inputs and caches; none of its tests is imported)
import test_gpu_cert_proof as tp  # noqa: E402  (likewise)
import test_gpu_covariance as tcov  # noqa: E402  (likewise: the converged points)
import test_gpu_polish as tpol  # noqa: E402  (likewise: device_free_bytes)
import test_staircase_host as tsh  # noqa: E402  (likewise: the rings and the restatement's runs)

import dpgo_amd  # noqa: E402
from oracle.problem import LOSS_NONE  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ROOT = tc.ROOT
TIGHT = st.TIGHT


def ring_group(d, nn):
    g = tsh.ring12(d)[2]
    G = dpgo_amd.graph_from_edges(d, 12, g["I"], g["J"], g["R"], g["t"], g["kappa"], g["tau"], nn)
    return dpgo_amd.NodeGroup(G, range(nn), dpgo_amd.Options.driver(LOSS_NONE, True, max_iterations=0))


def twisted_start(d):
    return tsh.synthetic.twisted_ring(d, 12, 0.02, 1, 1)[1]


def show(tag, res, log):
    for L in log:
        print("%s: rank %d, F %.10g -> %.10g, |grad| %.3g, %d iterations, %d products, %s, theta %.6g, alpha %g, %d halvings" %
              (tag, L[0], L[1], L[2], L[3], L[4], L[5], dpgo_amd.CERT_NAMES[int(L[6])], L[7], L[8], L[9]))
    print("%s: %s at rank %d, %s, F %.10g -> sdp %.10g, rounded %.10g, final %.10g, gap %.3g, sigma %s, %d bytes, %.1f ms "
          "(optimise %.1f, verify %.1f, round %.1f)" %
          (tag, dpgo_amd.STAIR_NAMES[res.outcome], res.final_rank, dpgo_amd.CERT_NAMES[res.cert_status], res.F_initial, res.F_sdp,
           res.F_rounded, res.F_final, res.gap, np.array2string(np.array(res.sigma[:]), precision=4), res.device_bytes, res.total_ms,
           res.optimise_ms, res.verify_ms, res.round_ms))


def evaluation_floor(M, X):
    return U * float(np.linalg.norm(X)) * float(np.linalg.norm(M @ X))


def value_bound(M, X):
    """What two fp64 evaluations of F = 1/2 <X, M X> may differ by: the entries of M X are sums of the terms of |M| |X|, whatever
    cancels between them, so 4 u |X|_F | |M| |X| |_F (weak_duality_interval's `err`, for the same reason)."""
    return 4 * U * float(np.linalg.norm(X)) * float(np.linalg.norm(abs(M) @ np.abs(X)))


@pytest.mark.parametrize("d,nn", [(2, 1), (2, 3), (3, 1), (3, 3)])
def test_twisted_ring_reaches_the_certified_optimum(d, nn):
    gp, mm, g, Xt_ref, Xc = tsh.ring12(d)
    M = gp.M
    grp = ring_group(d, nn)
    Xp, pres, _ = grp.polish(twisted_start(d))
    assert pres.outcome == dpgo_amd.POLISH_CONVERGED and grp.verify(Xp)[0].status == dpgo_amd.CERT_NEGATIVE
    Xh, res, log, Y = grp.staircase(Xp, **TIGHT)
    show("ring12 d=%d x %d" % (d, nn), res, log)
    assert res.outcome == dpgo_amd.STAIR_SOLVED and res.cert_status == dpgo_amd.CERT_PROVEN
    assert d < res.final_rank <= 2 * d and res.levels == len(log) == res.final_rank - d + 1
    assert res.replaced_by_input == 0
    assert grp.verify(Xh)[0].status == dpgo_amd.CERT_PROVEN
    assert not Y[:, res.final_rank:].any()
    Yr = st.rot(Y, d)
    assert np.abs(Yr @ Yr.transpose(0, 2, 1) - np.eye(d)).max() <= 64 * U
    # the value
    Fstar = st.objective(M, Xc)
    lo, hi, lam, err = st.weak_duality_interval(M, Y[:, :res.final_rank], d, float(np.sum(Xc * Xc)))
    floor = evaluation_floor(M, Xc) + evaluation_floor(M, Y) + err
    print("    F* %.15g, interval [%.15g, %.15g] (lambda_min %.3g), F_sdp %.15g, F_final %.15g, floor %.3g" %
          (Fstar, lo, hi, lam, res.F_sdp, res.F_final, floor))
    assert lam >= -0.5e-3
    assert abs(res.F_sdp - Fstar) <= (hi - lo) + floor
    assert abs(res.F_final - Fstar) <= (hi - lo) + floor
    assert abs(res.F_final - st.objective(M, Xh)) <= value_bound(M, Xh) and res.gap == res.F_final - res.F_sdp
    assert abs(res.F_initial - st.objective(M, Xp)) <= value_bound(M, Xp)
    assert res.F_final < 1e-3 * res.F_initial
    # tight: d singular values of sqrt(12), the others small against them
    sig = np.array(res.sigma[:2 * d])
    assert np.all(np.abs(sig[:d] - np.sqrt(12.0)) <= 1e-6) and np.all(sig[d:] <= 1e-4)
    Yh = st.rot(Xh, d)
    assert np.abs(Yh @ Yh.transpose(0, 2, 1) - np.eye(d)).max() <= 64 * U and np.all(np.linalg.det(Yh) > 0)
    # the same bits run to run
    again = grp.staircase(Xp, **TIGHT)
    assert np.array_equal(again[0], Xh) and np.array_equal(again[3], Y) and np.array_equal(again[2], log)
    assert (again[1].F_sdp, again[1].F_final, again[1].tnt_iterations, again[1].hess_products) == \
        (res.F_sdp, res.F_final, res.tnt_iterations, res.hess_products)


@pytest.mark.parametrize("precondition", [1, 0])
def test_tinygrid_is_a_lower_bound_not_a_better_point(fixtures_dir, precondition):
    N, mm, gp, X0, make = tp.instance(fixtures_dir, "tinyGrid3D")
    M, d = gp.M, 3
    X = tcov.converged(fixtures_dir, "tinyGrid3D")
    grp = make(2)[0]
    Xh, res, log, Y = grp.staircase(X, precondition=precondition, **TIGHT)
    show("tinyGrid3D pre=%d" % precondition, res, log)
    ref = tsh.table_run(fixtures_dir, "tinyGrid3D", 3, True)[2]
    assert res.outcome == dpgo_amd.STAIR_SOLVED and res.final_rank == 4 and res.levels == 2
    lo, hi, lam, err = st.weak_duality_interval(M, Y[:, :4], d, float(np.sum(ref["Y"] ** 2)))
    floor = evaluation_floor(M, Y) + evaluation_floor(M, ref["Y"]) + err
    print("    interval [%.12g, %.12g] (lambda_min %.3g), F_sdp %.12g, the restatement's %.12g, floor %.3g" %
          (lo, hi, lam, res.F_sdp, ref["F_sdp"], floor))
    assert tsh.quoted(ref["F_sdp"], 37.1686023)
    assert abs(res.F_sdp - ref["F_sdp"]) <= (hi - lo) + floor
    assert res.gap > 1.0 and res.gap == res.F_final - res.F_sdp
    assert res.F_final <= res.F_initial + evaluation_floor(M, X)
    assert res.sigma[3] > 1.0                                   # not tight
    assert res.F_rounded > res.F_initial                        # the rounded point is worse; the polish brings it back
    assert abs(res.F_final - st.objective(M, Xh)) <= value_bound(M, Xh) or res.replaced_by_input
    Yh = st.rot(Xh, d)
    assert np.abs(Yh @ Yh.transpose(0, 2, 1) - np.eye(d)).max() <= 64 * U


def test_smallgrid_has_nothing_to_escape(fixtures_dir):
    X = tcov.converged(fixtures_dir, "smallGrid3D")
    grp = tpol.make_group(fixtures_dir, "smallGrid3D", 5)
    Xh, res, log, Y = grp.staircase(X, **TIGHT)
    show("smallGrid3D", res, log)
    assert res.outcome == dpgo_amd.STAIR_SOLVED and res.cert_status == dpgo_amd.CERT_PROVEN
    assert res.levels == 1 and res.final_rank == 3 and log[0, 8] == 0.0 and not Y[:, 3:].any()
    assert res.F_final <= res.F_initial and res.gap >= -value_bound(tp.instance(fixtures_dir, "smallGrid3D")[2].M, X)
    # the defaults (SESyncOpts' tolerances) end there too
    res2 = grp.staircase(X)[1]
    assert res2.outcome == dpgo_amd.STAIR_SOLVED and res2.levels == 1


def test_max_rank_returns_the_input(fixtures_dir):
    """r_max = d: nothing can be escaped; Xhat is the polished input up to the gauge -- the same value within what the two
    gradients allow, |g|^2 / (2 lambda_min(H)) each, plus the evaluation's floor."""
    d = 2
    gp = tsh.ring12(d)[0]
    grp = ring_group(d, 3)
    Xp = grp.polish(twisted_start(d))[0]
    Xh, res, log, Y = grp.staircase(Xp, r_max=d, **TIGHT)
    show("ring12 d=2 r_max=2", res, log)
    assert res.outcome == dpgo_amd.STAIR_MAX_RANK and res.final_rank == d and res.levels == 1
    assert res.cert_status == dpgo_amd.CERT_NEGATIVE and res.theta < -0.5e-3   # (the search stops at the first Ritz value below -eta / 2)
    lam_min = float(np.linalg.eigvalsh(nr.anchored_hessian(gp.M, Xp, d, 0))[0])
    g2 = sum(float(np.linalg.norm(nr.grad(gp.M, Z, d, 0))) ** 2 for Z in (Xp, Xh))
    assert lam_min > 0
    assert abs(st.objective(gp.M, Xh) - st.objective(gp.M, Xp)) <= g2 / (2 * lam_min) + 2 * value_bound(gp.M, Xp)
    assert res.F_final <= res.F_initial


def test_skipped_allocates_nothing(fixtures_dir):
    X = tcov.converged(fixtures_dir, "smallGrid3D")
    grp = tpol.make_group(fixtures_dir, "smallGrid3D", 2)
    grp.staircase(X, max_bytes=1)       # (the certificate's buffers come here)
    free0 = tpol.device_free_bytes()
    Xh, res, log, Y = grp.staircase(X, max_bytes=1)
    assert tpol.device_free_bytes() == free0
    assert res.outcome == dpgo_amd.STAIR_SKIPPED and np.array_equal(Xh, X) and len(log) == 0 and not Y.any()
    assert res.device_bytes > 8 * 24 * X.size and res.levels == 0
    assert grp.staircase(X, max_bytes=res.device_bytes - 1)[1].outcome == dpgo_amd.STAIR_SKIPPED
    ok = grp.staircase(X, max_bytes=res.device_bytes)[1]
    assert ok.outcome == dpgo_amd.STAIR_SOLVED and ok.device_bytes == res.device_bytes


def test_refusals(fixtures_dir):
    path, N, mm, gp, X0 = tc.problem(fixtures_dir, "smallGrid3D")
    X = tcov.converged(fixtures_dir, "smallGrid3D")
    G = dpgo_amd.read_g2o(path, 2)
    hub = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(dpgo_amd.LOSS_HUBER, True), X0=X0)
    Yl = st.lift(X, 3)
    with pytest.raises(RuntimeError):
        hub.group.staircase(X)                   # a robust loss
    with pytest.raises(RuntimeError):
        hub.group.stair_eval(Yl)
    part = dpgo_amd.NodeGroup(G, [0], dpgo_amd.Options.driver(LOSS_NONE, True))
    with pytest.raises(RuntimeError):
        part.staircase(X)                        # a group that hosts one of two nodes
    with pytest.raises(RuntimeError):
        part.stair_round(Yl)
    grp = tpol.make_group(fixtures_dir, "smallGrid3D", 2)
    for bad in (dict(r_max=2), dict(r_max=7), dict(r_max=-1), dict(max_iterations=-1), dict(grad_norm_tol=-1.0), dict(STPCG_kappa=0.0),
                dict(min_eig_num_tol=-1.0)):
        with pytest.raises(RuntimeError):
            grp.staircase(X, **bad)
    with pytest.raises(RuntimeError):
        grp.staircase(X[:-1])                    # a short leading dimension
    import ctypes as C
    L = dpgo_amd.lib()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    Xf = np.asfortranarray(X)
    out, r, o = np.full(Xf.shape, 7.0, order="F"), dpgo_amd.StaircaseResult(), dpgo_amd.StaircaseOptions()
    rows = Xf.shape[0]
    assert L.dpgo_group_staircase(grp._h, dp(Xf), rows, C.byref(o), 0, dp(out), rows - 1, None, 0, None, 0, C.byref(r)) == -1
    assert L.dpgo_group_staircase(grp._h, dp(Xf), rows, C.byref(o), 0, None, rows, None, 0, None, 0, C.byref(r)) == -1
    assert L.dpgo_group_staircase(grp._h, None, rows, C.byref(o), 0, dp(out), rows, None, 0, None, 0, C.byref(r)) == -1
    assert L.dpgo_group_staircase(grp._h, dp(Xf), rows, C.byref(o), 0, dp(out), rows, None, 0, None, 0, None) == -1
    assert L.dpgo_group_staircase(grp._h, dp(Xf), rows, C.byref(o), 0, dp(out), rows, None, 0, None, 3, C.byref(r)) == -1
    assert np.all(out == 7.0)                    # (touched nothing)
    assert grp.staircase(X)[1].outcome == dpgo_amd.STAIR_SOLVED


def test_staircase_does_not_disturb_the_optimiser(fixtures_dir):
    """20 AMM-PGO# iterations with a staircase on a sibling trivial-loss group after every fifth: bit for bit the run without."""
    path = tc.problem(fixtures_dir, "tinyGrid3D")[0]
    runs = []
    for with_stair in (False, True):
        drv = dpgo_amd.DistPGO(dpgo_amd.read_g2o(path, 2), dpgo_amd.Options.driver(LOSS_NONE, True))
        sib = tc.group(path, 2)[0] if with_stair else None
        for it in range(20):
            assert drv.step() == 0
            if with_stair and it % 5 == 4:
                assert sib.staircase(drv.X())[1].outcome != dpgo_amd.STAIR_SKIPPED
        runs.append(np.array(drv.X()))
    assert np.array_equal(runs[0], runs[1])


# ---------------------------------------------------------------------------------------------------------------
# the facade and the driver
# ---------------------------------------------------------------------------------------------------------------
_py = {}
FIELDS = ("final_rank", "F_initial", "F_sdp", "F_final", "gap")


def python_run(fixtures_dir):
    """What the driver and the facade example do, through Python: chordal point, 100 AMM-PGO# iterations of tinyGrid3D on 2
    nodes, then on the group that iterated the staircase from that point (the facade), and the polish with the staircase from
    the polished point (the driver with --polish --staircase)."""
    if not _py:
        path = tc.problem(fixtures_dir, "tinyGrid3D")[0]
        drv = dpgo_amd.DistPGO(dpgo_amd.read_g2o(path, 2), dpgo_amd.Options.driver(LOSS_NONE, True))
        for _ in range(100):
            assert drv.step() == 0
        X = np.array(drv.X())
        _py["facade"] = drv.group.staircase(X)
        _py["driver"] = drv.group.staircase(drv.group.polish(X)[0])
        for v in _py.values():
            assert v[1].outcome in (dpgo_amd.STAIR_SOLVED, dpgo_amd.STAIR_MAX_RANK) and v[1].final_rank >= 4 and v[1].gap > 1.0
    return _py


def check_line(fields, res):
    assert fields[1] == dpgo_amd.STAIR_NAMES[res.outcome] and int(fields[2]) == res.final_rank
    assert [float(v) for v in fields[3:7]] == [res.F_initial, res.F_sdp, res.F_final, res.gap]


def test_cpp_facade_riemannian_staircase(fixtures_dir):
    """examples/facade_mm.cpp with `staircase`: DPGOHashGroup::riemannian_staircase after the loop, on stderr; stdout the same
    trace as without; the point and the numbers those of NodeGroup.staircase bit for bit."""
    exe = os.path.join(ROOT, "dpgo_amd", "facade_mm")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    args = [exe, os.path.join(fixtures_dir, "tinyGrid3D.g2o"), "2", "100", "trivial", "1"]
    plain = subprocess.run(args, check=True, capture_output=True, text=True, timeout=300)
    out = subprocess.run(args + ["staircase"], check=True, capture_output=True, text=True, timeout=300)
    assert out.stdout == plain.stdout and "staircase" not in plain.stderr
    lines = [l.split() for l in out.stderr.splitlines() if l.startswith("staircase: ")]
    Xh, res, _, _ = python_run(fixtures_dir)["facade"]
    check_line(lines[-1], res)
    assert [int(l[2]) for l in lines[:-1]] == list(range(Xh.shape[0]))
    assert np.array_equal(np.array([[float(v) for v in l[3:]] for l in lines[:-1]]), Xh)


def test_dist_pgo_staircase_flag(fixtures_dir, tmp_path):
    """--staircase adds one line behind --polish's and ahead of --verify's, which then acts on Xhat; without it stdout is what it
    was.  A robust loss: the line says why there is no staircase."""
    exe = os.path.join(ROOT, "dpgo_amd", "dist_pgo")
    base = [exe, "--dataset", os.path.join(fixtures_dir, "tinyGrid3D.g2o"), "--num_nodes", "2", "--iters", "100", "--dist_init", "false",
            "--save", "false"]
    outs = {}
    for tag, extra in (("plain", ["--polish", "--verify"]), ("stair", ["--polish", "--staircase", "--verify"])):
        outs[tag] = subprocess.run(base + extra, capture_output=True, text=True, cwd=tmp_path, timeout=300)
        assert outs[tag].returncode == 0, outs[tag].stderr[-2000:]

    def steady(text):   # (the summary's wall time differs from run to run)
        return [l for l in text.splitlines() if not l.startswith(("time: ", "staircase: ", "verification: "))]

    assert steady(outs["plain"].stdout) == steady(outs["stair"].stdout) and "staircase" not in outs["plain"].stdout
    tail = outs["stair"].stdout.rstrip().splitlines()[-3:]
    assert tail[0].startswith("polish: ") and tail[1].startswith("staircase: ") and tail[2].startswith("verification: ")
    check_line(tail[1].split(), python_run(fixtures_dir)["driver"][1])
    assert tail[2].split()[1] == "NEGATIVE"      # tinyGrid3D: Xhat is the local minimum again; the line above carries the bound
    hub = subprocess.run(base[:-6] + ["--iters", "5", "--dist_init", "false", "--loss", "huber", "--staircase", "--save", "false"],
                         capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert hub.returncode == 0 and "staircase: not computed" in hub.stdout
