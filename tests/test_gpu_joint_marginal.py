"""Joint marginals of a pose set on the device (dpgo_amd/csrc/marg.h): NodeGroup.joint_marginal on tinyGrid3D x {1, 2} nodes,
smallGrid3D x {1, 5} and the d = 2 ladder x 6, anchors 0 and N - 1, at the POLISHED points and with the references and groups of
tests/test_gpu_pairs.py (the restated anchored H, its long-double Cholesky factor, bSigma).

Bounds (tests/marg_restatement.py); nothing in them comes from the device.
  cov              absolute: bSigma entrywise against the long-double inverse; relative: margin_rel against the restatement
  info, logdet     info_bound, logdet_bound from the entrywise bound B of cov; every kept set is asserted to satisfy
                   rho = |B|_2 |cov^-1|_2 <= 0.1 (absolute: n bSigma |cov^-1|_2) -- a condition on the inputs, not a tolerance
  partitions       twice the bound, each side being within it of the same reference
  two anchors      the relative form under anchors 0 and N - 1: the two margins plus the difference the restatement itself shows
                   between the two at this point (the point is critical to rounding only)
The device's worst figure per case is printed and held below 1.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_restatement as cr  # noqa: E402
import marg_restatement as mr  # noqa: E402
import test_gpu_certify as tc  # noqa: E402  (its inputs; none of its tests is imported)
import test_gpu_covariance as tgc  # noqa: E402  (its groups; none of its tests is imported)
import test_gpu_cert_proof as tp  # noqa: E402
import test_gpu_pairs as tgp  # noqa: E402  (its polished points and references; none of its tests is imported)

import dpgo_amd  # noqa: E402
from oracle.problem import LOSS_NONE  # noqa: E402

pytestmark = pytest.mark.gpu

LD, U = mr.LD, mr.U
# (fixture, nodes, kept poses): every non-anchor pose of the tiny grid; 11 poses = 66 columns, the eleventh astride the batch
# edge; 22 poses = 132 columns in three batches; d = 2: 22 poses = 66 columns
CASES = [("tinyGrid3D", 1, 8), ("tinyGrid3D", 2, 8), ("smallGrid3D", 1, 11), ("smallGrid3D", 5, 11), ("smallGrid3D", 1, 22),
         ("smallGrid3D", 5, 22), ("ladder2", 6, 22)]


def seeded_keep(N, anchor, seed, count, with_anchor=False):
    """Distinct seeded poses in seeded (unsorted) order, the first and the last pose of the range that are not the anchor among
    them (they lie on different nodes of every partition); with_anchor: the anchor second."""
    rng = np.random.default_rng(seed)
    ends = [g for g in (0, 1, N - 2, N - 1) if g != anchor]
    ends = [ends[0], ends[-1]]
    pool = [g for g in range(N) if g != anchor and g not in ends]
    keep = ends + [int(g) for g in rng.permutation(pool)[:count - 2 - (1 if with_anchor else 0)]]
    keep = [int(keep[i]) for i in rng.permutation(len(keep))]
    if with_anchor:
        keep.insert(1, anchor)
    assert len(set(keep)) == count and keep != sorted(keep)
    return keep


# The relative form's sets: pose 0 second (the anchor itself under anchor 0), the others seeded.  For the two larger graphs they were
# picked on the CPU, among seeded sets of four at the points of tests/test_marg_host.py, as sets that keep rho <= 0.1 under both
# anchors and every base below with the whole bSigma: a relative covariance has the information of a chain of edges for its
# inverse, and bSigma carries the Hessian's own error, so a larger set or one with two neighbours does not satisfy the condition.
REL_KEEP = {"tinyGrid3D": None, "smallGrid3D": [51, 0, 90, 47], "ladder2": [243, 0, 388, 346]}

_want = {}


def wanted(fixtures_dir, name, anchor, keep, base):
    """The long-double answers and the bounds of a call, once: cov, info, logdet, the entrywise bound of cov, those of info and
    logdet; rho is asserted."""
    key = (name, anchor, tuple(keep), base)
    if key not in _want:
        R = tgp.reference(fixtures_dir, name, anchor)
        d, dof, X = R["d"], R["dof"], R["X"]
        S = mr.sigma_kk(R["A"], dof, keep, anchor, R["L"])
        if base is None:
            cov, bound = S, np.full(S.shape, R["bSigma"])
        else:
            cov = mr.rel_cov(mr.jacobian_set(X, d, keep, base, LD), S)
            bound = mr.margin_rel(X, d, keep, base, anchor, np.asarray(S, np.float64), R["bSigma"])
        rho = mr.rho_of(cov, bound)
        assert rho <= 0.1, "the kept set does not satisfy the condition rho <= 0.1: %g" % rho
        info, logdet, sal = mr.inverse_ld(cov)
        _want[key] = dict(cov=cov, info=info, logdet=logdet, b_cov=bound, b_info=mr.info_bound(cov, bound),
                          b_logdet=mr.logdet_bound(cov, bound, sal), rho=rho)
    return _want[key]


def ratios(out, W):
    return np.array([float(np.max(np.abs(np.asarray(out["cov"], LD) - W["cov"]) / (W["b_cov"] + 1e-300))),
                     float(np.abs(np.asarray(out["info"], LD) - W["info"]).max() / W["b_info"]),
                     float(abs(LD(out["logdet"]) - W["logdet"]) / W["b_logdet"])])


_first = {}


@pytest.mark.parametrize("name,nn,count", CASES)
def test_absolute_form_against_the_restatement_and_the_pair_covariances(fixtures_dir, name, nn, count):
    grp = tgc.make_group(fixtures_dir, name, nn)
    N = tp.instance(fixtures_dir, name)[0]
    for a in (0, N - 1):
        R = tgp.reference(fixtures_dir, name, a)
        dof = R["dof"]
        keep = seeded_keep(N, a, 5 + count, count)
        if nn > 1:
            assert len({tgp.node_of(grp, g) for g in keep}) > 1
        W = wanted(fixtures_dir, name, a, keep, None)
        out = grp.joint_marginal(R["X"], keep, anchor=a)
        res = out["result"]
        assert res.outcome == dpgo_amd.MARG_OK and not res.info_not_pd and res.unknowns == dof * N and res.pivot_min > 0
        assert res.n == dof * count and res.columns == dof * count and res.batches == (res.columns + 63) // 64
        assert res.dense_pivot_min > 0 and res.device_bytes > 0 and out["order"].tolist() == keep
        w = ratios(out, W)
        print("%s x %d, anchor %d, %d poses: n = %d, %d batches, rho %.3g; cov %.3g, info %.3g, logdet %.3g of their bounds"
              % (name, nn, a, count, res.n, res.batches, W["rho"], w[0], w[1], w[2]))
        assert w.max() < 1.0, w
        assert np.array_equal(out["cov"], out["cov"].T) and np.array_equal(out["info"], out["info"].T)
        if count == N - 1:   # every other pose kept: the information matrix is the restated H itself
            idx = mr.unknowns(dof, keep)
            assert np.abs(out["info"] - R["A"][np.ix_(idx, idx)]).max() <= W["b_info"]
        # the same bits on a second call; without the information form, the same cov
        again = grp.joint_marginal(R["X"], keep, anchor=a)
        assert all(np.array_equal(again[k], out[k]) for k in ("cov", "info")) and again["logdet"] == out["logdet"]
        bare = grp.joint_marginal(R["X"], keep, anchor=a, want_info=False)
        assert np.array_equal(bare["cov"], out["cov"]) and bare["info"] is None and bare["logdet"] is None
        # the lower entries are pair_covariance's joint blocks: S_pq with p = keep[k], q = keep[l], k > l; the lower triangle of S_pp
        ks = list(range(0, count, max(count // 6, 1)))
        pairs = [(keep[k], keep[l]) for k in ks for l in ks if k > l]
        pc = grp.pair_covariance(R["X"], pairs, anchor=a)["joint"]
        for i, (k, l) in enumerate((k, l) for k in ks for l in ks if k > l):
            blk = lambda r, c: out["cov"][dof * r:dof * r + dof, dof * c:dof * c + dof]
            assert np.array_equal(blk(k, l), pc[i][1]) and np.array_equal(np.tril(blk(k, k)), np.tril(pc[i][0]))
        # every partition: other orderings, other fronts, the same answer
        first = _first.setdefault((name, a, count), out)
        assert np.all(np.abs(out["cov"] - first["cov"]) <= 2 * W["b_cov"]) and np.abs(out["info"] - first["info"]).max() <= 2 * W["b_info"]
        assert abs(out["logdet"] - first["logdet"]) <= 2 * W["b_logdet"]


@pytest.mark.parametrize("name,nn", [("tinyGrid3D", 2), ("smallGrid3D", 5), ("ladder2", 6)])
def test_relative_form(fixtures_dir, name, nn):
    grp = tgc.make_group(fixtures_dir, name, nn)
    N = tp.instance(fixtures_dir, name)[0]
    X = tgp.reference(fixtures_dir, name, 0)["X"]
    d = tgp.reference(fixtures_dir, name, 0)["d"]
    keep = REL_KEEP[name] or seeded_keep(N, 0, 21, 6, with_anchor=True)   # (pose 0 is the anchor, or an ordinary pose under N - 1)
    if nn > 1:
        assert len({tgp.node_of(grp, g) for g in keep}) > 1
    outs = {}
    for a in (0, N - 1):
        for base in (keep[0], keep[-1], 0):   # the base first, last, and pose 0 -- the anchor itself under anchor 0
            W = wanted(fixtures_dir, name, a, keep, base)
            out = grp.joint_marginal(X, keep, anchor=a, base=base)
            res = out["result"]
            dof = cr.dof_of(d)
            ncol = dof * (len(keep) - (1 if a in keep else 0))
            assert res.outcome == dpgo_amd.MARG_OK and not res.info_not_pd and res.n == dof * (len(keep) - 1) and res.columns == ncol
            assert out["order"].tolist() == [g for g in keep if g != base]
            w = ratios(out, W)
            print("%s x %d, anchor %d, base %d: rho %.3g; cov %.3g, info %.3g, logdet %.3g of their bounds" % (name, nn, a, base, W["rho"], w[0], w[1], w[2]))
            assert w.max() < 1.0, w
            assert np.array_equal(out["cov"], out["cov"].T) and np.array_equal(out["info"], out["info"].T)
            assert np.array_equal(grp.joint_marginal(X, keep, anchor=a, base=base)["cov"], out["cov"])
            outs[(a, base)] = (out, W)
    # the gauge-free summary: the two anchors give the same relative covariance to first order at a critical point
    for base in (keep[0], keep[-1], 0):
        (o0, W0), (o1, W1) = outs[(0, base)], outs[(N - 1, base)]
        own = np.asarray(np.abs(W0["cov"] - W1["cov"]), np.float64)
        assert np.all(np.abs(o0["cov"] - o1["cov"]) <= W0["b_cov"] + W1["b_cov"] + own)
        print("%s, base %d: the restatement's own difference between the anchors %.3g" % (name, base, own.max()))
    # K = 2: pair_covariance's rel, each within its margin of the same restatement
    p, q = keep[2], keep[3]
    two = grp.joint_marginal(X, [p, q], base=p)
    W = wanted(fixtures_dir, name, 0, [p, q], p)
    rel = grp.pair_covariance(X, [(p, q)])["rel"][0]
    assert np.all(np.abs(two["cov"] - rel) <= 2 * W["b_cov"]) and ratios(two, W).max() < 1.0


def test_a_point_that_is_no_minimum_and_the_calls_around_it(fixtures_dir):
    R = tgp.reference(fixtures_dir, "smallGrid3D", 0)
    grp = tgc.make_group(fixtures_dir, "smallGrid3D", 2)
    keep = seeded_keep(R["N"], 0, 3, 5)
    before = grp.joint_marginal(R["X"], keep)
    bad = grp.joint_marginal(cr.random_rotations_point(R["X"], R["d"], 5), keep)
    assert bad["result"].outcome == dpgo_amd.MARG_NOT_PD and not bad["cov"].any() and not bad["info"].any() and bad["logdet"] == 0.0
    after = grp.joint_marginal(R["X"], keep)
    assert after["result"].outcome == dpgo_amd.MARG_OK
    assert np.array_equal(before["cov"], after["cov"]) and np.array_equal(before["info"], after["info"]) and before["logdet"] == after["logdet"]


def test_skipped_allocates_nothing_and_predicts_what_a_run_reports(fixtures_dir):
    R = tgp.reference(fixtures_dir, "smallGrid3D", 0)
    grp = tgc.make_group(fixtures_dir, "smallGrid3D", 2)
    keep = seeded_keep(R["N"], 0, 4, 7)
    grp.joint_marginal(R["X"], keep, max_bytes=1)   # (the certificate's buffers and M's values come here)
    free0 = tgp.device_free_bytes()
    out = grp.joint_marginal(R["X"], keep, max_bytes=1)
    assert tgp.device_free_bytes() == free0
    res = out["result"]
    assert res.outcome == dpgo_amd.MARG_SKIPPED and not out["cov"].any() and not out["info"].any()
    assert res.unknowns == 6 * R["N"] and res.n == 42 and res.columns == 42 and res.batches == 1 and res.stationarity > 0
    assert grp.joint_marginal(R["X"], keep, max_bytes=res.device_bytes - 1)["result"].outcome == dpgo_amd.MARG_SKIPPED
    ok = grp.joint_marginal(R["X"], keep, max_bytes=res.device_bytes)
    assert ok["result"].outcome == dpgo_amd.MARG_OK and ok["result"].device_bytes == res.device_bytes
    assert ratios(ok, wanted(fixtures_dir, "smallGrid3D", 0, keep, None)).max() < 1.0
    bare = grp.joint_marginal(R["X"], keep, want_info=False, max_bytes=1)["result"]
    assert bare.outcome == dpgo_amd.MARG_SKIPPED and bare.device_bytes < res.device_bytes   # (no dense factor to count)


def test_refusals(fixtures_dir):
    path, N, mm, gp, X0 = tc.problem(fixtures_dir, "smallGrid3D")
    X = tgp.reference(fixtures_dir, "smallGrid3D", 0)["X"]
    G = dpgo_amd.read_g2o(path, 2)
    hub = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(dpgo_amd.LOSS_HUBER, True), X0=X0)
    with pytest.raises(RuntimeError):
        hub.group.joint_marginal(X, [1, 5])              # a robust loss
    part = dpgo_amd.NodeGroup(G, [0], dpgo_amd.Options.driver(LOSS_NONE, True))
    with pytest.raises(RuntimeError):
        part.joint_marginal(X, [1, 5])                   # a group that does not host every node
    grp = tgc.make_group(fixtures_dir, "smallGrid3D", 2)
    bad = [dict(keep=[1, 5], anchor=N), dict(keep=[1, 5], anchor=-1), dict(keep=[1, N]), dict(keep=[-1, 3]), dict(keep=[4, 9, 4]),
           dict(keep=[0, 5]),                            # the anchor kept without a base
           dict(keep=[3, 5], anchor=5),
           dict(keep=[1, 5], base=7),                    # a base that is not kept
           dict(keep=[5], base=5)]                       # K < 2 with a base
    for kw in bad:
        with pytest.raises(RuntimeError):
            grp.joint_marginal(X, **kw)
    with pytest.raises(RuntimeError):
        grp.joint_marginal(X[:-1], [1, 5])
    # a null output behind a valid group
    import ctypes as C
    L = dpgo_amd.lib()
    Xf = np.asfortranarray(X)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    K = np.array([1, 5], np.int32)
    ip = K.ctypes.data_as(C.POINTER(C.c_int))
    cov, info, logdet, res = np.zeros(144), np.zeros(144), np.zeros(1), dpgo_amd.MargResult()
    call = lambda k, c, i, l, want, out: L.dpgo_group_joint_marginal(grp._h, dp(Xf), Xf.shape[0], k, 2, 0, -1, want, 0, c, i, l, out)
    assert call(ip, dp(cov), dp(info), dp(logdet), 1, C.byref(res)) == 0 and res.outcome == dpgo_amd.MARG_OK
    assert call(None, dp(cov), dp(info), dp(logdet), 1, C.byref(res)) == -1 and call(ip, None, dp(info), dp(logdet), 1, C.byref(res)) == -1
    assert call(ip, dp(cov), None, dp(logdet), 1, C.byref(res)) == -1 and call(ip, dp(cov), dp(info), None, 1, C.byref(res)) == -1
    assert call(ip, dp(cov), dp(info), dp(logdet), 1, None) == -1
    assert call(ip, dp(cov), None, dp(logdet), 0, C.byref(res)) == 0   # (no information form asked for: no array needed)
    assert grp.joint_marginal(X, [1, 5])["result"].outcome == dpgo_amd.MARG_OK


def test_joint_marginal_does_not_disturb_the_optimiser(fixtures_dir):
    """30 AMM-PGO# iterations with a call on a sibling trivial-loss group after every fifth: bit for bit the run without."""
    path = tc.problem(fixtures_dir, "smallGrid3D")[0]
    runs = []
    for with_call in (False, True):
        drv = dpgo_amd.DistPGO(dpgo_amd.read_g2o(path, 2), dpgo_amd.Options.driver(LOSS_NONE, True))
        sib = tc.group(path, 2)[0] if with_call else None
        trace = []
        for it in range(30):
            assert drv.step() == 0
            if with_call and it % 5 == 4:
                assert sib.joint_marginal(drv.X(), [3, 90, 7], base=90)["result"].outcome in (dpgo_amd.MARG_OK, dpgo_amd.MARG_NOT_PD)
            trace.append([getattr(drv.group.results(a), f) for a in range(2) for f in ("fobj", "gamma", "gradFnorm", "Gk")])
        runs.append((np.array(drv.X()), [drv.group[a].Xk() for a in range(2)], np.array(trace)))
    assert np.array_equal(runs[0][0], runs[1][0])
    for a in range(2):
        assert np.array_equal(runs[0][1][a], runs[1][1][a])
    assert np.array_equal(runs[0][2], runs[1][2])


def test_reweighted_with_unit_weights_is_the_group_call(fixtures_dir):
    path = tc.problem(fixtures_dir, "smallGrid3D")[0]
    R = tgp.reference(fixtures_dir, "smallGrid3D", 0)
    G = dpgo_amd.read_g2o(path, 2)
    keep = seeded_keep(R["N"], 0, 9, 5)
    for base in (None, keep[1]):
        got = dpgo_amd.joint_marginal_reweighted(G, R["X"], LOSS_NONE, keep, base=base)
        want = tgc.make_group(fixtures_dir, "smallGrid3D", 2).joint_marginal(R["X"], keep, base=base)
        assert got["result"].outcome == dpgo_amd.MARG_OK and got["summary"].num_downweighted == 0
        assert np.array_equal(got["cov"], want["cov"]) and np.array_equal(got["info"], want["info"]) and got["logdet"] == want["logdet"]


# ---------------------------------------------------------------------------------------------------------------
# the drivers
# ---------------------------------------------------------------------------------------------------------------
KEPT = [7, 2, 5, 3]
_py = {}


def python_run(fixtures_dir, base):
    """What the drivers do on tinyGrid3D x 2: 30 iterations, the polish, the joint marginal of KEPT."""
    if base not in _py:
        drv = dpgo_amd.DistPGO(dpgo_amd.read_g2o(os.path.join(fixtures_dir, "tinyGrid3D.g2o"), 2), dpgo_amd.Options.driver(LOSS_NONE, True))
        for _ in range(30):
            assert drv.step() == 0
        Xp, pres, _ = drv.group.polish(drv.X())
        assert pres.outcome == dpgo_amd.POLISH_CONVERGED
        out = drv.group.joint_marginal(Xp, KEPT, base=base)
        assert out["result"].outcome == dpgo_amd.MARG_OK and not out["result"].info_not_pd
        _py[base] = out
    return _py[base]


def test_dist_pgo_marginal_flags(fixtures_dir, tmp_path):
    """--polish --marginal_set FILE --marginal_report FILE [--marginal_base P] adds the report and one line after the summary; the
    report holds NodeGroup.joint_marginal's numbers bit for bit; a robust loss says why not; one flag alone is an error."""
    import subprocess
    exe = os.path.join(tc.ROOT, "dpgo_amd", "dist_pgo")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    (tmp_path / "set.txt").write_text("".join("%d\n" % p for p in KEPT))
    path = os.path.join(fixtures_dir, "tinyGrid3D.g2o")
    common = [exe, "--dataset", path, "--num_nodes", "2", "--iters", "30", "--dist_init", "false", "--save", "false"]
    for base, extra in ((None, []), (5, ["--marginal_base", "5"])):
        run = subprocess.run(common + ["--polish", "--marginal_set", "set.txt", "--marginal_report", "marg.txt"] + extra, capture_output=True,
                             text=True, cwd=tmp_path, timeout=300)
        assert run.returncode == 0, run.stderr[-2000:]
        lines = [l for l in run.stdout.splitlines() if l.startswith("marginal: ")]
        assert len(lines) == 1 and run.stdout.rstrip().splitlines()[-1] == lines[0]
        want = python_run(fixtures_dir, base)
        res = want["result"]
        f = lines[0].split()
        assert f[1] == "OK" and [int(v) for v in f[2:8]] == [len(KEPT), res.n, res.columns, res.batches, res.device_bytes, 0]
        assert float(f[8]) == want["logdet"]
        text = (tmp_path / "marg.txt").read_text().splitlines()
        assert text[0].split()[:2] == ["n", str(res.n)] and float(text[0].split()[3]) == want["logdet"]
        assert [int(v) for v in text[1].split()] == want["order"].tolist()
        rows = np.array([[float(v) for v in l.split()] for l in text[2:]])
        assert rows.shape == (2 * res.n, res.n)
        assert np.array_equal(rows[:res.n], want["cov"]) and np.array_equal(rows[res.n:], want["info"])
    hub = subprocess.run(common + ["--loss", "huber", "--marginal_set", "set.txt", "--marginal_report", "m2.txt"], capture_output=True, text=True,
                         cwd=tmp_path, timeout=300)
    assert hub.returncode == 0 and "marginal: not computed" in hub.stdout and not (tmp_path / "m2.txt").exists()
    one = subprocess.run(common[:-6] + ["--iters", "1", "--dist_init", "false", "--save", "false", "--marginal_set", "set.txt"],
                         capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert one.returncode != 0


def test_cpp_facade_joint_marginal(fixtures_dir, tmp_path):
    """examples/facade_mm.cpp with `marginal FILE [BASE]`: DPGOHashGroup::newton_polish and ::joint_marginal after the loop, on
    stderr; stdout the same trace as without; cov, info and logdet those of NodeGroup.joint_marginal bit for bit; a pose listed
    twice refused."""
    import subprocess
    exe = os.path.join(tc.ROOT, "dpgo_amd", "facade_mm")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    (tmp_path / "set.txt").write_text("".join("%d\n" % p for p in KEPT))
    args = [exe, os.path.join(fixtures_dir, "tinyGrid3D.g2o"), "2", "30", "trivial", "1"]
    plain = subprocess.run(args, check=True, capture_output=True, text=True, timeout=300)
    for base, extra in ((None, []), (5, ["5"])):
        out = subprocess.run(args + ["marginal", str(tmp_path / "set.txt")] + extra, check=True, capture_output=True, text=True, timeout=300)
        assert out.stdout == plain.stdout and "marginal" not in plain.stderr
        lines = [l.split() for l in out.stderr.splitlines() if l.startswith("marginal: ")]
        want = python_run(fixtures_dir, base)
        res = want["result"]
        n = res.n
        assert len(lines) == 2 * n + 2 and lines[-2][1:6] == ["OK", str(n), str(res.columns), str(res.batches), "0"]
        assert float(lines[-2][6]) == want["logdet"]
        got = {w: np.array([[float(v) for v in l[3:]] for l in lines if l[1] == w]) for w in ("cov", "info")}
        assert np.array_equal(got["cov"], want["cov"]) and np.array_equal(got["info"], want["info"])
        assert lines[-1][1:] == ["repeated", "pose", "-1"]
