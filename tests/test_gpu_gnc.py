"""Graduated non-convexity on the device (NodeGroup.gnc: k_gnc_edge's weights, one polish_loop per level) against its numpy
restatement (tests/gnc_restatement.run) on the committed runs of tests/golden/gnc_reference.npz (made on the CPU by
tests/golden/make_gnc_reference.py; tests/test_gnc_host.py checks the file against the restatement).

Held exactly: the outcome, the number of levels, the counts of w == 0, w == 1 and 0 < w < 1 of every level, num_outliers, the
set {w == 0}, the same bits on a second call, the anchor's rows.  F_w and F_mu of every level (four columns of the log) are held
within max(100 D_k, 1e-10 |F|), D_k the spread of that entry between the restated run and the restated run from a start
perturbed by relative 1e-12: the margin of 100 covers the difference in summation order and in the factor's rounding, which the
single perturbed run does not sample.  Recorded on an MI355X (worst relative D_k of the input, the device's worst ratio to the
tolerance):
    c3_40  TLS 4.2e-12, 1.0e-4    GM 4.2e-09, 1.2e-2        c2_40  TLS 9.0e-12, 2.5e-5    GM 1.4e-11, 1.6e-5
    c3_24  TLS 4.7e-12, 2.1e-5    GM 3.5e-12, 9.1e-6        c3_150 TLS 1.4e-12, 1.8e-5
Within a level F_mu does not increase, from the device's own log, up to m u sum |terms|.  The final point is held as
tests/test_gpu_polish.py holds its own: the final weights are the restatement's, so the restated gradient of the final
weighted problem at the device's point is <= 2 rel_tol hmax and the distance to the restatement's point within
2 (|g_dev| + |g_ref|) / lambda_min.  Nothing comes from the code under test.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gnc_inputs as gi  # noqa: E402
import gnc_restatement as gr  # noqa: E402
import newton_restatement as nr  # noqa: E402
import robust_inputs as ri  # noqa: E402
import robust_restatement as rr  # noqa: E402
import test_gpu_polish as tpol  # noqa: E402  (device_free_bytes; none of its tests is imported)

import dpgo_amd  # noqa: E402

pytestmark = pytest.mark.gpu

U = gr.U
REL_TOL = 1e-9
RUNS = [(n, k) for n in ("c3_40", "c2_40", "c3_24") for k in (gr.TLS, gr.GM)] + [("c3_150", gr.TLS)]
FIELDS = ("outcome", "levels", "steps", "factorisations", "inner_outcome", "mu_initial", "mu_final", "s_max_initial", "F_initial",
          "F_weighted_final", "F_surrogate_final", "num_robust", "num_zero", "num_one", "num_between", "num_outliers", "device_bytes")

_obj = {}


def objects(name, out_frac=0.3):
    if (name, out_frac) not in _obj:
        P, X, outlier = gi.case(name, out_frac)
        G = ri.graph(P)
        _obj[(name, out_frac)] = (P, X, outlier, G, ri.group(G))
    return _obj[(name, out_frac)]


def options(kind, **kw):
    return dpgo_amd.GncOptions(kind=kind, barc2=gi.C2, mu_step=gi.MU_STEP, **kw)


@pytest.mark.parametrize("name,kind", RUNS)
def test_run_against_the_restatement(name, kind):
    P, X, outlier, G, grp = objects(name)
    want = gi.reference(name, kind)
    d, N, m, R = P["d"], P["N"], len(P["I"]), P["inter"]
    Xd, w, res, log = grp.gnc(G, X, options(kind))
    print("%s kind %d: %s, %d levels, %d steps, %d factorisations (restated %d, %d); total %.1f ms, edge passes %.1f ms, inner %.1f ms"
          % (name, kind, dpgo_amd.GNC_NAMES[res.outcome], res.levels, res.steps, res.factorisations, want["steps"], want["factorisations"],
             res.total_ms, res.edge_ms, res.inner_ms))
    assert (res.outcome, res.levels, res.num_outliers) == (want["outcome"], want["levels"], want["num_outliers"]) and len(log) == res.levels
    assert np.array_equal(log[:, 7:], want["log"][:, 7:])
    assert np.array_equal(w == 0, want["w"] == 0) and np.all(w[~R] == 1.0)
    assert np.array_equal((w == 0) if kind == gr.TLS else ((gr.edge_s(P, Xd) > gi.C2) & R), outlier)
    assert res.num_robust == R.sum() and (res.num_zero, res.num_one, res.num_between) == \
        (int(np.sum(w[R] == 0)), int(np.sum(w[R] == 1)), int(np.sum((w[R] > 0) & (w[R] < 1))))
    assert res.inner_outcome == dpgo_amd.POLISH_CONVERGED and np.all(log[:, 6] == dpgo_amd.POLISH_CONVERGED)
    assert res.steps >= log[:, 5].sum() and res.F_weighted_final == log[-1, 3] and res.F_surrogate_final == log[-1, 4]
    assert res.mu_final == log[-1, 0] and res.mu_initial == log[0, 0] and want["same_counts"]
    assert np.all(np.abs(log[:, 0] - want["log"][:, 0]) <= 1e-9 * want["log"][:, 0])
    # F_w and F_mu of every level
    tol = np.maximum(100.0 * want["spread"], 1e-10 * np.abs(want["log"][:, 1:5]))
    ratio = np.abs(log[:, 1:5] - want["log"][:, 1:5]) / tol
    print("    worst relative D_k %.3g; the device's worst |dF| / tolerance %.3g" %
          (np.max(want["spread"] / np.abs(want["log"][:, 1:5])), ratio.max()))
    assert np.all(ratio <= 1.0), ratio.max()
    # within a level the surrogate does not increase (every term of F is non-negative: sum |terms| = 2 F)
    assert np.all(log[:, 4] <= log[:, 1] + m * U * 2.0 * (log[:, 1] + log[:, 4]))
    # a second call: the same bits; the anchor's record is X's
    Xd2, w2, res2, log2 = grp.gnc(G, X, options(kind))
    assert np.array_equal(Xd, Xd2) and np.array_equal(w, w2) and np.array_equal(log, log2)
    assert all(getattr(res, f) == getattr(res2, f) for f in FIELDS)
    assert np.array_equal(Xd[0], X[0]) and np.array_equal(Xd[N:N + d], X[N:N + d])
    # the final point: a critical point of the restatement's final weighted problem
    M = rr.weighted_matrix(P, want["w"])
    H = nr.anchored_hessian(M, want["X"], d, 0)
    hmax, lam_min = nr.hmax_of(H, 0, d + d * (d - 1) // 2), float(np.linalg.eigvalsh(H)[0])
    g_dev, g_ref = (float(np.linalg.norm(nr.grad(M, Z, d, 0))) for Z in (Xd, want["X"]))
    dist, bound = float(np.linalg.norm(Xd - want["X"])), 2.0 * (g_dev + g_ref) / lam_min
    print("    restated |g(X_dev)| %.3g (2 rel_tol hmax = %.3g), |X_dev - X_ref| %.3g (bound %.3g)" % (g_dev, 2 * REL_TOL * hmax, dist, bound))
    assert lam_min > 0 and g_dev <= 2.0 * REL_TOL * hmax and dist <= bound
    # the final weights are the restatement's: to the bit under TLS (0 or 1); under GM a smooth function of s at the point before,
    # which the device knows as well as it knows the final one: |dw/ds| |grad s_e| (twice the distance bound), |dw/ds| =
    # 2 w / (s + delta), |grad s_e| = 2 |M_e X|_F, plus the rounding of the formula (36 u w)
    if kind == gr.TLS:
        assert np.array_equal(w, want["w"])
    else:
        s_ref = gr.edge_s(P, want["X"])
        grad_s = 2.0 * np.sqrt(np.sum(rr.edge_rows(P, want["X"]) ** 2, axis=(1, 2, 3)))
        tol_w = 2.0 * want["w"] / (s_ref + want["mu_final"] * gi.C2) * grad_s * 2.0 * bound + 36 * U * want["w"]
        print("    GM weights: worst |dw| %.3g, worst |dw| / tolerance %.3g" % (np.abs(w - want["w"]).max(), np.max(np.abs(w - want["w"])[R] / tol_w[R])))
        assert np.all(np.abs(w - want["w"]) <= tol_w)


def test_all_inliers_is_the_polish():
    """out_frac = 0: ALL_INLIERS at level 0 under TLS, and X0 is the point NodeGroup.polish gives, held as that test holds it."""
    P, X, outlier, G, grp = objects("c3_40", 0.0)
    d = P["d"]
    Xd, w, res, log = grp.gnc(G, X, options(gr.TLS))
    assert not outlier.any() and res.outcome == dpgo_amd.GNC_ALL_INLIERS and res.levels == 0 and len(log) == 0 and np.all(w == 1.0)
    assert 2 * res.s_max_initial <= gi.C2 and res.num_outliers == 0 and res.inner_outcome == dpgo_amd.POLISH_CONVERGED
    Xp, pres, _ = grp.polish(X)
    assert pres.outcome == dpgo_amd.POLISH_CONVERGED and abs(res.F_initial - pres.F_initial) <= 1e-12 * pres.F_initial
    M = rr.weighted_matrix(P, np.ones(len(P["I"])))
    H = nr.anchored_hessian(M, Xp, d, 0)
    hmax, lam_min = nr.hmax_of(H, 0, d + d * (d - 1) // 2), float(np.linalg.eigvalsh(H)[0])
    g0, gp = (float(np.linalg.norm(nr.grad(M, Z, d, 0))) for Z in (Xd, Xp))
    assert lam_min > 0 and g0 <= 2.0 * REL_TOL * hmax and np.linalg.norm(Xd - Xp) <= 2.0 * (g0 + gp) / lam_min
    assert abs(res.F_weighted_final - pres.F_final) <= 1e-12 * pres.F_final


def test_max_levels_and_an_empty_robust_set():
    P, X, _, G, grp = objects("c2_40")
    want = gi.reference("c2_40", gr.TLS)
    Xd, w, res, log = grp.gnc(G, X, options(gr.TLS, max_levels=3))
    assert res.outcome == dpgo_amd.GNC_MAX_LEVELS and res.levels == 3 and len(log) == 3
    assert np.array_equal(log[:, 7:], want["log"][:3, 7:])
    for kind in (gr.TLS, gr.GM):
        Xd, w, res, log = grp.gnc(G, X, options(kind), robust_set=np.zeros(len(P["I"]), np.int32))
        assert res.outcome == dpgo_amd.GNC_ALL_INLIERS and res.levels == 0 and res.num_robust == 0 and np.all(w == 1.0)


def test_an_inner_stall_is_an_outcome():
    """max_tries = 1: the Hessian at the start is indefinite (the outliers), the one factorisation at mu = 0 fails and the level-0
    solve stalls -- INNER_FAILED with X itself and unit weights, as the restatement says, not an error."""
    P, X, _, G, grp = objects("c2_40")
    want = gr.run(P, X, gr.TLS, gi.C2, mu_step=gi.MU_STEP, max_tries=1)
    assert want["outcome"] == gr.INNER_FAILED and want["levels"] == 0 and want["inner"] == [nr.STALLED]
    Xd, w, res, log = grp.gnc(G, X, options(gr.TLS, max_tries=1))
    assert res.outcome == dpgo_amd.GNC_INNER_FAILED and res.levels == 0 and res.inner_outcome == dpgo_amd.POLISH_STALLED and len(log) == 0
    assert np.array_equal(Xd, X) and np.all(w == 1.0) and res.steps == 0 and res.factorisations == 1


def test_a_given_robust_set_on_a_one_node_graph():
    """robust_set lets a graph without inter-node edges use the feature: the chain on ONE node with its closures as the robust
    set rejects exactly the injected outliers, level by level as the restatement does."""
    P4, X, outlier = gi.case("c2_40")
    P = rr.problem(P4["d"], P4["N"], P4["I"], P4["J"], P4["R"], P4["t"], P4["kappa"], P4["tau"], 1)
    R = np.arange(len(P["I"])) >= P["N"] - 1
    assert not P["inter"].any()
    want = gr.run(P, X, gr.TLS, gi.C2, R=R, mu_step=gi.MU_STEP)
    G = ri.graph(P)
    Xd, w, res, log = ri.group(G).gnc(G, X, options(gr.TLS), robust_set=R.astype(np.int32))
    assert (res.outcome, res.levels, res.num_robust) == (want["outcome"], want["levels"], int(R.sum())) and res.outcome == dpgo_amd.GNC_CONVERGED
    assert np.array_equal(log[:, 7:], want["log"][:, 7:]) and np.array_equal(w, want["w"]) and np.array_equal(w == 0, outlier)


def test_skipped_allocates_nothing():
    P, X, _, G, _ = objects("c3_24")
    grp = ri.group(G)
    grp.gnc(G, X, options(gr.TLS), max_bytes=1)   # (the certificate's buffers and M's values come here)
    free0 = tpol.device_free_bytes()
    Xo, w, res, log = grp.gnc(G, X, options(gr.TLS), max_bytes=1)
    assert tpol.device_free_bytes() == free0
    assert res.outcome == dpgo_amd.GNC_SKIPPED and np.array_equal(Xo, X) and len(log) == 0 and res.levels == 0 and res.steps == 0
    robust = grp.robust_polish(X, 0, max_bytes=1, graph=G)[1]
    assert res.device_bytes > robust.device_bytes > 1            # the arrays of the edge pass are counted in
    assert grp.gnc(G, X, options(gr.TLS), max_bytes=res.device_bytes - 1)[2].outcome == dpgo_amd.GNC_SKIPPED
    ok = grp.gnc(G, X, options(gr.TLS), max_bytes=res.device_bytes)[2]
    assert ok.outcome == dpgo_amd.GNC_CONVERGED and ok.device_bytes == res.device_bytes


def test_refusals():
    P, X, _, G, grp = objects("c2_40")
    for bad in (dict(kind=2), dict(kind=-1), dict(barc2=0.0), dict(barc2=float("nan")), dict(barc2=float("inf")), dict(mu_step=1.0),
                dict(mu_step=0.5), dict(max_levels=0), dict(max_tries=0), dict(anchor=P["N"])):
        kw = dict(kind=0, barc2=gi.C2)
        kw.update(bad)
        with pytest.raises(RuntimeError):
            grp.gnc(G, X, dpgo_amd.GncOptions(**kw))
    with pytest.raises(RuntimeError):
        ri.group(G, loss=1).gnc(G, X, options(gr.TLS))                          # a group created with a robust loss
    with pytest.raises(RuntimeError):
        grp.gnc(objects("c3_24")[3], X, options(gr.TLS))                        # another graph


def test_the_verdict_reaches_the_certificate():
    """Graph.scale_edges(weights) of the TLS result, a new group, verify at GNC's point: it runs (no verdict is asserted)."""
    P, X, _, G, grp = objects("c2_40")
    Xd, w, res, _ = grp.gnc(G, X, options(gr.TLS))
    Gw = G.scale_edges(w)
    cert, _, fac = ri.group(Gw).verify(Xd)
    print("verify on the re-weighted graph: status %d, stationarity %.3g" % (cert.status, cert.stationarity))
    assert np.isfinite(cert.stationarity) and np.isfinite(cert.theta)


# ---------------------------------------------------------------------------------------------------------------
# the facade and the driver
# ---------------------------------------------------------------------------------------------------------------
_py = {}


def python_run(fixtures_dir):
    """What the driver and the facade example do, through Python: chordal point, 20 trivial-loss AMM-PGO# iterations on 2 nodes,
    GNC-TLS with barc2 = 4 on a trivial-loss group of the same graph."""
    if not _py:
        G = dpgo_amd.read_g2o(os.path.join(fixtures_dir, "smallGrid3D.g2o"), 2)
        drv = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(0, True))
        for _ in range(20):
            assert drv.step() == 0
        _py["v"] = (G,) + ri.group(G).gnc(G, drv.X(), dpgo_amd.GncOptions(barc2=4.0))
        assert _py["v"][3].outcome != dpgo_amd.GNC_SKIPPED
    return _py["v"]


def test_cpp_facade_gnc(fixtures_dir):
    exe = os.path.join(ri.ROOT, "dpgo_amd", "facade_mm")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    args = [exe, os.path.join(fixtures_dir, "smallGrid3D.g2o"), "2", "20", "trivial", "1"]
    plain = subprocess.run(args, check=True, capture_output=True, text=True, timeout=300)
    out = subprocess.run(args + ["gnc"], check=True, capture_output=True, text=True, timeout=300)
    assert out.stdout == plain.stdout and "gnc" not in plain.stderr
    lines = [l[len("gnc: "):].split() for l in out.stderr.splitlines() if l.startswith("gnc: ")]
    G, Xp, w, res, _ = python_run(fixtures_dir)
    last = lines[-1]
    assert last[0] == dpgo_amd.GNC_NAMES[res.outcome]
    assert [int(v) for v in last[1:6]] == [res.levels, res.steps, res.factorisations, res.num_zero, res.num_outliers]
    assert [float(v) for v in last[6:9]] == [res.F_initial, res.F_weighted_final, res.F_surrogate_final]
    assert np.array_equal(np.array([float(l[2]) for l in lines if l[0] == "w"]), w)
    assert np.array_equal(np.array([[float(v) for v in l[2:]] for l in lines if l[0] == "x"]), Xp)


def test_dist_pgo_gnc_flags(fixtures_dir, tmp_path):
    """--gnc adds one line after the summary, writes its report and the filtered graph, and --polish behind it acts on its
    point; without the flag every output is as before."""
    exe = os.path.join(ri.ROOT, "dpgo_amd", "dist_pgo")
    base = [exe, "--dataset", os.path.join(fixtures_dir, "smallGrid3D.g2o"), "--num_nodes", "2", "--iters", "20", "--dist_init", "false",
            "--save", "false", "--loss", "trivial", "--polish"]
    rep, flt = tmp_path / "gnc.txt", tmp_path / "kept.g2o"
    plain = subprocess.run(base, capture_output=True, text=True, cwd=tmp_path, timeout=300)
    run = subprocess.run(base + ["--gnc", "tls", "--gnc_barc2", "4", "--gnc_report", str(rep), "--gnc_filtered", str(flt)],
                         capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert plain.returncode == 0 and run.returncode == 0, run.stderr[-2000:]
    assert "gnc" not in plain.stdout

    def steady(text):
        return [l for l in text.splitlines() if not l.startswith(("time: ", "gnc: ", "polish: "))]

    assert steady(plain.stdout) == steady(run.stdout)
    G, Xp, w, res, _ = python_run(fixtures_dir)
    line = [l for l in run.stdout.splitlines() if l.startswith("gnc: ")]
    assert len(line) == 1
    f = line[0][len("gnc: "):].split()
    assert f[0] == dpgo_amd.GNC_NAMES[res.outcome]
    assert [int(v) for v in f[1:8]] == [res.levels, res.steps, res.factorisations, res.num_robust, res.num_zero, res.num_between, res.num_outliers]
    assert [float(v) for v in f[8:13]] == [res.mu_initial, res.mu_final, res.F_initial, res.F_weighted_final, res.F_surrogate_final]
    got = np.loadtxt(rep)
    I, J = G.edges()[:2]
    s = np.add(*dpgo_amd.EdgeEval(G).run(Xp)[:2])
    assert got.shape == (G.num_edges, 5) and np.array_equal(got[:, 0], I) and np.array_equal(got[:, 1], J)
    assert np.array_equal(got[:, 3], w) and np.array_equal(got[:, 4], s) and got[:, 2].sum() == res.num_robust
    kept = dpgo_amd.read_g2o(str(flt), 2)
    assert kept.num_edges == int(np.sum(w != 0)) and kept.num_poses == G.num_poses
    # the polish behind it starts at GNC's point
    pol = [l for l in run.stdout.splitlines() if l.startswith("polish: ")][0].split()
    assert pol[1] == "CONVERGED" and float(pol[5]) == ri.group(G).polish(Xp)[1].F_initial
    bad = subprocess.run(base + ["--gnc", "huber"], capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert bad.returncode != 0 and "--gnc takes tls or gm" in bad.stderr
