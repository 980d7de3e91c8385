"""Graduated non-convexity on the maximum-likelihood objective on the device (Group::ml_gnc: one polish_loop per level under
the hooks of ml_gnc.cpp) against the committed restated runs (tests/golden/ml_gnc_reference.npz, made on the CPU by
tests/golden/make_ml_gnc_reference.py from tests/ml_gnc_restatement.run), held as tests/test_gpu_gnc.py holds its own.

Held exactly: outcome, levels and the count columns of every level; the inner steps and outcomes where the committed run says
its perturbed twin took the same ones (same_steps); {w == 0}, num_outliers, num_robust; the final weights bitwise under TLS.
mu within 1e-9 relative.  The four F columns within max(100 D_k, 1e-10 |F|), D_k the committed spread against the run from
X (1 + 1e-12 xi); the factor 100 is tests/test_gpu_gnc.py's own margin.  F_mu does not increase within a level, from the
device's own log.  The final point is held as tests/test_gpu_ml_polish.py holds its own, on the restatement's final weights;
GM's final weights within |dw/dchi2| |grad chi2_e| (twice the distance bound) + 36 u w.  Nothing comes from the device.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gnc_restatement as gr  # noqa: E402
import ml_gnc_inputs as mgi  # noqa: E402
import ml_gnc_restatement as mgr  # noqa: E402
import ml_restatement as mr  # noqa: E402
import newton_restatement as nr  # noqa: E402
import test_gpu_ml_ops as ops  # noqa: E402  (its groups; none of its tests is imported)
import test_gpu_polish as tgp  # noqa: E402  (device_free_bytes; none of its tests is imported)
import test_ml_host as tmh  # noqa: E402

import dpgo_amd  # noqa: E402
from oracle.problem import LOSS_NONE  # noqa: E402

pytestmark = pytest.mark.gpu

U = gr.U
REL_TOL = 1e-9
FIELDS = ("outcome", "levels", "steps", "factorisations", "inner_outcome", "mu_initial", "mu_final", "s_max_initial", "F_initial",
          "F_weighted_final", "F_surrogate_final", "num_robust", "num_zero", "num_one", "num_between", "num_outliers", "device_bytes",
          "near_pi", "near_pi_all")
_obj = {}


def objects(name):
    if name not in _obj:
        E, X, R, outlier, rs = mgi.case(name)
        grp = ops.group_of(E, E["nn"])
        _obj[name] = (E, X, R, outlier, rs, grp.graph, grp)
    return _obj[name]


def options(d, kind, **kw):
    return dpgo_amd.GncOptions(kind=kind, barc2=mgi.C2[d], mu_step=mgi.MU_STEP, **kw)


@pytest.mark.parametrize("name,kind", mgi.RUNS)
def test_run_against_the_restatement(name, kind):
    E, X, R, outlier, rs, G, grp = objects(name)
    want = mgi.reference(name, kind)
    d, N, m = E["d"], E["N"], len(E["I"])
    c2 = mgi.C2[d]
    Xd, w, res, log = grp.ml_gnc(G, X, options(d, kind), robust_set=rs)
    print("%s kind %d: %s, %d levels, %d steps, %d factorisations (restated %d, %d); total %.1f ms, edge passes %.1f ms, inner %.1f ms"
          % (name, kind, dpgo_amd.GNC_NAMES[res.outcome], res.levels, res.steps, res.factorisations, want["steps"], want["factorisations"],
             res.total_ms, res.edge_ms, res.inner_ms))
    assert (res.outcome, res.levels, res.num_outliers) == (want["outcome"], want["levels"], want["num_outliers"]) and len(log) == res.levels
    assert np.array_equal(log[:, 7:], want["log"][:, 7:]) and want["same_counts"]
    if want["same_steps"]:
        assert np.array_equal(log[:, 5:7], want["log"][:, 5:7]) and res.inner_outcome == want["inner"][-1]
        assert res.steps == want["steps"] and res.factorisations == want["factorisations"]
    assert np.array_equal(w == 0, want["w"] == 0) and np.all(w[~R] == 1.0)
    chi2_dev = mgr.chi2_theta(E, Xd)[0]
    assert np.array_equal((w == 0) if kind == gr.TLS else ((chi2_dev > c2) & R), outlier)
    assert res.num_robust == R.sum() and (res.num_zero, res.num_one, res.num_between) == \
        (int(np.sum(w[R] == 0)), int(np.sum(w[R] == 1)), int(np.sum((w[R] > 0) & (w[R] < 1))))
    assert res.inner_outcome == dpgo_amd.POLISH_CONVERGED and not np.any(log[:, 6] == dpgo_amd.POLISH_STALLED)
    assert res.steps >= log[:, 5].sum() and res.F_weighted_final == log[-1, 3] and res.F_surrogate_final == log[-1, 4]
    assert res.mu_final == log[-1, 0] and res.mu_initial == log[0, 0] and (res.near_pi, res.near_pi_all) == (0, 0)
    assert abs(res.s_max_initial - want["s_max_initial"]) <= 1e-9 * want["s_max_initial"]
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
    Xd2, w2, res2, log2 = grp.ml_gnc(G, X, options(d, kind), robust_set=rs)
    assert np.array_equal(Xd, Xd2) and np.array_equal(w, w2) and np.array_equal(log, log2)
    assert all(getattr(res, f) == getattr(res2, f) for f in FIELDS)
    assert np.array_equal(Xd[0], X[0]) and np.array_equal(Xd[N:N + d], X[N:N + d])
    # the final point: a critical point of the restatement's final weighted problem
    Ew = mgr.scaled(E, want["w"])
    _, g_ref, H = mr.assemble(Ew, want["X"], 0)
    hmax, lam_min = nr.hmax_of(H, 0, mr.dof_of(d)), float(np.linalg.eigvalsh(0.5 * (H + H.T))[0])
    g_dev, g_ref = float(np.linalg.norm(mr.assemble(Ew, Xd, 0)[1])), float(np.linalg.norm(g_ref))
    dist, bound = float(np.linalg.norm(Xd - want["X"])), 2.0 * (g_dev + g_ref) / lam_min
    print("    restated |g_w(X_dev)| %.3g (2 rel_tol hmax = %.3g), |X_dev - X_ref| %.3g (bound %.3g)" % (g_dev, 2 * REL_TOL * hmax, dist, bound))
    assert lam_min > 0 and g_dev <= 2.0 * REL_TOL * hmax and dist <= bound
    if kind == gr.TLS:
        assert np.array_equal(w, want["w"])
    else:
        per = mr.edges_all(E, want["X"])
        grad_s = 2.0 * np.sqrt(np.sum(per["grad"] ** 2, axis=(1, 2)))
        tol_w = 2.0 * want["w"] / (per["chi2"] + want["mu_final"] * c2) * grad_s * 2.0 * bound + 36 * U * want["w"]
        print("    GM weights: worst |dw| %.3g, worst |dw| / tolerance %.3g" % (np.abs(w - want["w"]).max(), np.max(np.abs(w - want["w"])[R] / tol_w[R])))
        assert np.all(np.abs(w - want["w"]) <= tol_w)


def test_all_inliers_is_the_ml_polish():
    """No robust edge is an outlier (the inliers of the case alone): ALL_INLIERS at level 0 under TLS, and X0 is the point
    NodeGroup.ml_polish gives, held as that test holds it."""
    E, X, R, outlier, rs, G, grp = objects("m3_24")
    keep = ~outlier
    Ek = dict(E, **{k: E[k][keep] for k in ("I", "J", "R", "t", "kappa", "tau", "Om")})
    grp2 = ops.group_of(Ek, 1)
    d = E["d"]
    Xd, w, res, log = grp2.ml_gnc(grp2.graph, X, options(d, gr.TLS, max_steps=40), robust_set=R[keep].astype(np.int32))
    assert res.outcome == dpgo_amd.GNC_ALL_INLIERS and res.levels == 0 and len(log) == 0 and np.all(w == 1.0)
    assert 2 * res.s_max_initial <= mgi.C2[d] and res.num_outliers == 0 and res.inner_outcome == dpgo_amd.POLISH_CONVERGED
    Xp, pres, _ = grp2.ml_polish(X, max_steps=40)
    assert pres.outcome == dpgo_amd.POLISH_CONVERGED and abs(res.F_initial - pres.F_initial) <= 1e-12 * pres.F_initial
    _, gp, H = mr.assemble(Ek, Xp, 0)
    hmax, lam_min = nr.hmax_of(H, 0, mr.dof_of(d)), float(np.linalg.eigvalsh(0.5 * (H + H.T))[0])
    g0, gp = float(np.linalg.norm(mr.assemble(Ek, Xd, 0)[1])), float(np.linalg.norm(gp))
    assert lam_min > 0 and g0 <= 2.0 * REL_TOL * hmax and np.linalg.norm(Xd - Xp) <= 2.0 * (g0 + gp) / lam_min
    assert abs(res.F_weighted_final - pres.F_final) <= 1e-12 * pres.F_final and res.F_surrogate_final == res.F_weighted_final


def test_max_levels_and_an_empty_robust_set():
    E, X, R, _, rs, G, grp = objects("m2_40")
    want = mgi.reference("m2_40", gr.TLS)
    Xd, w, res, log = grp.ml_gnc(G, X, options(2, gr.TLS, max_levels=2), robust_set=rs)
    assert res.outcome == dpgo_amd.GNC_MAX_LEVELS and res.levels == 2 and len(log) == 2
    assert np.array_equal(log[:, 7:], want["log"][:2, 7:])
    for kind in (gr.TLS, gr.GM):
        Xd, w, res, log = grp.ml_gnc(G, X, options(2, kind), robust_set=np.zeros(len(R), np.int32))
        assert res.outcome == dpgo_amd.GNC_ALL_INLIERS and res.levels == 0 and res.num_robust == 0 and np.all(w == 1.0)
    # the inter-node rule on one node: no robust edge either
    Xd, w, res, log = grp.ml_gnc(G, X, options(2, gr.TLS))
    assert res.outcome == dpgo_amd.GNC_ALL_INLIERS and res.num_robust == 0


def test_a_rank_deficient_level_is_an_outcome():
    """ml_gnc_inputs.pendant: the two robust edges that hold the last pose are dropped at the same level, whose H_w then has a
    zero block.  With the default tries the Levenberg-Marquardt shift copes; with max_tries = 1 the one factorisation at mu = 0
    meets the zero pivot and the level's solve stalls: INNER_FAILED with X_{k-1} and the weights it was solved with, as the
    restatement says, not an error."""
    E, X, R = mgi.pendant()
    d, N, m = E["d"], E["N"], len(E["I"])
    want = mgr.run(E, X, gr.TLS, mgi.C2[d], R, mu_step=mgi.MU_STEP, max_tries=1)
    assert want["outcome"] == gr.INNER_FAILED and want["levels"] >= 2 and want["inner"][-1] == nr.STALLED
    assert np.all(want["w"][-2:] > 0)                      # (the weights returned are the level before's: the pose still hangs)
    grp = ops.group_of(E, 1)
    G = grp.graph
    Xd, w, res, log = grp.ml_gnc(G, X, options(d, gr.TLS, max_tries=1), robust_set=R.astype(np.int32))
    assert res.outcome == dpgo_amd.GNC_INNER_FAILED and res.levels == want["levels"] and res.inner_outcome == dpgo_amd.POLISH_STALLED
    assert len(log) == res.levels and log[-1, 6] == dpgo_amd.POLISH_STALLED and log[-1, 5] == 0
    assert log[-1, 7] == np.sum(want["w"] == 0) + 2       # the failing level's weights had both edges at zero
    assert np.array_equal(log[:-1, 5:], want["log"][:, 5:])
    # X_{k-1} is the converged point of the restatement's weighted problem of the level before: held by the distance bound of
    # test_run_against_the_restatement on those weights.  Its weights are weight_mu(chi2) at the point before it, at the level
    # before's mu: 0 and 1 exactly where the restatement has them; between, within |dw/dchi2| |grad chi2_e| (twice the distance
    # bound) + w_bound, |dw/dchi2| = (w + mu) / (2 chi2) under TLS (gnc_restatement's docstring), as that test holds GM's.
    assert want["inner"][-2] == nr.CONVERGED
    Ew = mgr.scaled(E, want["w"])
    _, g_ref, H = mr.assemble(Ew, want["X"], 0)
    hmax, lam_min = nr.hmax_of(H, 0, mr.dof_of(d)), float(np.linalg.eigvalsh(0.5 * (H + H.T))[0])
    g_dev, g_ref = float(np.linalg.norm(mr.assemble(Ew, Xd, 0)[1])), float(np.linalg.norm(g_ref))
    dist, bound = float(np.linalg.norm(Xd - want["X"])), 2.0 * (g_dev + g_ref) / lam_min
    print("    restated |g_w(X_dev)| %.3g (2 rel_tol hmax = %.3g), |X_dev - X_ref| %.3g (bound %.3g)" % (g_dev, 2 * REL_TOL * hmax, dist, bound))
    assert lam_min > 0 and g_dev <= 2.0 * REL_TOL * hmax and dist <= bound
    mu_prev = float(want["log"][-1, 0])
    per = mr.edges_all(E, want["X"])
    grad_s = 2.0 * np.sqrt(np.sum(per["grad"] ** 2, axis=(1, 2)))
    mid = (want["w"] > 0) & (want["w"] < 1)
    tol_w = (want["w"] + mu_prev) / (2.0 * np.where(mid, per["chi2"], 1.0)) * grad_s * 2.0 * bound + gr.w_bound(gr.TLS, mu_prev, want["w"])
    assert np.array_equal(w == 0, want["w"] == 0) and np.array_equal(w == 1, want["w"] == 1) and mid.any()
    print("    the weights between 0 and 1: worst |dw| %.3g, worst |dw| / tolerance %.3g" %
          (np.abs(w - want["w"])[mid].max(), np.max(np.abs(w - want["w"])[mid] / tol_w[mid])))
    assert np.all(np.abs(w - want["w"])[mid] <= tol_w[mid])
    assert (res.num_zero, res.num_between) == (int(np.sum(w[R] == 0)), int(np.sum((w[R] > 0) & (w[R] < 1))))
    ok = grp.ml_gnc(G, X, options(d, gr.TLS), robust_set=R.astype(np.int32))
    assert ok[2].outcome == dpgo_amd.GNC_CONVERGED and np.all(ok[1][-2:] == 0) and np.all(np.isfinite(ok[0]))


def test_a_level_zero_stall_is_evaluated():
    """test_ml_gnc_host.LEVEL0_STALL: with max_tries = 1 the unit-weight solve stalls before any level.  INNER_FAILED at level 0
    with X itself and unit weights, the counts of the restatement -- and, unlike NodeGroup.gnc, with the sums, the counts and
    near_pi of one FULL pass at (X, w = 1, mu = 1): the bits of ml_gnc_eval there, which is the same kernel at the same point."""
    E, X, R, _, rs, G, grp = objects("m2_40")
    d, m = E["d"], len(E["I"])
    c2 = mgi.C2[d]
    want = mgr.run(E, X, gr.TLS, c2, R, mu_step=mgi.MU_STEP, max_tries=1)
    assert want["outcome"] == gr.INNER_FAILED and want["levels"] == 0 and want["inner"] == [nr.STALLED]
    Xd, w, res, log = grp.ml_gnc(G, X, options(d, gr.TLS, max_tries=1), robust_set=rs)
    chi2, _, sums = grp.ml_gnc_eval(G, X, gr.TLS, 1.0, c2, robust_set=rs, w_in=np.ones(m))
    print("level-0 stall: %s, level %d, inner %d, %d steps, %d factorisations (restated %d, %d); F_w %.17g (eval %.17g), "
          "outliers %d (eval %d), near_pi %d / %d (eval %d / %d)"
          % (dpgo_amd.GNC_NAMES[res.outcome], res.levels, res.inner_outcome, res.steps, res.factorisations, want["steps"],
             want["factorisations"], res.F_weighted_final, 0.5 * (sums[0] + sums[1]), res.num_outliers, int(np.sum(R & (chi2 > c2))),
             res.near_pi, res.near_pi_all, int(sums[8]), int(sums[9])))
    assert res.outcome == dpgo_amd.GNC_INNER_FAILED and res.levels == 0 and res.inner_outcome == dpgo_amd.POLISH_STALLED
    assert len(log) == 0 and np.array_equal(Xd, X) and np.all(w == 1.0)
    assert (res.steps, res.factorisations) == (want["steps"], want["factorisations"])
    assert res.num_robust == R.sum() and res.num_one == res.num_robust and (res.num_zero, res.num_between) == (0, 0)
    assert res.near_pi == res.near_pi_all and (res.near_pi, res.near_pi_all) == (int(sums[8]), int(sums[9]))
    assert res.F_weighted_final == 0.5 * (sums[0] + sums[1])
    assert res.num_outliers == int(np.sum(R & (chi2 > c2)))


def test_skipped_allocates_nothing():
    E, X, R, _, rs, G, _ = objects("m3_24")
    grp = ops.group_of(E, 1)
    G = grp.graph
    d = E["d"]
    grp.ml_gnc(G, X, options(d, gr.TLS), robust_set=rs, max_bytes=1)   # (the certificate's buffers come here)
    free0 = tgp.device_free_bytes()
    Xo, w, res, log = grp.ml_gnc(G, X, options(d, gr.TLS), robust_set=rs, max_bytes=1)
    assert tgp.device_free_bytes() == free0
    assert res.outcome == dpgo_amd.GNC_SKIPPED and np.array_equal(Xo, X) and len(log) == 0 and res.levels == 0 and res.steps == 0
    plain = grp.ml_polish(X, max_bytes=1)[1]
    assert res.device_bytes > plain.device_bytes > 1            # the weights, the robust set and the partials are counted in
    assert grp.ml_gnc(G, X, options(d, gr.TLS), robust_set=rs, max_bytes=res.device_bytes - 1)[2].outcome == dpgo_amd.GNC_SKIPPED
    ok = grp.ml_gnc(G, X, options(d, gr.TLS), robust_set=rs, max_bytes=res.device_bytes)[2]
    assert ok.outcome == dpgo_amd.GNC_CONVERGED and ok.device_bytes == res.device_bytes


def test_refusals():
    E, X, R, _, rs, G, grp = objects("m2_40")
    for bad in (dict(kind=2), dict(kind=-1), dict(barc2=0.0), dict(barc2=float("nan")), dict(barc2=float("inf")), dict(mu_step=1.0),
                dict(mu_step=0.5), dict(max_levels=0), dict(max_tries=0), dict(anchor=E["N"]), dict(anchor=-1)):
        kw = dict(kind=0, barc2=mgi.C2[2])
        kw.update(bad)
        with pytest.raises(RuntimeError):
            grp.ml_gnc(G, X, dpgo_amd.GncOptions(**kw), robust_set=rs)
    hub = dpgo_amd.NodeGroup(G, range(1), dpgo_amd.Options.driver(dpgo_amd.LOSS_HUBER, True, max_iterations=0))
    E3, X3 = objects("m3_40x3")[:2]
    G3 = objects("m3_40x3")[5]
    part = dpgo_amd.NodeGroup(G3, [0], dpgo_amd.Options.driver(LOSS_NONE, True, max_iterations=0))
    bad = E["Om"].copy()
    bad[11, 1, 1] = -1.0
    notspd = tmh.graph_of(dict(E, Om=bad), 1)
    for g, graph, x in ((hub, G, X), (part, G3, X3), (grp, objects("m3_24")[5], X), (grp, notspd, X)):
        with pytest.raises(RuntimeError):
            g.ml_gnc(graph, x, options(2, gr.TLS))
        with pytest.raises(RuntimeError):
            g.ml_gnc_eval(graph, x, gr.TLS, 1.0, 1.0)
    for kw in (dict(kind=2, mu=1.0, barc2=1.0), dict(kind=0, mu=0.0, barc2=1.0), dict(kind=0, mu=1.0, barc2=-1.0)):
        with pytest.raises(RuntimeError):
            grp.ml_gnc_eval(G, X, **kw)
    with pytest.raises(ValueError):
        grp.ml_gnc(G, X, options(2, gr.TLS), robust_set=rs[:-1])


def test_ml_gnc_does_not_disturb_the_optimiser():
    """20 AMM-PGO# iterations with the two calls on the iterating group after every fifth: bit for bit the run without."""
    E, X, R, _, rs, _, _ = objects("m3_40x3")
    runs = []
    for with_gnc in (False, True):
        G = tmh.graph_of(E, 3)
        drv = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(LOSS_NONE, True))
        trace = []
        for it in range(20):
            assert drv.step() == 0
            if with_gnc and it % 5 == 4:
                Z = drv.X()
                assert drv.group.ml_gnc(G, Z, options(3, gr.TLS, max_levels=2, max_steps=3))[2].levels == 2
                drv.group.ml_gnc_eval(G, Z, gr.GM, 2.0, mgi.C2[3])
            trace.append([getattr(drv.group.results(a), f) for a in range(3) for f in ("fobj", "gamma", "gradFnorm", "Gk")])
        runs.append((np.array(drv.X()), np.array(trace)))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


# ---------------------------------------------------------------------------------------------------------------
# the facade and the driver
# ---------------------------------------------------------------------------------------------------------------
_py = {}
# smallGrid3D has no gross outlier: at the 0.999 quantile the call ends ALL_INLIERS at level 0 (max_R chi2 = 7.94 at the ML point)
# and nothing behind it would run on a filtered graph.  At barc2 = 5 the restatement (CPU, from the chordal point) takes 9
# levels and rejects 12 of the 30 inter-node edges, no chi2 closer than 8e-3 relative to a threshold, and the graph without them
# is connected with lambda_min(H) = 0.076: the levels, the zero weights, the filter and the covariance all run.
BARC2 = 5.0


def python_run(fixtures_dir):
    """What the driver does, through Python: chordal point, 20 AMM-PGO# iterations on 2 nodes, the polish, the refinement on the
    file's own information matrices and, from its point, GNC-TLS on chi2 on the group that iterated; and what the facade
    example does: GNC-TLS from the iterations' point on a second, trivial-loss group."""
    if not _py:
        G = dpgo_amd.read_g2o(os.path.join(fixtures_dir, "smallGrid3D.g2o"), 2)
        drv = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(LOSS_NONE, True))
        for _ in range(20):
            assert drv.step() == 0
        X = drv.X()
        post = dpgo_amd.NodeGroup(G, range(2), dpgo_amd.Options.driver(LOSS_NONE, True, max_iterations=0))
        _py["facade"] = post.ml_gnc(G, X, dpgo_amd.GncOptions(barc2=BARC2))
        Xm = drv.group.ml_polish(drv.group.polish(X)[0])[0]
        Xg, w, res, _ = drv.group.ml_gnc(G, Xm, dpgo_amd.GncOptions(barc2=BARC2))
        assert res.outcome == dpgo_amd.GNC_CONVERGED and res.levels >= 1 and np.any(w == 0) and 0 < np.sum(w > 0) < G.num_edges
        chi2 = drv.group.ml_gnc_eval(G, Xg, gr.TLS, res.mu_final, BARC2, w_in=w)[0]
        kept = G.filter_edges(w > 0)
        _py["driver"] = (G, Xg, w, res, chi2, drv.group.ml_covariance(Xg, graph=kept), drv.group.ml_eval(Xg, graph=kept))
        assert _py["driver"][5][2].outcome == dpgo_amd.COV_OK
        # (the covariance of the whole graph at that point is another matrix: the filter is not a no-op)
        assert not np.array_equal(drv.group.ml_covariance(Xg)[0], _py["driver"][5][0])
    return _py


def test_cpp_facade_ml_gnc(fixtures_dir):
    """examples/facade_mm.cpp with `ml_gnc tls 5`: DPGOHashGroup::ml_graduated_non_convexity on stderr; stdout the same
    trace as without; the weights, the point and the counts those of NodeGroup.ml_gnc bit for bit."""
    exe = os.path.join(tgp.ROOT, "dpgo_amd", "facade_mm")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    args = [exe, os.path.join(fixtures_dir, "smallGrid3D.g2o"), "2", "20", "trivial", "1"]
    plain = subprocess.run(args, check=True, capture_output=True, text=True, timeout=300)
    out = subprocess.run(args + ["ml_gnc", "tls", "%.17g" % BARC2], check=True, capture_output=True, text=True, timeout=300)
    assert out.stdout == plain.stdout and "ml gnc" not in plain.stderr
    lines = [l[len("ml gnc: "):].split() for l in out.stderr.splitlines() if l.startswith("ml gnc: ")]
    Xg, w, res, _ = python_run(fixtures_dir)["facade"]
    last = lines[-1]
    assert last[0] == dpgo_amd.GNC_NAMES[res.outcome] and res.outcome == dpgo_amd.GNC_CONVERGED
    assert res.levels >= 1 and np.any(w == 0) and np.any(w == 1)            # WEIGH levels ran, and edges were rejected
    assert [int(v) for v in last[1:6]] == [res.levels, res.steps, res.factorisations, res.num_zero, res.num_outliers]
    assert [float(v) for v in last[6:9]] == [res.F_initial, res.F_weighted_final, res.F_surrogate_final]
    assert [int(v) for v in last[9:11]] == [res.near_pi, res.near_pi_all]
    assert np.array_equal(np.array([float(l[2]) for l in lines if l[0] == "w"]), w)
    assert np.array_equal(np.array([[float(v) for v in l[2:]] for l in lines if l[0] == "x"]), Xg)


def test_dist_pgo_ml_gnc_flags(fixtures_dir, tmp_path):
    """--ml_gnc behind --ml_polish adds one line and puts its point into the result files; --ml_gnc_report holds the weights and
    chi2 at that point; --ml_covariance and --ml_report behind it are those of filter_edges(w > 0); all of it bit for bit the
    Python calls.  Without the flag stdout is what it was."""
    exe = os.path.join(tgp.ROOT, "dpgo_amd", "dist_pgo")
    base = [exe, "--dataset", os.path.join(fixtures_dir, "smallGrid3D.g2o"), "--num_nodes", "2", "--iters", "20", "--dist_init", "false",
            "--save", "false", "--polish", "--ml_polish"]
    plain = subprocess.run(base, capture_output=True, text=True, cwd=tmp_path, timeout=300)
    run = subprocess.run(base + ["--ml_gnc", "tls", "--ml_gnc_barc2", "%.17g" % BARC2, "--ml_gnc_report", "mlgnc.txt",
                                 "--ml_covariance", "mlcov.txt", "--ml_report", "chi2.txt"], capture_output=True, text=True, cwd=tmp_path,
                         timeout=300)
    assert plain.returncode == 0 and run.returncode == 0, run.stderr[-2000:]
    steady = lambda text: [l for l in text.splitlines() if not l.startswith(("time: ", "ml gnc: ", "ml covariance: "))]
    assert steady(plain.stdout) == steady(run.stdout) and "ml gnc" not in plain.stdout
    G, Xg, w, res, chi2, cov, ev = python_run(fixtures_dir)["driver"]
    f = [l for l in run.stdout.splitlines() if l.startswith("ml gnc: ")][0][len("ml gnc: "):].split()
    assert f[0] == dpgo_amd.GNC_NAMES[res.outcome]
    assert [int(v) for v in f[1:8]] == [res.levels, res.steps, res.factorisations, res.num_robust, res.num_zero, res.num_between, res.num_outliers]
    assert [float(v) for v in f[8:13]] == [res.mu_initial, res.mu_final, res.F_initial, res.F_weighted_final, res.F_surrogate_final]
    assert [int(v) for v in f[13:15]] == [res.near_pi, res.near_pi_all]
    rep = open(tmp_path / "mlgnc.txt").read().splitlines()
    head = rep[0].split()
    assert head[:3] == ["#", "ml_gnc", dpgo_amd.GNC_NAMES[res.outcome]] and float(head[4]) == BARC2 and int(head[6]) == G.num_edges
    assert [int(head[k]) for k in (8, 10, 12)] == [res.num_robust, res.num_zero, res.num_outliers]
    got = np.array([[float(v) for v in l.split()] for l in rep[1:]])
    I, J = G.edges()[:2]
    assert got.shape == (G.num_edges, 5) and np.array_equal(got[:, 0], I) and np.array_equal(got[:, 1], J)
    assert np.array_equal(got[:, 3], w) and np.array_equal(got[:, 4], chi2) and got[:, 2].sum() == res.num_robust
    # the covariance and the report of the inlier set
    keep = w > 0
    assert res.levels >= 1 and np.any(w == 0) and 0 < keep.sum() < G.num_edges and cov[2].outcome == dpgo_amd.COV_OK
    line = [l for l in run.stdout.splitlines() if l.startswith("ml covariance: ")][0].split()
    assert line[2] == "OK"
    mc = np.loadtxt(tmp_path / "mlcov.txt")
    iu = np.triu_indices(6)
    assert np.array_equal(mc[:, 0], np.arange(len(mc))) and np.array_equal(mc[:, 1:], np.array([m[iu] for m in cov[0]]))
    ch = open(tmp_path / "chi2.txt").read().splitlines()
    assert int(ch[0].split()[6]) == int(keep.sum()) and float(ch[0].split()[2]) == ev[0]
    assert [[int(v) for v in l.split()[:2]] for l in ch[1:]] == np.stack([I[keep], J[keep]], axis=1).tolist()
    assert np.array_equal(np.array([float(l.split()[2]) for l in ch[1:]]), ev[2])
    bad = subprocess.run(base + ["--ml_gnc", "huber"], capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert bad.returncode != 0 and "--ml_gnc takes tls or gm." in bad.stderr
