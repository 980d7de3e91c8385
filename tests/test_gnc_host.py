"""Graduated non-convexity without a GPU (dpgo_amd/csrc/gnc.h): the entry points, the kernel's weight arithmetic through its host
hook (dpgo_debug_gnc_weight_host compiles gnc_math.h, which k_gnc_edge compiles too) against the long-double restatement,
Black-Rangarajan duality, and the restated loop (tests/gnc_restatement.run) on the four inputs of tests/gnc_inputs.py.

Bounds (derived in tests/gnc_restatement.py): TLS |dw| <= 16 u (mu + 1), GM |dw| <= 36 u w, four times the first-order
constants 4 and 9.  Measured on the grid below: the float64 numpy restatement's worst ratio is 0.096 of the TLS bound and
0.118 of the GM bound (a quarter is allowed); the library's host hook gives the same two figures.

The restated runs reproduce tests/gnc_inputs.TABLE and the committed tests/golden/gnc_reference.npz, keep
F_mu(X_k) <= F_mu(X_{k-1}) within every level, keep every robust s_e(X_{k-1}) at least 1e-6 (relative) away from both TLS
thresholds at every level (smallest margin 2.3e-3), and give the same counts per level from a start perturbed by relative
1e-12.  D_k, the per-level spread of F between those two runs, is the sensitivity tests/test_gpu_gnc.py uses.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gnc_inputs as gi  # noqa: E402
import gnc_restatement as gr  # noqa: E402
import robust_inputs as ri  # noqa: E402

import dpgo_amd  # noqa: E402

LD = np.longdouble
NEW_SYMBOLS = ("dpgo_gnc_options_default", "dpgo_group_gnc", "dpgo_group_gnc_eval", "dpgo_debug_gnc_weight_host")
MUS = [1e-12, 1e-3, 1.0] + [1.4 ** k for k in range(1, 21)] + [1e12]
C2S = (4.0, 0.37)


def grid(mu, c2):
    """s on a log grid, both thresholds exactly and +- 1 ulp, s = 0."""
    lo, hi = gr.thresholds(mu, c2)
    edge = [f(t) for t in (lo, hi) for f in (lambda v: v, lambda v: np.nextafter(v, 0.0), lambda v: np.nextafter(v, np.inf))]
    between = np.exp(np.linspace(np.log(lo), np.log(hi), 41))[1:-1]
    return np.concatenate([[0.0], c2 * np.logspace(-14, 14, 113), edge, between])


def test_symbols_and_argument_checks():
    import ctypes as C
    L = dpgo_amd.lib()
    header = open(os.path.join(ri.ROOT, "include", "dpgo_amd.h")).read()
    for sym in NEW_SYMBOLS:
        assert sym + "(" in header and sym in dpgo_amd.SYMBOLS and hasattr(L, sym)
    o = dpgo_amd.GncOptions()
    assert (o.kind, o.barc2, o.mu_step, o.max_levels) == (dpgo_amd.GNC_TLS, 1.0, 1.4, 100)
    p = dpgo_amd.PolishOptions()
    assert all(getattr(o.inner, f) == getattr(p, f) for f, _ in dpgo_amd.PolishOptions._fields_)
    o = dpgo_amd.GncOptions(kind=dpgo_amd.GNC_GM, barc2=4.0, max_steps=7, anchor=3)
    assert (o.kind, o.barc2, o.inner.max_steps, o.inner.anchor) == (1, 4.0, 7, 3)
    with pytest.raises(TypeError):
        dpgo_amd.GncOptions(nonsense=1)
    s = np.array([0.0, 1.0, 5.0])
    for bad in (dict(kind=2), dict(kind=-1), dict(mu=0.0), dict(mu=float("nan")), dict(barc2=0.0), dict(barc2=-1.0),
                dict(barc2=float("inf")), dict(s=np.array([-1.0])), dict(s=np.array([float("nan")]))):
        kw = dict(kind=0, mu=1.0, barc2=4.0, s=s)
        kw.update(bad)
        with pytest.raises(ValueError):
            dpgo_amd.gnc_weight_debug(**kw)
    assert len(dpgo_amd.gnc_weight_debug(0, 1.0, 4.0, np.zeros(0))[0]) == 0
    # NULL handles and outputs: -1 before anything touches a device
    P, X, _ = gi.case("c2_40")
    G = ri.graph(P)
    Xf = np.asfortranarray(X)
    xp = Xf.ctypes.data_as(C.POINTER(C.c_double))
    w = np.ones(G.num_edges)
    wp = w.ctypes.data_as(C.POINTER(C.c_double))
    r = dpgo_amd.GncResult()
    assert L.dpgo_group_gnc(None, G._h, xp, Xf.shape[0], None, None, 0, xp, Xf.shape[0], wp, None, 0, C.byref(r)) == -1
    assert L.dpgo_group_gnc_eval(None, G._h, xp, Xf.shape[0], 0, 1.0, 4.0, None, None, wp, wp, wp, wp) == -1
    assert L.dpgo_debug_gnc_weight_host(0, 1.0, 4.0, None, 3, wp, wp) == -1
    assert L.dpgo_debug_gnc_weight_host(0, 1.0, 4.0, wp, -1, wp, wp) == -1


@pytest.mark.parametrize("kind", (gr.TLS, gr.GM))
def test_weight_against_the_long_double_restatement(kind):
    worst = {"library": 0.0, "float64 restatement": 0.0}
    slip_caught = False
    for c2 in C2S:
        for mu in MUS:
            s = grid(mu, c2)
            w_ref, rho_ref = gr.weight_rho(kind, mu, c2, s, LD)
            bound = gr.w_bound(kind, mu, w_ref)
            w_lib, rho_lib = dpgo_amd.gnc_weight_debug(kind, mu, c2, s)
            w_np, rho_np = gr.weight_rho(kind, mu, c2, s)
            for name, w in (("library", w_lib), ("float64 restatement", w_np)):
                err = np.abs(np.asarray(w, LD) - w_ref)
                assert np.all(err <= bound), (name, kind, mu, c2, float(np.max(err / np.maximum(bound, 1e-300))))
                live = bound > 0
                if live.any():
                    worst[name] = max(worst[name], float(np.max(err[live] / bound[live])))
            assert np.all((w_lib >= 0) & (w_lib <= 1))
            assert w_lib[0] == 1.0 and rho_lib[0] == 0.0                     # s = 0
            # rho: 12 roundings against the magnitudes of its terms (2 sqrt(a s) and mu (c2 + s) cancel for large mu)
            mag = np.asarray(2 * np.sqrt(LD(c2) * LD(mu) * (LD(mu) + 1) * np.asarray(s, LD)) + LD(mu) * (LD(c2) + np.asarray(s, LD)), np.float64) \
                if kind == gr.TLS else np.asarray(rho_ref, np.float64)
            assert np.all(np.abs(np.asarray(rho_lib, LD) - rho_ref) <= 12 * gr.U * np.maximum(mag, np.asarray(rho_ref, np.float64)))
            if kind == gr.TLS:
                w_slip = gr.weight_rho(kind, mu, c2, s, swap_thresholds=True)[0]
                slip_caught = slip_caught or bool(np.any(np.abs(np.asarray(w_slip, LD) - w_ref) > bound))
    print("kind %d: worst |dw| / bound: %s" % (kind, ", ".join("%s %.3g" % kv for kv in worst.items())))
    assert worst["float64 restatement"] <= 0.25
    assert kind == gr.GM or slip_caught                                      # mu/(mu+1) and (mu+1)/mu swapped is caught


@pytest.mark.parametrize("kind", (gr.TLS, gr.GM))
def test_black_rangarajan_duality(kind):
    """rho_mu(s) = min_w [w s + Phi_mu(w)], attained at weight_mu(s): in long double, on the grid."""
    wg = np.concatenate([np.linspace(0, 1, 201), np.logspace(-12, 0, 49)]).astype(LD)
    for c2 in C2S:
        for mu in MUS:
            s = np.asarray(grid(mu, c2), LD)
            w, rho = gr.weight_rho(kind, mu, c2, s, LD)
            scale = np.maximum(rho, LD(mu) * LD(c2) if kind == gr.TLS else rho) + LD(1e-300)
            tol = 64 * np.finfo(LD).eps * (scale + s * w + gr.phi(kind, mu, c2, w, LD))
            at = w * s + gr.phi(kind, mu, c2, w, LD)
            assert np.all(np.abs(at - rho) <= tol), (kind, mu, c2, float(np.max(np.abs(at - rho) / tol)))
            everywhere = wg[None, :] * s[:, None] + gr.phi(kind, mu, c2, wg, LD)[None, :]
            assert np.all(everywhere >= (rho - tol)[:, None]), (kind, mu, c2)


_runs = {}


def live_run(name, kind):
    if (name, kind) not in _runs:
        _runs[(name, kind)] = gi.compute(name, kind)
    return _runs[(name, kind)]


@pytest.mark.parametrize("kind", (gr.TLS, gr.GM))
@pytest.mark.parametrize("name", list(gi.CASES))
def test_the_restated_loop_on_the_inputs(name, kind):
    P, X, outlier = gi.case(name)
    R = P["inter"]
    r, gold = live_run(name, kind), gi.reference(name, kind)
    s = gr.edge_s(P, r["X"])
    print("%s kind %d: %d edges, %d in R, %d outliers; %d levels; worst inlier s %.3g, smallest outlier s %.4g; margin %.3g; worst "
          "relative D_k %.3g" % (name, kind, len(R), R.sum(), outlier.sum(), r["levels"], s[R & ~outlier].max(), s[outlier].min(),
                                 r["margin"], np.max(r["spread"] / np.abs(r["log"][:len(r["spread"]), 1:5]))))
    # the table
    assert (len(R), int(R.sum()), int(outlier.sum()), r["levels"]) == gi.TABLE[name][:3] + (gi.TABLE[name][3 + kind],)
    assert r["outcome"] == gr.CONVERGED and set(r["inner"]) == {0}
    rejected = (r["w"] == 0) if kind == gr.TLS else (s > gi.C2)
    assert np.array_equal(rejected & R, outlier) and r["num_outliers"] == outlier.sum()
    assert np.all(r["w"][~R] == 1.0)
    # within a level the surrogate does not increase; the thresholds are far; the perturbed start counts the same
    assert np.all(r["log"][:, 4] <= r["log"][:, 1])
    assert r["margin"] >= 1e-6
    assert r["same_counts"]
    # the committed file is this run
    assert (gold["outcome"], gold["levels"], gold["num_outliers"], gold["inner"]) == (r["outcome"], r["levels"], r["num_outliers"], r["inner"])
    assert np.array_equal(gold["log"][:, 7:], r["log"][:, 7:]) and gold["same_counts"] and gold["log"][:, 0].tolist() == r["log"][:, 0].tolist()
    assert np.all(np.abs(gold["log"][:, 1:5] - r["log"][:, 1:5]) <= np.maximum(100 * gold["spread"], 1e-9 * np.abs(r["log"][:, 1:5])))
    assert np.array_equal(gold["w"] == 0, r["w"] == 0) and np.allclose(gold["w"], r["w"], rtol=0, atol=1e-6)
    assert np.allclose(gold["X"], r["X"], rtol=0, atol=1e-6)
    assert np.all(gold["spread"] <= 1e-7 * np.abs(gold["log"][:, 1:5]))


def test_swapped_thresholds_are_caught_by_the_table():
    """The built-in slip (mu/(mu+1) and (mu+1)/mu swapped) changes the level count of the cheapest input."""
    P, X, _ = gi.case("c2_40")
    r = gr.run(P, X, gr.TLS, gi.C2, mu_step=gi.MU_STEP, swap_thresholds=True)
    assert r["levels"] != gi.TABLE["c2_40"][3] or not np.array_equal(r["log"][:, 7:], gi.reference("c2_40", gr.TLS)["log"][:, 7:])


def test_all_inliers_and_an_empty_robust_set():
    P, X, outlier = gi.case("c2_40", out_frac=0.0)
    assert not outlier.any()
    r = gr.run(P, X, gr.TLS, gi.C2)
    assert r["outcome"] == gr.ALL_INLIERS and r["levels"] == 0 and np.all(r["w"] == 1.0) and 2 * r["s_max_initial"] <= gi.C2
    for kind in (gr.TLS, gr.GM):
        r = gr.run(gi.case("c2_40")[0], gi.case("c2_40")[1], kind, gi.C2, R=np.zeros(len(P["I"]), bool))
        assert r["outcome"] == gr.ALL_INLIERS and r["levels"] == 0
    r = gr.run(gi.case("c2_40")[0], gi.case("c2_40")[1], gr.TLS, gi.C2, max_levels=3)
    assert r["outcome"] == gr.MAX_LEVELS and r["levels"] == 3
