"""The weighted edge pass of graduated non-convexity on the maximum-likelihood objective on the device
(dpgo_amd/csrc/ml_gnc.hip: k_ml_gnc_edge; gnc.hip: k_gnc_final) through NodeGroup.ml_gnc_eval, against the long-double restatement
(tests/ml_gnc_restatement.py) within the bounds tests/test_ml_gnc_host.py states -- ml_restatement.edge_bounds with the
constants of tests/test_ml_host.py, gnc_restatement.w_bound, and  w bound(q) + bound(w) |q| + u |w q|  -- and no others.

The chains are ml_inputs.chain(d, m) for m in {1, 63, 64, 65, 130}: one lane, a workgroup's edge on either side, and two
partials plus a remainder for the strided final wave.  The robust sets: empty, full, and one whose members all lie in one
workgroup.  WEIGH runs at three values of mu chosen on the CPU so that every robust edge sits at least 1e-6 relative from
either TLS threshold and (m >= 63) every branch -- w = 1, w = 0, between -- is taken by an edge.  The pass is held in stages:
chi2 against the restatement; w against the long-double weight of the device's own chi2 (w_bound is the bound of the formula
at a given s); the weighted outputs against the restatement with that w; the sums against the restated sums of the device's
own per-edge values within m u sum |terms|.  Edge 4 (m >= 5) sits at theta = pi - 5e-4, where chi2 is not specified: it is
kept out of the WEIGH runs' robust sets and gets weight 0 in the FIXED runs.  Nothing in a bound comes from the device.
"""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_restatement as cr  # noqa: E402
import gnc_restatement as gr  # noqa: E402
import ml_gnc_restatement as mgr  # noqa: E402
import ml_inputs as mi  # noqa: E402
import test_gpu_ml_ops as ops  # noqa: E402  (its groups; none of its tests is imported)
import test_ml_gnc_host as tgh  # noqa: E402  (its weights and ratios; none of its tests is imported)
import test_ml_host as tmh  # noqa: E402

import dpgo_amd  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = cr.LD
CONST = tmh.CONSTANTS
SIZES = [1, 63, 64, 65, 130]
_obj = {}


def objects(d, m):
    if (d, m) not in _obj:
        E, X, near = mi.chain(d, m)
        ref1 = mgr.weighted_edges(E, X, np.ones(m), LD)
        held = tmh.held_edges(E, ref1["unweighted"])
        grp = ops.group_of(E, 1)
        _obj[(d, m)] = (E, X, near, ref1, held, grp, grp.graph)
    return _obj[(d, m)]


def robust_sets(m, held, seed):
    """name -> R (bool): empty, full (every held edge), and a seeded half of one workgroup's edges (the second where there is one)."""
    rng = np.random.default_rng(seed)
    one = np.zeros(m, bool)
    lo, hi = (64, min(m, 128)) if m > 64 else (0, m)
    one[lo:hi] = rng.uniform(size=hi - lo) < 0.5
    one[lo] = True
    return {"empty": np.zeros(m, bool), "full": held.copy(), "one_workgroup": one & held}


def choose_mu(kind, c2, chi2, want_branches):
    """Three values of mu from a fixed ladder at which every chi2 sits >= 1e-6 relative from either TLS threshold and, if asked,
    every branch is taken."""
    out = []
    for k in range(60):
        mu = 0.05 * 1.31 ** k
        lo, hi = gr.thresholds(mu, c2)
        if len(chi2) and min(np.min(np.abs(chi2 - lo) / lo), np.min(np.abs(chi2 - hi) / hi)) < 1e-6:
            continue
        if kind == gr.TLS and want_branches and not (np.any(chi2 <= lo) and np.any(chi2 >= hi) and np.any((chi2 > lo) & (chi2 < hi))):
            continue
        out.append(mu)
    assert len(out) >= 3
    return [out[0], out[len(out) // 2], out[-1]]


def check_sums(kind, mu, c2, chi2, w, R, near, sums, m):
    want = mgr.sums(kind, mu, c2, chi2, w, R, near)
    tol = m * U
    assert abs(sums[0] - want["sum_out"]) <= tol * np.abs(chi2[~R]).sum()
    assert abs(sums[1] - want["sum_ws"]) <= tol * np.abs(w[R] * chi2[R]).sum() + U * np.abs(w[R] * chi2[R]).sum()
    rho = gr.weight_rho(kind, mu, c2, chi2[R], np.longdouble)[1].astype(np.float64)
    # rho: the formula's own rounding, a few u of its largest intermediate (2 sqrt(a s) and mu (c2 + s))
    brho = 8 * U * (np.abs(rho) + (mu + 1) * (c2 + chi2[R]) * (kind == gr.TLS))
    assert abs(sums[2] - rho.sum()) <= tol * np.abs(rho).sum() + brho.sum()
    assert sums[3] == want["s_max"] and sums[4] == want["w_min"]
    assert [int(v) for v in sums[5:]] == [want["zero"], want["one"], want["between"], want["near_pi"], want["near_pi_all"]]


def check_edges(E, X, w, bw, got, held, what, ref1):
    ref = mgr.weighted_edges(E, X, w, LD, unweighted=ref1)
    bnd = mgr.weighted_bounds(E, X, ref, w, bw, CONST)
    rr = tgh.worst_ratios(got, ref, bnd, held, w == 0)
    print("%s: %s" % (what, " ".join("%s %.3g" % kv for kv in rr.items())))
    assert all(v <= 1.0 for v in rr.values()), (what, rr)


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("m", SIZES)
def test_weigh_pass_against_the_restatement(d, m):
    E, X, near, ref1, held, grp, G = objects(d, m)
    chi2_ref = ref1["chi2"].astype(np.float64)
    c2 = float(np.median(chi2_ref[held])) if m > 1 else float(chi2_ref[0])
    nearf = ref1["near"]
    plain = grp.ml_eval(X, full=True)
    for kind in (gr.TLS, gr.GM):
        for rname, R in robust_sets(m, held, 7 * m + d).items():
            for mu in choose_mu(kind, c2, chi2_ref[R], m >= 63 and rname == "full"):
                start = np.full(m, 0.25)
                chi2, w, sums, more = grp.ml_gnc_eval(G, X, kind, mu, c2, robust_set=R.astype(np.int32), w_start=start, full=True)
                got = dict(more, chi2=chi2)
                assert np.array_equal(w[~R], start[~R])                     # the array outside R is not touched
                err = np.abs(chi2.astype(LD) - ref1["chi2"]).astype(np.float64)
                assert np.all(err[held] <= CONST["chi2"] * mgr.mr.edge_bounds(E, X, ref1["unweighted"])["chi2"][held])
                wl = gr.weight_rho(kind, mu, c2, chi2[R].astype(np.longdouble), np.longdouble)[0]
                assert np.all(np.abs(w[R] - wl.astype(np.float64)) <= gr.w_bound(kind, mu, wl))
                if kind == gr.TLS:
                    lo, hi = gr.thresholds(mu, c2)
                    assert np.array_equal(w[R] == 1, chi2_ref[R] <= lo) and np.array_equal(w[R] == 0, chi2_ref[R] >= hi)
                    if m >= 63 and rname == "full":
                        assert np.any(w[R] == 1) and np.any(w[R] == 0) and np.any((w[R] > 0) & (w[R] < 1))
                weff = np.where(R, w, 1.0)
                check_edges(E, X, weff, 0.0, got, held, "d = %d, m = %d, kind %d, R %s, mu %.3g" % (d, m, kind, rname, mu), ref1)
                check_sums(kind, mu, c2, chi2, weff, R, nearf, sums, m)
                if rname == "empty":     # w = 1 everywhere: the bits of k_ml_edge<D, true>
                    assert np.array_equal(chi2, plain[2]) and np.array_equal(more["r"], plain[1])
                    for k in ("wr", "grad", "Ji", "Jj", "Wi", "Wj"):
                        assert np.array_equal(more[k].view(np.uint64), plain[4][k].view(np.uint64)), k
                    assert sums[8] == sums[9] == near == plain[3]
    # a second call gives the same bits
    R = robust_sets(m, held, 7 * m + d)["full"].astype(np.int32)
    a = grp.ml_gnc_eval(G, X, gr.TLS, 1.0, c2, robust_set=R, full=True)
    b = grp.ml_gnc_eval(G, X, gr.TLS, 1.0, c2, robust_set=R, full=True)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and all(np.array_equal(a[3][k], b[3][k]) for k in a[3])


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("m", SIZES)
def test_fixed_pass_against_the_restatement(d, m):
    """Given weights with exact zeros -- on the edge near pi and on ordinary edges -- and exact ones, R every edge."""
    E, X, near, ref1, held, grp, G = objects(d, m)
    w = tgh.weights_for(m, 31 + m)
    R = np.ones(m, bool)
    c2 = float(np.median(ref1["chi2"].astype(np.float64)[held]))
    chi2, wo, sums, more = grp.ml_gnc_eval(G, X, gr.TLS, 1.0, c2, robust_set=R.astype(np.int32), w_in=w, full=True)
    got = dict(more, chi2=chi2)
    assert np.array_equal(wo, w)
    check_edges(E, X, w, 0.0, got, held, "d = %d, m = %d, fixed" % (d, m), ref1)
    zero = w == 0
    for k in ("wr", "grad", "Ji", "Jj", "Wi", "Wj"):
        assert not more[k][zero].any() and not np.signbit(more[k][zero]).any(), k
    assert np.all(np.isfinite(more["grad"])) and np.all(np.isfinite(more["Wi"])) and np.all(np.isfinite(more["Wj"]))
    check_sums(gr.TLS, 1.0, c2, chi2, w, R, ref1["near"], sums, m)
    assert sums[8] == 0 and sums[9] == near
    # unit weights on every edge, R full: the bits of the unweighted pass
    plain = grp.ml_eval(X, full=True)
    chi2, wo, sums, more = grp.ml_gnc_eval(G, X, gr.GM, 3.0, c2, robust_set=R.astype(np.int32), w_in=np.ones(m), full=True)
    assert np.array_equal(chi2, plain[2]) and np.array_equal(more["r"], plain[1]) and sums[6] == m and sums[8] == near
    for k in ("wr", "grad", "Ji", "Jj", "Wi", "Wj"):
        assert np.array_equal(more[k].view(np.uint64), plain[4][k].view(np.uint64)), k


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("m", [65, 130])
def test_zero_weights_are_the_filtered_graph_bit_for_bit(d, m):
    """g_w and H_w of weights in {0, 1} -- 0 on the edge near pi and on a seeded fifth of the others -- are finite and
    array_equal to g and H of the graph without those edges; H_w is symmetric to the bit; a second call gives the same bits."""
    E, X, near, ref1, held, grp, G = objects(d, m)
    rng = np.random.default_rng(3 * m + d)
    w = (rng.uniform(size=m) >= 0.2).astype(np.float64)
    w[4] = 0.0
    w[0] = 1.0
    dof = cr.dof_of(d)
    n = dof * E["N"]
    for a in (0, E["N"] - 1):
        ptr, col, val, g = grp.ml_gnc_hessian(G, X, w, robust_set=np.ones(m, np.int32), anchor=a)
        again = grp.ml_gnc_hessian(G, X, w, robust_set=np.ones(m, np.int32), anchor=a)
        assert np.all(np.isfinite(val)) and np.all(np.isfinite(g))
        assert np.array_equal(val, again[2]) and np.array_equal(g, again[3])
        D = sp.csr_matrix((val, col, ptr), shape=(n, n)).toarray()
        assert np.array_equal(D, D.T)
        p2, c2_, v2, g2, _ = grp.ml_hessian(X, anchor=a, graph=G.filter_edges(w > 0))
        assert np.array_equal(ptr, p2) and np.array_equal(col, c2_)
        assert np.array_equal(val, v2) and np.array_equal(g, g2)
        # and the restatement's, within the unweighted test's bounds, on the poses no edge near pi of positive weight touches
        Fr, gr_, Hr = mgr.assemble_w(E, X, w, a, LD)
        Ew = mgr.scaled(E, w)
        refw = mgr.mr.edges_all(Ew, X, LD)
        bF, bg, bH = mgr.mr.sum_bounds(Ew, E["N"], refw, mgr.mr.edge_bounds(Ew, X, refw))
        keep = np.ones(n, bool)
        keep[dof * a:dof * a + dof] = False
        eg = np.abs(np.asarray(g, LD) - gr_).astype(np.float64)
        eH = np.abs(np.asarray(D, LD) - Hr).astype(np.float64)
        kk = np.outer(keep, keep)
        assert np.all(eg[keep] <= CONST["g"] * bg[keep]) and np.all(eH[kk] <= CONST["H"] * bH[kk])
