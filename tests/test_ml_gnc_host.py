"""Graduated non-convexity on the maximum-likelihood objective, without a GPU: the host twin of the weighted edge pass
(dpgo_debug_ml_gnc_edge_host, through dpgo_amd/csrc/ml_gnc_math.h) against the long-double restatement
(tests/ml_gnc_restatement.py), the two exact cases w = 1 and w = 0, the committed restated runs
(tests/golden/ml_gnc_reference.npz) against a recomputed one and against the maker's conditions, the Black-Rangarajan
invariant on their logs, the weighted gradient against a central difference of F_w, and the C ABI.

The bounds: ml_restatement.edge_bounds with the constants of tests/test_ml_host.py (CONSTANTS) for the unweighted quantities,
gnc_restatement.w_bound for w, and  w bound(q) + bound(w) |q| + u |w q|  for a weighted quantity w q
(ml_gnc_restatement.weighted_bounds).  No further constant was needed: test_host_twin prints how much of each bound is used.
The GPU tests use these bounds and no others.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_restatement as cr  # noqa: E402
import gnc_restatement as gr  # noqa: E402
import ml_gnc_inputs as mgi  # noqa: E402
import ml_gnc_restatement as mgr  # noqa: E402
import ml_inputs as mi  # noqa: E402
import ml_restatement as mr  # noqa: E402
import newton_restatement as nr  # noqa: E402
import test_ml_host as tmh  # noqa: E402  (its constants, graphs and helpers; none of its tests is imported)

import dpgo_amd  # noqa: E402

U = 2.0 ** -53
LD = cr.LD
CONST = tmh.CONSTANTS
KEYS = ("r", "chi2", "wr", "grad", "Ji", "Jj", "Wi", "Wj")


def weights_for(m, seed):
    """Seeded weights in [0, 1] with exact zeros and ones among them; m >= 5: edge 4 (ml_inputs.chain's edge near pi) gets 0."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0, 1, m)
    w[rng.uniform(size=m) < 0.2] = 0.0
    w[rng.uniform(size=m) < 0.2] = 1.0
    if m >= 5:
        w[4] = 0.0
    return w


def worst_ratios(got, ref, bnd, held, zero):
    """Per output the largest error in units of its bound over the held edges; where the bound is zero the error must be.
    held: the edges away from pi; zero: the edges of weight 0, whose weighted outputs are exact zeros even near pi."""
    out = {}
    for k in KEYS:
        hk = held if k in ("r", "chi2") else held | zero
        err = np.abs(np.asarray(got[k], LD) - ref[k]).astype(np.float64)[hk]
        b = bnd[k][hk]
        assert np.all(err[b == 0] == 0), k
        out[k] = float((err[b > 0] / b[b > 0]).max()) if np.any(b > 0) else 0.0
    return out


def twin_inputs():
    out = [("chain%d_%d" % (d, m),) + mi.chain(d, m)[:2] for d in (2, 3) for m in (1, 65)]
    for name in mgi.CASES:
        E, X = mgi.case(name)[:2]
        out.append((name, E, X))
    return out


def test_host_twin_against_the_long_double_restatement():
    for name, E, X in twin_inputs():
        m = len(E["I"])
        w = weights_for(m, 5 + m)
        ref = mgr.weighted_edges(E, X, w, LD)
        bnd = mgr.weighted_bounds(E, X, ref, w, 0.0, CONST)
        held = tmh.held_edges(E, ref["unweighted"])
        got = dpgo_amd.ml_gnc_edge_debug(tmh.graph_of(E), X, w)
        rr = worst_ratios(got, ref, bnd, held, w == 0)
        print(name, " ".join("%s %.3g" % kv for kv in rr.items()))
        assert all(v <= 1.0 for v in rr.values()), (name, rr)
        near = ref["near"]
        assert got["near_pi"] == int(np.sum(near & (w > 0))) and got["near_pi_all"] == int(near.sum())
        # the fp64 restatement obeys the same bounds
        own = worst_ratios(mgr.weighted_edges(E, X, w), ref, bnd, held, w == 0)
        assert all(v <= 1.0 for v in own.values()), (name, own)


@pytest.mark.parametrize("d", [2, 3])
def test_unit_weights_give_the_unweighted_bits_and_zero_weights_exact_zeros(d):
    E, X, near = mi.chain(d, 65)
    G = tmh.graph_of(E)
    m = len(E["I"])
    plain = dpgo_amd.ml_edge_debug(G, X)
    one = dpgo_amd.ml_gnc_edge_debug(G, X, np.ones(m))
    Wi = np.einsum("ekl,ela->eka", E["Om"], plain["Ji"])
    for k in ("r", "wr", "chi2", "Ji", "Jj", "grad"):
        assert np.array_equal(one[k].view(np.uint64), plain[k].view(np.uint64)), k
    assert np.abs(one["Wi"] - Wi).max() <= 64 * U * np.abs(Wi).max()
    assert one["near_pi"] == one["near_pi_all"] == plain["near_pi"] == near == 1
    # edge 4 sits at theta = pi - 5e-4, where the values are not specified: weight 0 takes it out whatever they are
    zero = dpgo_amd.ml_gnc_edge_debug(G, X, np.zeros(m))
    for k in ("wr", "grad", "Ji", "Jj", "Wi", "Wj"):
        assert not zero[k].any() and not np.signbit(zero[k]).any(), k
    assert np.array_equal(zero["r"], plain["r"]) and np.array_equal(zero["chi2"], plain["chi2"])
    assert zero["near_pi"] == 0 and zero["near_pi_all"] == 1
    w = np.ones(m)
    w[4] = 0.0
    mixed = dpgo_amd.ml_gnc_edge_debug(G, X, w)
    assert not mixed["grad"][4].any() and not mixed["Wi"][4].any() and not mixed["Ji"][4].any() and mixed["near_pi"] == 0
    keep = w > 0
    assert np.array_equal(mixed["grad"][keep], plain["grad"][keep]) and np.array_equal(mixed["wr"][keep], plain["wr"][keep])
    with pytest.raises(ValueError):
        dpgo_amd.ml_gnc_edge_debug(G, X, 1.5 * np.ones(m))
    with pytest.raises(ValueError):
        dpgo_amd.ml_gnc_edge_debug(G, X, np.ones(m - 1))


def test_golden_file_is_the_restatement_on_the_smallest_case():
    name, kind = mgi.SMALLEST
    run = mgi.compute(name, kind)
    z = np.load(os.path.join(mgi.GOLDEN, "ml_gnc_reference.npz"))
    for k, v in mgi.pack(name, kind, run).items():
        assert np.array_equal(z[k], v), k
    assert set(z.files) == {k for n, kd in mgi.RUNS for k in mgi.pack(n, kd, dict(run))}


@pytest.mark.parametrize("name,kind", mgi.RUNS)
def test_committed_runs_meet_the_conditions_and_the_invariant(name, kind):
    """The maker's conditions, from the committed arrays (the restatement is not run again), and F_mu(X_k) <= F_mu(X_{k-1})
    within a level up to the rounding of the two sums, m u sum |terms| <= m u (F_mu(X_{k-1}) + F_mu(X_k))."""
    E, X, R, outlier, _ = mgi.case(name)
    ref = mgi.reference(name, kind)
    chi2 = mgr.chi2_theta(E, ref["X"])[0]
    rejected = (R & (ref["w"] == 0)) if kind == mgr.TLS else (R & (chi2 > mgi.C2[E["d"]]))
    print("%s %d: %d levels, inner %s, %d outliers, TLS margin %.3g, decision margin %.3g, theta_max %.3g" %
          (name, kind, ref["levels"], ref["inner"], int(outlier.sum()), ref["margin"], ref["decision_margin"], ref["theta_max"]))
    assert ref["outcome"] == mgr.CONVERGED and nr.STALLED not in ref["inner"] and ref["inner"][-1] == nr.CONVERGED
    assert np.array_equal(rejected, outlier) and outlier.sum() >= 1 and ref["num_outliers"] == outlier.sum()
    assert ref["margin"] >= 1e-6 and ref["theta_max"] <= np.pi - 0.1 and ref["same_counts"]
    assert ref["near_pi"] == 0 and ref["decision_margin"] >= 4 * max(CONST["g"], CONST["F"])
    log = ref["log"]
    assert len(log) == ref["levels"] and np.all(ref["w"][~R] == 1.0)
    m = len(R)
    assert np.all(log[:, 4] <= log[:, 1] + m * U * (log[:, 1] + log[:, 4]))
    assert np.all(log[:, 3] <= log[:, 2] + m * U * (log[:, 2] + log[:, 3]))      # the inner solve does not increase F_w
    if kind == mgr.TLS:
        assert log[-1, 9] == 0 and np.all(log[:-1, 9] > 0) and np.all((ref["w"] == 0) | (ref["w"] == 1))
    else:
        assert log[-1, 0] == 1.0 and np.all(log[:-1, 0] > 1.0)


LEVEL0_STALL = dict(name="m2_40", kind=mgr.TLS, max_tries=1)   # tests/test_gpu_ml_gnc.py runs the device on the same input


@pytest.mark.parametrize("start", ["X", "perturbed"])
def test_level_zero_stall_of_the_restatement(start):
    """With one try per step the unit-weight solve of m2_40 stalls before any level: INNER_FAILED at level 0 with the start
    itself and unit weights, from the case's start and from the perturbed one alike -- the input of the device's test of that
    path."""
    E, X, R, _, _ = mgi.case(LEVEL0_STALL["name"])
    X0 = X if start == "X" else mgi.perturbed(X)
    run = mgr.run(E, X0, LEVEL0_STALL["kind"], mgi.C2[E["d"]], R, mu_step=mgi.MU_STEP, max_tries=LEVEL0_STALL["max_tries"])
    assert run["outcome"] == mgr.INNER_FAILED and run["levels"] == 0 and run["inner"] == [nr.STALLED] and len(run["log"]) == 0
    assert (run["steps"], run["factorisations"]) == (14, 15)
    assert np.array_equal(run["X"], X0) and np.all(run["w"] == 1.0)


@pytest.mark.parametrize("name", ["m3_24", "m2_40"])
def test_weighted_gradient_is_the_central_difference_of_F_w(name):
    """g_w'v, g_w assembled from the host twin's gradient terms, against (F_w(retract(X, h v)) - F_w(retract(X, -h v))) / 2h with
    F_w in long double, five seeded directions, h = 1e-5, seeded weights with zeros and ones: the tolerance of
    tests/test_ml_host.py's gradient test.  A gradient that ignores the weights has to fail."""
    E, X = mgi.case(name)[:2]
    d, N = E["d"], E["N"]
    dof = cr.dof_of(d)
    w = weights_for(len(E["I"]), 91)
    got = dpgo_amd.ml_gnc_edge_debug(tmh.graph_of(E), X, w)
    g, g_plain = np.zeros(dof * N), np.zeros(dof * N)
    plain = mr.edges_all(E, X)
    for e in range(len(w)):
        for a, p in enumerate((int(E["I"][e]), int(E["J"][e]))):
            g[dof * p:dof * p + dof] += got["grad"][e, a]
            g_plain[dof * p:dof * p + dof] += plain["grad"][e, a]
    Ew = mgr.scaled(E, w)
    rng = np.random.default_rng(29)
    h, told = 1e-5, 0
    rounding = U * float(np.linalg.norm(X)) * float(np.sqrt((got["grad"] ** 2).sum())) * np.sqrt(len(w)) / h
    for _ in range(5):
        v = rng.standard_normal(len(g))
        v /= np.linalg.norm(v)
        fd, floor = tmh.central(lambda s: mr.objective(Ew, cr.retract(X, s * v, d), LD), h)
        gv = float(g @ v)
        tol = 1e-6 * abs(gv) + float(floor) + rounding
        told += abs(float(fd) - float(g_plain @ v)) > tol
        print("%s: g_w'v %.9g, central difference %.9g, difference %.3g, tolerance %.3g" % (name, gv, float(fd), abs(float(fd) - gv), tol))
        assert abs(float(fd) - gv) <= tol
    assert told >= 3


def test_weights_through_the_host_weight_function_on_chi2():
    """gnc_weight_rho is unchanged and is applied to s = chi2: the host hook's w on the twin's chi2 within w_bound of the
    long-double weight of the same chi2, at the three mu of a level's thresholds."""
    E, X, R, _, _ = mgi.case("m3_24")
    chi2 = dpgo_amd.ml_gnc_edge_debug(tmh.graph_of(E), X, np.ones(len(R)))["chi2"]
    c2 = mgi.C2[3]
    for kind in (mgr.TLS, mgr.GM):
        for mu in (0.05, 1.0, 40.0):
            w, rho = dpgo_amd.gnc_weight_debug(kind, mu, c2, chi2[R])
            wl = gr.weight_rho(kind, mu, c2, chi2[R], np.longdouble)[0]
            assert np.all(np.abs(w - wl.astype(np.float64)) <= gr.w_bound(kind, mu, wl))


def test_ml_gnc_abi():
    L = dpgo_amd.lib()
    # the GNC result, two long longs
    assert C.sizeof(dpgo_amd.MlGncResult) == C.sizeof(dpgo_amd.GncResult) + 16
    r = dpgo_amd.MlGncResult()
    assert r.outcome == 0 and r.gnc.levels == 0 and r.near_pi == 0 and r.near_pi_all == 0
    with pytest.raises(AttributeError):
        r.no_such_field
    X = np.zeros((8, 3), order="F")
    dp = X.ctypes.data_as(C.POINTER(C.c_double))
    o = dpgo_amd.GncOptions(barc2=22.458)
    assert o.barc2 == 22.458 and o.kind == dpgo_amd.GNC_TLS
    nnz = C.c_longlong(0)
    E, Xc, _ = mi.chain(3, 1)
    G = tmh.graph_of(E)
    w = np.ones(1)
    wp = w.ctypes.data_as(C.POINTER(C.c_double))
    for grp in (None, C.c_void_p(0)):
        assert L.dpgo_group_ml_gnc(grp, G._h, dp, 8, C.byref(o), None, 0, dp, 8, wp, None, 0, C.byref(r)) == -1
        assert L.dpgo_group_ml_gnc_eval(grp, G._h, dp, 8, 0, 1.0, 1.0, None, None, 0, wp, wp, dp, None, None, None, None) == -1
        assert L.dpgo_group_debug_ml_gnc_hessian(grp, G._h, dp, 8, 0, None, wp, None, None, None, 0, C.byref(nnz), None) == -1
    assert L.dpgo_debug_ml_gnc_edge_host(None, dp, 8, wp, *[None] * 7) == -1
    assert L.dpgo_debug_ml_gnc_edge_host(G._h, dp, 3, wp, *[None] * 7) == -1      # (a short X)
    assert L.dpgo_debug_ml_gnc_edge_host(G._h, dp, 8, None, *[None] * 7) == -1    # (no weights)
    header = open(os.path.join(os.path.dirname(dpgo_amd.__file__), "..", "include", "dpgo_amd.h")).read()
    for sym in ("dpgo_group_ml_gnc", "dpgo_group_ml_gnc_eval", "dpgo_group_debug_ml_gnc_hessian", "dpgo_debug_ml_gnc_edge_host"):
        assert sym + "(" in header and sym in dpgo_amd.SYMBOLS and hasattr(L, sym)
    assert "dpgo_ml_gnc_result_t" in header
    for name in ("ml_gnc", "ml_gnc_eval", "ml_gnc_hessian"):
        assert hasattr(dpgo_amd.NodeGroup, name)
    assert hasattr(dpgo_amd, "ml_gnc_edge_debug") and hasattr(dpgo_amd, "MlGncResult")
