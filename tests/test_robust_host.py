"""The robust objective without a GPU: the numpy restatement (tests/robust_restatement.py) against finite differences and
against the restatements it extends, the library's per-edge arithmetic (dpgo_amd/csrc/robust_math.h through
dpgo_debug_robust_edge_host) against the long-double restatement within first-order bounds, the bounds held honest in both
directions (the fp64 restatement stays inside, injected faults fall outside), the committed trajectory table, and the argument
checks of the new entry points.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cert_restatement as cert  # noqa: E402
import cov_restatement as cr  # noqa: E402
import newton_restatement as nr  # noqa: E402
import robust_inputs as ri  # noqa: E402
import robust_restatement as rr  # noqa: E402

import dpgo_amd  # noqa: E402
from oracle.problem import LOSS_GM, LOSS_HUBER, LOSS_NONE, LOSS_WELSCH  # noqa: E402

LD = np.longdouble
LOSSES = (LOSS_HUBER, LOSS_GM, LOSS_WELSCH)
OPS_INPUTS = {"tiny": 5.0, "rand2_70": 5.0, "rand3_70": 5.0, "rand2_160": 5.0, "rand3_160": 5.0, "ladder2": 0.25, "ladder3": 0.25,
              "rand2_600": 5.0, "rand3_600": 5.0, "rand2_40": 5.0, "rand3_40": 5.0, "ladder2x2": 0.25, "ladder3x2": 0.25}


def worst(got, want, bound):
    err = np.abs(np.asarray(np.asarray(got, LD) - want, np.float64))
    assert np.all(np.isfinite(bound))
    return float(np.max(err / np.maximum(bound, 1e-300))), bool(np.all(err <= bound))


# ---------------------------------------------------------------------------------------------------------------
# 1. the restatement itself
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("loss", LOSSES)
def test_gradient_and_hessian_against_central_differences(d, loss):
    """At random_graph's own X (not a critical point), in long double: g'v against the central difference of F along the
    retraction, and v'Hv against the central difference of g'v -- the one-parameter subgroups of the retraction are geodesics,
    so the frame's own derivative drops out of v' (d/dh g) -- and against the second difference of F.  Steps 1e-5 and 1e-4:
    the truncation error of a central difference is O(h^2) of third derivatives, the rounding 2^-64 / h."""
    P, X = ri.named("rand%d_70" % d)
    dl = 5.0
    dof = cr.dof_of(d)
    v = np.random.default_rng(7).standard_normal(dof * P["N"])
    v /= np.linalg.norm(v)
    g = rr.grad(P, X, loss, dl, dtype=LD)
    H = rr.hessian(P, X, loss, dl, 1, dtype=LD)
    h = 1e-5
    Zp, Zm = cr.retract(X, h * v, d), cr.retract(X, -h * v, d)
    dF = (rr.objective(P, Zp, loss, dl, LD) - rr.objective(P, Zm, loss, dl, LD)) / (2 * h)
    dg = (rr.grad(P, Zp, loss, dl, dtype=LD) @ v - rr.grad(P, Zm, loss, dl, dtype=LD) @ v) / (2 * h)
    h2 = 1e-4
    d2F = (rr.objective(P, cr.retract(X, h2 * v, d), loss, dl, LD) - 2 * rr.objective(P, X, loss, dl, LD) +
           rr.objective(P, cr.retract(X, -h2 * v, d), loss, dl, LD)) / h2 ** 2
    gv, vHv = float(g @ v), float(v @ H @ v)
    print("d %d loss %d: g'v %.12g (difference %.12g), v'Hv %.12g (of g: %.12g, of F: %.12g)" % (d, loss, gv, float(dF), vHv, float(dg), float(d2F)))
    assert abs(gv - float(dF)) <= 1e-7 * abs(gv)
    assert abs(vHv - float(dg)) <= 1e-6 * abs(vHv) and abs(vHv - float(d2F)) <= 1e-5 * abs(vHv)
    # the curvature of the loss is part of it: without the rank-one terms the same comparison fails
    H0 = rr.hessian(P, X, loss, dl, 0, dtype=LD)
    assert abs(float(v @ H0 @ v) - float(dg)) > 1e-4 * abs(vHv)
    assert float(np.abs(H - H.T).max()) <= 1e-15 * float(np.abs(H).max())


@pytest.mark.parametrize("name", ["tiny", "rand2_70", "rand3_70"])
def test_trivial_loss_is_the_newton_restatement(name):
    """Under loss 0 every weight is 1 and every curvature 0: M_w is the data matrix, and the loop is newton_restatement's on
    it -- the same outcome, counts and tries; F and the point to rounding (F is summed per edge here, as a product there)."""
    P, X = ri.named(name)
    d = P["d"]
    s, rho, w, c = rr.weights(P, X, LOSS_NONE, 1.0)
    assert np.all(w == 1.0) and not c.any() and np.array_equal(rho, s)
    M = rr.weighted_matrix(P, w)
    assert np.array_equal(rr.hessian(P, X, LOSS_NONE, 1.0, 1, 0), rr.hessian(P, X, LOSS_NONE, 1.0, 0, 0))
    Hn = nr.anchored_hessian(M, X, d, 0)
    Hr = rr.hessian(P, X, LOSS_NONE, 1.0, 1, 0)
    assert np.abs(Hr - Hn).max() <= 1e-12 * np.abs(Hn).max()
    assert np.abs(rr.grad(P, X, LOSS_NONE, 1.0, 0) - nr.grad(M, X, d, 0)).max() <= 1e-12 * np.abs(nr.grad(M, X, d, 0)).max()
    a, b = rr.polish_full(P, X, LOSS_NONE, 1.0), nr.polish_full(M, X, d)
    for f in ("outcome", "steps", "factorisations", "indefinite"):
        assert a[f] == b[f], f
    assert np.array_equal(a["log"][:, 4], b["log"][:, 4])
    # F is summed per edge from the residuals here and is 1/2 <X, M X> there: the two differ by the constant
    # 1/2 sum_e kappa_e tr(R_e R_e^T - I), which is zero to rounding only for an exactly orthogonal measured R
    off = 0.5 * float(np.sum(P["kappa"] * (np.einsum("eij,eij->e", P["R"], P["R"]) - d)))
    assert np.all(np.abs(a["log"][:, 0] - b["log"][:, 0] - off) <= 1e-11 * np.abs(b["log"][:, 0]))
    assert np.abs(a["X"] - b["X"]).max() <= 1e-9


def test_the_data_matrix_is_the_oracles(fixtures_dir):
    """sum_e M_e is the certificate's M (oracle.star.GlobalProblem.M) on tinyGrid3D, entry by entry within the bound of M_w."""
    import test_gpu_certify as tc
    P, X = ri.named("tiny")
    M = np.asarray(tc.problem(fixtures_dir, "tinyGrid3D")[3].M.todense())
    R = ri.reference("tiny", LOSS_NONE, 1.0)
    assert np.all(np.abs(np.asarray(M - R["M"], np.float64)) <= R["bM"] + 8 * rr.U * np.abs(M))


@pytest.mark.parametrize("name", ["tiny", "rand2_160", "rand3_70"])
@pytest.mark.parametrize("loss", LOSSES)
def test_curvature_0_is_the_covariance_hessian_of_the_scaled_graph(name, loss):
    P, X = ri.named(name)
    d, dl = P["d"], OPS_INPUTS[name]
    w = rr.weights(P, X, loss, dl)[2]
    Ms = rr.weighted_matrix(dict(P, kappa=P["kappa"] * w, tau=P["tau"] * w), np.ones(len(w)))
    want = cr.hessian(cert.S_matrix(Ms, X, d), X, d)
    got = rr.hessian(P, X, loss, dl, 0)
    R = ri.reference(name, loss, dl, curvature=0, anchor=None)
    assert np.all(np.abs(got - want) <= 2 * R["bH"])


# ---------------------------------------------------------------------------------------------------------------
# 2. robust_math.h against the long-double restatement; the bounds in both directions
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(OPS_INPUTS))
def test_per_edge_arithmetic_against_the_restatement(name):
    P, X = ri.named(name)
    dl = OPS_INPUTS[name]
    G = ri.graph(P)
    rows_ref, rb = rr.edge_rows(P, X, LD), rr.rows_bound(P, X)
    gh_ref, gb = rr.edge_ghat(P, X, LD, rows_ref), rr.ghat_bound(P, X, rb)
    for loss in (LOSS_NONE,) + LOSSES:
        w, c, rows, gh = dpgo_amd.robust_edge_debug(G, X, loss, dl)
        s, rho, w_ref, c_ref = rr.weights(P, X, loss, dl, LD)
        bw, bc = rr.w_bound(P, X, loss, dl), rr.c_bound(P, X, loss, dl)
        res = [worst(w, w_ref, bw), worst(c, c_ref, bc), worst(rows, rows_ref, rb), worst(gh, gh_ref, gb)]
        # the fp64 numpy restatement stays inside the same bounds
        s64, _, w64, c64 = rr.weights(P, X, loss, dl)
        r64 = rr.edge_rows(P, X)
        res64 = [worst(w64, w_ref, bw), worst(c64, c_ref, bc), worst(r64, rows_ref, rb), worst(rr.edge_ghat(P, X, rows=r64), gh_ref, gb)]
        print("%s loss %d: error / bound of w, c, rows, ghat: library %s, fp64 numpy %s" %
              (name, loss, ["%.3f" % r[0] for r in res], ["%.3f" % r[0] for r in res64]))
        assert all(r[1] for r in res) and all(r[1] for r in res64)
        assert np.all(c[~P["inter"]] == 0.0) and np.all(c[w == 0.0] == 0.0)
        if loss == LOSS_NONE:
            assert not c.any() and np.all(w == 1.0)
        # the host's weights are edge_eval_host's, bit for bit: the same edge_lane
        assert np.array_equal(w, dpgo_amd.edge_eval_host(G, X, loss, dl)[3])


@pytest.mark.parametrize("name", ["rand2_160", "rand3_160", "ladder2", "ladder3", "rand2_600", "rand3_40", "ladder3x2"])
def test_fp64_restatement_stays_inside_the_bounds_of_g_H_and_M(name):
    P, X = ri.named(name)
    dl = OPS_INPUTS[name]
    for loss in LOSSES:
        R = ri.reference(name, loss, dl)
        out = [worst(rr.hessian(P, X, loss, dl, 1, 0), R["H"], R["bH"]), worst(rr.grad(P, X, loss, dl, 0), R["g"], R["bg"]),
               worst(rr.weighted_matrix(P, rr.weights(P, X, loss, dl)[2]), R["M"], R["bM"])]
        print("%s loss %d: fp64 error / bound of H %.3f, g %.3f, M_w %.3f" % (name, loss, out[0][0], out[1][0], out[2][0]))
        assert all(o[1] for o in out)


def faulty_hessian(P, X, loss, dl, fault, anchor=0):
    """The fp64 restated H with one fault injected."""
    d = P["d"]
    dof = cr.dof_of(d)
    s, _, w, c = rr.weights(P, X, loss, dl)
    ge = rr.edge_ghat(P, X)
    left, right = ge, ge
    reversed_inter = np.nonzero(P["inter"] & (P["I"] > P["J"]) & (c != 0))[0]
    pairs = {}
    for e in np.nonzero(c)[0]:
        pairs.setdefault((min(P["I"][e], P["J"][e]), max(P["I"][e], P["J"][e])), []).append(e)
    parallel = [v for v in pairs.values() if len(v) > 1]
    if fault == "sign of c":
        c = -c
    elif fault == "factor 2 in c":
        c = 2 * c
    elif fault == "Huber's c below the kink":
        assert loss == LOSS_HUBER and (P["inter"] & (s <= dl)).any()
        c = np.where(P["inter"], -w / s, 0.0)
    elif fault == "roles swapped on a reversed edge":
        assert len(reversed_inter)
        left = right = ge.copy()
        left[reversed_inter[0]] = ge[reversed_inter[0], ::-1]
    elif fault == "a parallel edge dropped":
        assert parallel
        c = c.copy()
        c[parallel[0][1]] = 0
    _, S = rr.S_w(P, X, w)
    H = rr.add_rank1(P, rr.project(S, X, d), left, right, c)
    if fault == "the anchor's column not skipped":
        A = np.array(H)
        r = slice(dof * anchor, dof * anchor + dof)
        A[r, :] = 0
        A[r, r] = np.eye(dof)
        return A
    return rr.anchored(H, anchor, dof)


FAULTS = [("sign of c", LOSS_GM), ("factor 2 in c", LOSS_WELSCH), ("Huber's c below the kink", LOSS_HUBER),
          ("roles swapped on a reversed edge", LOSS_GM), ("a parallel edge dropped", LOSS_GM), ("the anchor's column not skipped", LOSS_GM),
          ("sign of c", LOSS_HUBER)]


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("fault,loss", FAULTS)
def test_injected_faults_fall_outside_the_bound(d, fault, loss):
    """Each fault, injected into the fp64 restatement, is caught by the bound of H on random_graph(d, 160, N=40) (parallel and
    reversed inter-node edges); without a fault the same function stays inside."""
    name = "rand%d_160" % d
    P, X = ri.named(name)
    dl = OPS_INPUTS[name]
    R = ri.reference(name, loss, dl)
    assert worst(faulty_hessian(P, X, loss, dl, None), R["H"], R["bH"])[1]
    ratio, ok = worst(faulty_hessian(P, X, loss, dl, fault), R["H"], R["bH"])
    print("d %d, %s: worst error / bound %.3g" % (d, fault, ratio))
    assert not ok and ratio > 1e3


# ---------------------------------------------------------------------------------------------------------------
# 3. the committed trajectory table
# ---------------------------------------------------------------------------------------------------------------
def test_trajectory_table_is_the_restatements():
    rows = ri.trajectories()
    by = {r["name"]: r for r in rows}
    for r in rows:
        c1 = r["curvature1"]
        assert r["device"] == (c1["outcome"] == rr.CONVERGED and c1["factorisations"] <= 12)
        assert len(c1["tries"]) == len(c1["F"]) and sum(c1["tries"]) == c1["factorisations"]
    assert sum(r["device"] for r in rows) >= 10
    assert any(r["device"] and r["loss"] == LOSS_WELSCH and r["input"].startswith("random:2") for r in rows)   # the Welsch d = 2 row
    assert not by["random3_huber5"]["device"] and by["random3_huber5"]["curvature1"]["factorisations"] == 20
    # the curvature of the loss pays on every Huber row
    for r in rows:
        if r["loss"] == LOSS_HUBER and r["device"]:
            assert r["curvature0"]["steps"] > r["curvature1"]["steps"], r["name"]
    assert by["big2_huber5"]["device"] and by["ones2_huber5"]["device"] and by["ones3_huber5"]["device"]
    for name in ("tiny2_huber", "random2_huber5", "random2_welsch100", "ones2_huber5"):
        r = by[name]
        P, X = ri.trajectory_problem(r)
        for curv in (1, 0):
            run, want = rr.polish_full(P, X, r["loss"], r["delta"], curv), r["curvature%d" % curv]
            assert (run["outcome"], run["steps"], run["factorisations"], run["indefinite"]) == \
                (want["outcome"], want["steps"], want["factorisations"], want["indefinite"]), (name, curv)
            assert run["log"][:, 4].astype(int).tolist() == want["tries"] and run["log"][:, 0].tolist() == want["F"]


# ---------------------------------------------------------------------------------------------------------------
# 4. the entry points
# ---------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("dpgo_group_robust_polish", "dpgo_group_robust_covariance", "dpgo_group_robust_hessian", "dpgo_group_robust_matrix",
               "dpgo_debug_robust_edge_host")


def test_symbols_and_argument_checks():
    import ctypes as C
    L = dpgo_amd.lib()
    header = open(os.path.join(ri.ROOT, "include", "dpgo_amd.h")).read()
    for sym in NEW_SYMBOLS:
        assert sym + "(" in header and sym in dpgo_amd.SYMBOLS and hasattr(L, sym)
    P, X = ri.named("rand2_70")
    G = ri.graph(P)
    for bad in (dict(loss=4), dict(loss=-1), dict(loss=LOSS_HUBER, loss_reg=0.0), dict(loss=LOSS_GM, loss_reg=-1.0),
                dict(loss=LOSS_WELSCH, loss_reg=float("nan")), dict(loss=LOSS_HUBER, loss_reg=float("inf"))):
        with pytest.raises(ValueError):
            dpgo_amd.robust_edge_debug(G, X, **bad)
    with pytest.raises(ValueError):
        dpgo_amd.robust_edge_debug(G, X[:-1], LOSS_HUBER, 1.0)
    dpgo_amd.robust_edge_debug(G, X, LOSS_NONE, float("nan"))          # (loss 0 ignores loss_reg, as dpgo_edge_eval_run does)
    # NULL handles and outputs: -1 before anything touches a device
    Xf = np.asfortranarray(X)
    xp = Xf.ctypes.data_as(C.POINTER(C.c_double))
    nnz = C.c_longlong(0)
    r, cv = dpgo_amd.PolishResult(), dpgo_amd.CovResult()
    assert L.dpgo_group_robust_polish(None, G._h, xp, Xf.shape[0], 1, 0.25, 1, None, 0, xp, Xf.shape[0], None, 0, C.byref(r), None) == -1
    assert L.dpgo_group_robust_covariance(None, G._h, xp, Xf.shape[0], 1, 0.25, 1, 0, 0, None, 0, xp, None, C.byref(cv)) == -1
    assert L.dpgo_group_robust_hessian(None, G._h, xp, Xf.shape[0], 1, 0.25, 1, 0, None, None, None, 0, C.byref(nnz), None, None, None, None, None, None, None) == -1
    assert L.dpgo_group_robust_matrix(None, G._h, xp, Xf.shape[0], 1, 0.25, None, None, None, 0, C.byref(nnz)) == -1
    assert L.dpgo_debug_robust_edge_host(None, xp, Xf.shape[0], 1, 0.25, None, None, None, None) == -1
