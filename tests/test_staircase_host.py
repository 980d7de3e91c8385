"""Host side of the Riemannian staircase (dpgo_amd/csrc/stair.h): the numpy restatement of the rule
(tests/staircase_restatement.py) -- its gradient against central differences of F along the retraction, its Hessian against
central differences of the projected gradient, its retraction's orthonormality, the four runs the feature was asked for on --
and the argument checks of the C ABI.  No GPU.

The refusals that need a group (a robust loss, a strict subset of the nodes, r_max outside [d, 2d], a short ld on a live
handle) are in tests/test_gpu_staircase.py: a group cannot be created without a device.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import newton_restatement as nr  # noqa: E402
import staircase_restatement as st  # noqa: E402
import test_polish_host as tph  # noqa: E402  (its points and its long-double objective; none of its tests is imported)

import dpgo_amd  # noqa: E402
from dpgo_amd import synthetic  # noqa: E402
from oracle import g2o as og  # noqa: E402
from oracle.hash import Options as OOptions  # noqa: E402
from oracle.problem import LOSS_NONE  # noqa: E402
from oracle.star import GlobalProblem, chordal_initialization  # noqa: E402

U = 2.0 ** -53
ETA = 1e-3
_rings = {}


def ring12(d):
    """(GlobalProblem, mm, the twisted start polished to its local minimum, the polished chordal point) of
    synthetic.twisted_ring(d, 12, 0.02, 1, 1)."""
    if d not in _rings:
        g, X0 = synthetic.twisted_ring(d, 12, 0.02, 1, 1)
        z = np.zeros(12, np.int64)
        mm = og.Measurements(z, g["I"], z, g["J"], g["R"], g["t"], g["kappa"], g["tau"])
        gp = GlobalProblem(12, mm, 1, OOptions.driver(LOSS_NONE, True))
        Xt = nr.polish(gp.M, X0, d)[0]
        Xc = nr.polish(gp.M, chordal_initialization(12, mm), d)[0]
        _rings[d] = (gp, mm, g, Xt, Xc)
    return _rings[d]


def lifted_points(fixtures_dir):
    """tinyGrid3D's data matrix with seeded random feasible points at rank d, d + 1 and 2d (narrow: r columns)."""
    gp, _ = tph.start_point(fixtures_dir, "tinyGrid3D", "chordal")
    d = gp.d
    N = gp.M.shape[0] // (d + 1)
    rng = np.random.default_rng(77)
    return gp.M, d, [st.random_lifted_point(rng, N, d, r)[:, :r].copy() for r in (d, d + 1, 2 * d)]


def tangent(rng, X, d):
    v = st.proj(X, rng.standard_normal(X.shape), d)
    return v / np.linalg.norm(v)


def test_gradient_is_the_central_difference_of_F(fixtures_dir):
    """<grad, v> against (F(retract(X, h v)) - F(retract(X, -h v))) / 2h within 1e-6 |<grad, v>| plus the difference's own
    floor, by the derivation of tests/test_polish_host.py (difference_floor): the truncation h^2 / 6 times the third derivative
    from the five-point stencil at H = 1e-2, doubled, and the fp64 rounding of the two retracted points u |X|_F |M X|_F / h; F
    itself in long double.  h = 1e-5, three seeded tangent directions per rank.  A gradient of the wrong sign has to fail."""
    M, d, pts = lifted_points(fixtures_dir)
    rng = np.random.default_rng(5)
    h, H = 1e-5, 1e-2
    for X in pts:
        g = st.grad(M, X, d)
        assert np.abs(st.sym(st.rot(g, d) @ st.rot(X, d).transpose(0, 2, 1))).max() <= 1e-12 * np.abs(g).max()   # tangent
        for _ in range(3):
            v = tangent(rng, X, d)
            phi = lambda t: float(tph.objective_ld(M, st.retract(X, t * v, d)))
            fd = (phi(h) - phi(-h)) / (2 * h)
            third = abs(phi(2 * H) - 2 * phi(H) + 2 * phi(-H) - phi(-2 * H)) / (2 * H ** 3)
            floor = 2.0 * h * h / 6.0 * third + U * float(np.linalg.norm(X)) * float(np.linalg.norm(M @ X)) / h
            gv = float(np.sum(g * v))
            print("rank %d: <g, v> %.9g, central difference %.9g, difference %.3g, floor %.3g" % (X.shape[1], gv, fd, abs(fd - gv), floor))
            assert abs(fd - gv) <= 1e-6 * abs(gv) + floor
            assert 2 * abs(gv) > 1e-6 * abs(gv) + floor   # (the check has its teeth: -g would fail)


def test_hessian_is_the_central_difference_of_the_projected_gradient(fixtures_dir):
    """Hess[V] against Proj_X((grad(retract(X, h V)) - grad(retract(X, -h V))) / 2h) in the Frobenius norm, within 1e-6 |Hess[V]|
    plus the difference's floor: the truncation from the same five-point stencil applied to the projected gradient (doubled),
    and the rounding of two gradient evaluations, whose entries are sums of at most k terms of |M| |X| -- M's product, and
    Lambda's, which is made of the same terms -- hence 2 (2 k u) | |M| |X| |_F / 2h."""
    M, d, pts = lifted_points(fixtures_dir)
    Mabs = abs(sp.csr_matrix(M))
    k = int(np.diff(sp.csr_matrix(M).indptr).max()) + 2 * d + 2
    rng = np.random.default_rng(6)
    h, H = 1e-5, 1e-2
    for X in pts:
        Lam = st.lambda_blocks(M, X, d)
        for _ in range(2):
            V = tangent(rng, X, d)
            gp = lambda t: st.proj(X, st.grad(M, st.retract(X, t * V, d), d), d)
            fd = (gp(h) - gp(-h)) / (2 * h)
            third = np.linalg.norm(gp(2 * H) - 2 * gp(H) + 2 * gp(-H) - gp(-2 * H)) / (2 * H ** 3)
            floor = 2.0 * h * h / 6.0 * third + 2 * (2 * k * U) * float(np.linalg.norm(Mabs @ np.abs(X))) / (2 * h)
            HV = st.hess(M, X, V, d, Lam)
            err = float(np.linalg.norm(fd - HV))
            print("rank %d: |Hess[V]| %.6g, |difference| %.3g, floor %.3g" % (X.shape[1], np.linalg.norm(HV), err, floor))
            assert err <= 1e-6 * np.linalg.norm(HV) + floor
            assert 2 * np.linalg.norm(HV) > 1e-6 * np.linalg.norm(HV) + floor


def test_retraction_is_orthonormal(fixtures_dir):
    M, d, pts = lifted_points(fixtures_dir)
    rng = np.random.default_rng(7)
    for X in pts:
        for scale in (1e-3, 1.0, 10.0):
            Z = st.retract(X, scale * tangent(rng, X, d) * np.sqrt(X.shape[0] // (d + 1)), d)
            Y = st.rot(Z, d)
            assert np.abs(Y @ Y.transpose(0, 2, 1) - np.eye(d)).max() <= 64 * U
        assert np.abs(st.retract(X, 0 * X, d) - X).max() <= 8 * U


# ---------------------------------------------------------------------------------------------------------------
# the four runs
# ---------------------------------------------------------------------------------------------------------------
# per input: the ranks visited and F at the end of each level, to the digits they were quoted with when the feature was asked
# for.  Those were measured with a plain Steihaug CG; the restatement of the reference's TNT (oracle.tnt) visits the same
# levels and ends each of them at the same value to every quoted digit, with and without the preconditioner, so the table stands
# as quoted.
TABLE = {
    ("ring12", 2): ([2, 3, 4], [32.4316954, 21.802377, 0.0037256496]),
    ("ring12", 3): ([3, 4, 5], [32.3270944, 16.082971, 0.0126937670]),
    ("tinyGrid3D", 3): ([3, 4], [42.2501320, 37.1686023]),
    ("smallGrid3D", 3): ([3], [None]),
}
_runs = {}


def table_start(fixtures_dir, name, d):
    if name == "ring12":
        gp, _, _, Xt, _ = ring12(d)
        return gp.M, Xt
    gp, X = tph.start_point(fixtures_dir, name, {"tinyGrid3D": 100, "smallGrid3D": 200}[name])
    if name == "tinyGrid3D":
        X = nr.polish(gp.M, X, d)[0]
    return gp.M, X


def table_run(fixtures_dir, name, d, pre):
    key = (name, d, pre)
    if key not in _runs:
        M, X = table_start(fixtures_dir, name, d)
        _runs[key] = (M, X, st.staircase(M, X, d, eta=ETA, precondition_on=pre, **st.TIGHT))
    return _runs[key]


def quoted(value, want):
    """`value` agrees with `want` to the digits `want` was quoted with (half a unit of its last digit)."""
    digits = len(("%r" % want).split(".")[1]) if "." in "%r" % want else 0
    return abs(value - want) <= 0.5 * 10.0 ** -digits + 1e-12


@pytest.mark.parametrize("pre", [True, False])
@pytest.mark.parametrize("name,d", list(TABLE))
def test_restatement_reproduces_the_table(fixtures_dir, name, d, pre):
    M, X, r = table_run(fixtures_dir, name, d, pre)
    ranks, Fs = TABLE[(name, d)]
    for L in r["levels"]:
        print("%s d=%d pre=%d: rank %d, F %.10g -> %.10g, |grad| %.3g, %d iterations, %d products, lambda_min %.6g, alpha %g" %
              (name, d, pre, L["rank"], L["F_in"], L["F"], L["grad"], L["iterations"], L["products"], L["lambda_min"], L["alpha"]))
    print("    sigma %s, F_rounded %.10g" % (np.array2string(r["sigma"], precision=4), r["F_rounded"]))
    assert r["outcome"] == st.SOLVED
    assert [L["rank"] for L in r["levels"]] == ranks
    for L, want in zip(r["levels"], Fs):
        if want is not None:
            assert quoted(L["F"], want), (L["F"], want)
    assert r["lambda_min"] >= -0.5 * ETA
    assert all(L["lambda_min"] < -0.5 * ETA for L in r["levels"][:-1])
    Y = st.rot(r["Y"], d)
    assert np.abs(Y @ Y.transpose(0, 2, 1) - np.eye(d)).max() <= 64 * U


@pytest.mark.parametrize("pre", [True, False])
@pytest.mark.parametrize("d", [2, 3])
def test_the_ring_reaches_the_certified_optimum(fixtures_dir, d, pre):
    """F of the rounded point is F of the polished chordal point, itself certified, within the weak-duality interval of the
    final lifted point plus the evaluation's rounding floor u |X|_F |M X|_F and the interval's own (weak_duality_interval's err:
    at the optimum M X is small and what is left is the rounding of the sums it is made of); the relaxation is tight: d singular values of
    sqrt(12), the others at rounding level."""
    gp, _, _, Xt, Xc = ring12(d)
    M, X, r = table_run(fixtures_dir, "ring12", d, pre)
    assert st.min_eigenpair(M, Xc, d)[0] >= -0.5 * ETA
    Fstar = st.objective(M, Xc)
    lo, hi, lam, err = st.weak_duality_interval(M, r["Y"], d, float(np.sum(Xc * Xc)))
    floor = U * float(np.linalg.norm(Xc)) * float(np.linalg.norm(M @ Xc)) + err
    print("ring12 d=%d: F* %.15g, interval [%.15g, %.15g], F_rounded %.15g, floor %.3g" % (d, Fstar, lo, hi, r["F_rounded"], floor))
    assert lo - floor <= Fstar <= hi + floor
    assert abs(r["F_rounded"] - Fstar) <= (hi - lo) + 2 * floor
    assert np.all(np.abs(r["sigma"][:d] - np.sqrt(12.0)) <= 1e-6) and np.all(r["sigma"][d:] <= 1e-6)
    Yh = st.rot(r["Xhat"], d)
    assert np.abs(Yh @ Yh.transpose(0, 2, 1) - np.eye(d)).max() <= 64 * U and np.all(np.linalg.det(Yh) > 0)


def test_tinygrid_is_a_lower_bound_not_a_better_point(fixtures_dir):
    """The relaxation is solved at rank 4 and is NOT tight: four singular values of order one; the rounded point is worse than
    the input and its polish returns to the input's value."""
    M, X, r = table_run(fixtures_dir, "tinyGrid3D", 3, True)
    print("tinyGrid3D: sigma %s, F_sdp %.9g, F_rounded %.6g" % (r["sigma"], r["F_sdp"], r["F_rounded"]))
    assert r["final_rank"] == 4 and r["sigma"][3] > 1.0
    assert quoted(r["F_sdp"], 37.1686023) and r["F_rounded"] > st.objective(M, X)
    back = nr.polish_full(M, r["Xhat"], 3)
    assert back["outcome"] == nr.CONVERGED and quoted(back["F_final"], 42.2501320)
    assert st.objective(M, X) - r["F_sdp"] > 5.0


def test_round_solution_undoes_a_reflection():
    gp, _, _, Xt, _ = ring12(3)
    for Xin in (Xt, Xt * np.array([1.0, 1.0, -1.0])):
        Xh, B, sigma = st.round_solution(st.lift(Xin, 3), 3)
        Q = np.linalg.lstsq(Xt, Xh, rcond=None)[0]
        assert np.abs(Q @ Q.T - np.eye(3)).max() <= 1e-12 and np.abs(Xt @ Q - Xh).max() <= 1e-12
        assert np.all(np.linalg.det(st.rot(Xh, 3)) > 0)


# ---------------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------------
def test_staircase_abi():
    o = dpgo_amd.StaircaseOptions()
    assert (o.grad_norm_tol, o.preconditioned_grad_norm_tol, o.rel_func_decrease_tol, o.stepsize_tol) == (1e-2, 1e-4, 1e-6, 1e-3)
    assert (o.max_iterations, o.max_tCG_iterations, o.STPCG_kappa, o.STPCG_theta) == (1000, 10000, 0.1, 0.5)
    assert (o.r_max, o.precondition, o.polish, o.min_eig_num_tol, o.max_factor_bytes) == (0, 1, 1, 1e-3, 0)
    for k, v in st.DEFAULTS.items():
        assert getattr(o, k) == v
    assert (dpgo_amd.STAIR_SOLVED, dpgo_amd.STAIR_MAX_RANK, dpgo_amd.STAIR_SADDLE, dpgo_amd.STAIR_SKIPPED) == (0, 1, 2, 3)
    assert (st.SOLVED, st.MAX_RANK, st.SADDLE, st.SKIPPED) == (0, 1, 2, 3)
    # four doubles, two ints, two doubles, four ints, a double, a long long; eight ints, seven doubles, six, a long long, four
    assert C.sizeof(dpgo_amd.StaircaseOptions) == 32 + 8 + 16 + 16 + 8 + 8
    assert C.sizeof(dpgo_amd.StaircaseResult) == 32 + 56 + 48 + 8 + 32
    L = dpgo_amd.lib()
    X = np.full((8, 6), 7.0, order="F")
    keep = X.copy()
    dp = X.ctypes.data_as(C.POINTER(C.c_double))
    r = dpgo_amd.StaircaseResult()
    sent = bytes(r)
    fake = C.c_void_p(0)
    f = C.c_double(3.0)
    for grp in (None, fake):
        assert L.dpgo_group_staircase(grp, dp, 8, C.byref(o), 0, dp, 8, dp, 8, None, 0, C.byref(r)) == -1
        assert L.dpgo_group_stair_eval(grp, dp, 8, C.byref(f), C.byref(f), None, None, 0) == -1
        assert L.dpgo_group_stair_hess(grp, dp, 8, dp, 8, dp, 8) == -1
        assert L.dpgo_group_stair_retract(grp, dp, 8, dp, 8, dp, 8) == -1
        assert L.dpgo_group_stair_round(grp, dp, 8, dp, dp, dp, 8) == -1
    assert np.array_equal(X, keep) and bytes(r) == sent and f.value == 3.0   # (nothing touched)
    L.dpgo_staircase_options_default(None)   # (no crash)
    header = open(os.path.join(os.path.dirname(dpgo_amd.__file__), "..", "include", "dpgo_amd.h")).read()
    for sym in ("dpgo_staircase_options_default", "dpgo_group_staircase", "dpgo_group_stair_eval", "dpgo_group_stair_hess",
                "dpgo_group_stair_retract", "dpgo_group_stair_round"):
        assert sym + "(" in header and sym in dpgo_amd.SYMBOLS and hasattr(L, sym)
    with pytest.raises(TypeError):
        dpgo_amd.StaircaseOptions(no_such_field=1)


def test_twisted_ring_generator():
    """The instance is what the issue defines: the noise draws per edge in edge order (rotation first), kappa = tau = 10, the
    start with the true translations and one extra turn of the heading."""
    for d in (2, 3):
        g, X = synthetic.twisted_ring(d, 12, 0.02, 1, 1)
        rng = np.random.default_rng(1)
        ang = 2 * np.pi * np.arange(12) / 12
        for e in range(12):
            rot_draw = rng.standard_normal() if d == 2 else rng.standard_normal((1, 3))[0]
            tr_draw = rng.standard_normal(d)
            true_t = np.zeros(d)
            # R_k^T (t_{k+1} - t_k) in the plane: the chord, seen from pose k
            c = 12 / (2 * np.pi) * np.array([np.cos(ang[(e + 1) % 12]) - np.cos(ang[e]), np.sin(ang[(e + 1) % 12]) - np.sin(ang[e])])
            true_t[0] = np.cos(ang[e]) * c[0] + np.sin(ang[e]) * c[1]
            true_t[1] = -np.sin(ang[e]) * c[0] + np.cos(ang[e]) * c[1]
            assert np.abs(g["t"][e] - true_t - 0.02 * tr_draw).max() <= 1e-14
            assert abs(np.linalg.det(g["R"][e]) - 1) <= 1e-14
            if d == 2:
                a = 2 * np.pi / 12 + 0.02 * rot_draw
                assert np.abs(g["R"][e] - np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])).max() <= 1e-14
        assert (g["I"] == np.arange(12)).all() and (g["J"] == (np.arange(12) + 1) % 12).all()
        assert (g["kappa"] == 10).all() and (g["tau"] == 10).all() and g["num_poses"] == 12
        assert np.abs(np.linalg.norm(X[:12], axis=1) - 12 / (2 * np.pi)).max() <= 1e-14
        Y = st.rot(X, d)   # Y_k = R_k^T: the heading turns by twice the angle of the position
        assert abs(Y[3][0, 0] - np.cos(2 * ang[3])) <= 1e-14 and abs(Y[3][0, 1] - np.sin(2 * ang[3])) <= 1e-14
