"""Host side of the Newton polish (dpgo_amd/csrc/polish.h): the numpy restatement of the rule (tests/newton_restatement.py)
against the trajectories measured when the feature was asked for, its gradient against central differences of F along the
retraction, the vector-solve hook on the host (spd_solve_host through dpgo_amd.spd_vsolve_debug(host=True)) against the
long-double solve within tests/solve_restatement.py's bound, and the argument checks of the C ABI.  No GPU.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_restatement as cr  # noqa: E402
import factor_restatement as fr  # noqa: E402
import newton_restatement as nr  # noqa: E402
import solve_restatement as sr  # noqa: E402
import test_certify_host as tch  # noqa: E402  (its points; none of its tests is imported)
import test_gpu_cert_proof as tp  # noqa: E402  (the d = 2 graph; none of its tests is imported)

import dpgo_amd  # noqa: E402
from oracle import g2o as og  # noqa: E402
from oracle.hash import Options as OOptions  # noqa: E402
from oracle.problem import LOSS_NONE  # noqa: E402
from oracle.star import DistPGO as ODistPGO, chordal_initialization  # noqa: E402

U = 2.0 ** -53

# ---------------------------------------------------------------------------------------------------------------
# the restatement: every row of the table the rule was chosen on (anchor 0, the defaults)
# ---------------------------------------------------------------------------------------------------------------
# (input, start) -> outcome, accepted steps, factorisations, indefinite, |g| first, |g| last (two digits)
TABLE = {
    ("tinyGrid3D", "chordal"): (nr.CONVERGED, 8, 10, 1, 90.0, 4e-13),
    ("tinyGrid3D", 10): (nr.CONVERGED, 4, 4, 0, 0.63, 2e-13),
    ("tinyGrid3D", 100): (nr.CONVERGED, 1, 1, 0, 2.6e-4, 5e-8),
    ("tinyGrid3D", "random"): (nr.MAX_STEPS, 20, 34, 1, 668.0, 0.08),
    ("smallGrid3D", "chordal"): (nr.CONVERGED, 7, 8, 0, 335.0, 9e-9),
    ("smallGrid3D", 20): (nr.CONVERGED, 2, 2, 0, 0.30, 2.7e-10),
    ("smallGrid3D", 200): (nr.CONVERGED, 1, 1, 0, 1.5e-6, 2.3e-12),
    ("ladder2", 50): (nr.CONVERGED, 10, 11, 0, 117.0, 6e-8),
    ("ladder2", 300): (nr.CONVERGED, 2, 2, 0, 0.26, 7e-7),
}
_starts = {}


def start_point(fixtures_dir, name, which):
    """(GlobalProblem, X): the chordal point, the oracle's AMM-PGO# iterate after `which` iterations on its nodes (LOSS_NONE,
    driver options), or the chordal point with every rotation replaced by a seeded random one."""
    key = (name, which)
    if key not in _starts:
        if name == "ladder2":
            g, N, mm, gp, X0, nn = tp.ladder2()
            path = None
        else:
            gp, X0, Xc = tch.points(fixtures_dir, name)
            path = os.path.join(fixtures_dir, name + ".g2o")
            N, mm = og.read_g2o_file(path)
            nn = 2
        if which == "chordal":
            X = X0
        elif which == "random":
            X = cr.random_rotations_point(X0, gp.d, 5)
        elif name != "ladder2" and which == tch.ITERS[name]:
            X = Xc
        else:
            drv = ODistPGO(path, nn, OOptions.driver(LOSS_NONE, True), X0=X0, mm=mm, num_poses=N)
            drv.run(which, evaluate=False)
            X = np.array(drv.gather())
        _starts[key] = (gp, X)
    return _starts[key]


def orthogonality(X, d):
    N = X.shape[0] // (d + 1)
    Y = X[N:].reshape(N, d, d)
    return float(np.abs(Y @ np.transpose(Y, (0, 2, 1)) - np.eye(d)).max())


@pytest.mark.parametrize("name,which", list(TABLE))
def test_restatement_reproduces_the_table(fixtures_dir, name, which):
    gp, X = start_point(fixtures_dir, name, which)
    d = gp.d
    N = X.shape[0] // (d + 1)
    r = nr.polish_full(gp.M, X, d, anchor=0)
    Xn, outcome, steps, factorisations, indefinite, log = nr.polish(gp.M, X, d, anchor=0)
    assert (outcome, steps, factorisations, indefinite) == (r["outcome"], r["steps"], r["factorisations"], r["indefinite"])
    assert np.array_equal(Xn, r["X"]) and np.array_equal(log, r["log"])
    want = TABLE[(name, which)]
    print("%s %s: outcome %d, %d steps, %d factorisations, %d indefinite, |g| %.3g -> %.3g, F %.6g -> %.6g" %
          (name, which, outcome, steps, factorisations, indefinite, r["grad_initial"], r["grad_final"], r["F_initial"], r["F_final"]))
    assert (outcome, steps, factorisations, indefinite) == want[:4]
    # the table's |g| are quoted to two digits
    assert abs(r["grad_initial"] - want[4]) <= 0.05 * want[4]
    if outcome == nr.CONVERGED:
        assert r["grad_final"] <= nr.DEFAULTS["rel_tol"] * r["hmax"]
        assert 0.2 * want[5] <= r["grad_final"] <= 5 * want[5]    # (the floor is rounding: its digits are not held)
    else:
        assert abs(r["grad_final"] - want[5]) <= 0.05 * want[5]
        assert abs(r["F_initial"] - 1483.0) <= 1.0 and abs(r["F_final"] - 42.25) <= 0.01
    F = log[:, 0]
    for k in range(len(F) - 1):
        assert F[k + 1] <= F[k] or r["rounding"][k], (k, F[k], F[k + 1])
    assert int(log[:, 4].sum()) == factorisations and len(log) == steps + 1
    # the anchor's record bit for bit, the rotations orthogonal
    assert np.array_equal(Xn[0], X[0]) and np.array_equal(Xn[N:N + d], X[N:N + d])
    assert orthogonality(Xn, d) <= 64 * U


_Mld = {}


def objective_ld(M, Z):
    """F = 1/2 <Z, M Z> in long double (M dense): the evaluation's own rounding is 2 000 times below fp64's."""
    if id(M) not in _Mld:
        _Mld[id(M)] = np.asarray(sp.csr_matrix(M).toarray(), cr.LD)
    Zl = np.asarray(Z, cr.LD)
    return 0.5 * np.sum(Zl * (_Mld[id(M)] @ Zl))


def difference_floor(M, X, d, v, h):
    """What the central difference of F along retract(X, t v) with step h carries whatever the gradient is -- derived from F
    and X alone, nothing of `grad`.  F is evaluated in long double, so what is left is (a) the truncation h^2 / 6 times the
    third derivative, taken from the five-point stencil at H = 1e-2 and doubled for that estimate's own error, and (b) the
    fp64 rounding of the two retracted points themselves: entries off by u |Z| move F by at most u |Z|_F |M Z|_F each,
    hence u |X|_F |M X|_F / h in the quotient."""
    phi = lambda t: float(objective_ld(M, cr.retract(X, t * v, d)))
    H = 1e-2
    third = abs(phi(2 * H) - 2 * phi(H) + 2 * phi(-H) - phi(-2 * H)) / (2 * H ** 3)
    return 2.0 * h * h / 6.0 * third + U * float(np.linalg.norm(X)) * float(np.linalg.norm(M @ X)) / h


@pytest.mark.parametrize("name", ["tinyGrid3D", "smallGrid3D"])
@pytest.mark.parametrize("which", ["chordal", "early", "converged"])
def test_gradient_is_the_central_difference_of_F(fixtures_dir, name, which):
    """g'v against (F(retract(X, h v)) - F(retract(X, -h v))) / 2h within 1e-6 |g'v| plus the difference's own floor
    (difference_floor: derived from F, it knows nothing of the gradient; F itself in long double), five seeded directions, h = 1e-5, at the chordal
    point, after 10 / 20 iterations and at the converged point.  Away from the critical point the floor must leave the check
    its teeth: a gradient of the wrong sign (an error of 2 |g'v|) has to fail on at least three of the five directions.  At
    the converged points |g| is 2.6e-4 and 1.5e-6 and the test prints on how many directions it could still tell g from -g."""
    its = {"chordal": "chordal", "early": {"tinyGrid3D": 10, "smallGrid3D": 20}[name], "converged": tch.ITERS[name]}[which]
    gp, X = start_point(fixtures_dir, name, its)
    d = gp.d
    g = nr.grad(gp.M, X, d)
    rng = np.random.default_rng(23)
    h = 1e-5
    told = 0
    for _ in range(5):
        v = rng.standard_normal(len(g))
        v /= np.linalg.norm(v)
        fd = float((objective_ld(gp.M, cr.retract(X, h * v, d)) - objective_ld(gp.M, cr.retract(X, -h * v, d))) / (2 * h))
        gv = float(g @ v)
        floor = difference_floor(gp.M, X, d, v, h)
        tol = 1e-6 * abs(gv) + floor
        told += 2 * abs(gv) > tol
        print("%s %s: g'v %.9g, central difference %.9g, difference %.3g, floor %.3g" % (name, which, gv, fd, abs(fd - gv), floor))
        assert abs(fd - gv) <= tol
    print("%s %s: a gradient of the wrong sign would have failed on %d of 5 directions" % (name, which, told))
    if which != "converged" or name == "tinyGrid3D":
        assert told >= 3
    ga = nr.grad(gp.M, X, d, anchor=0)
    dof = cr.dof_of(d)
    assert not ga[:dof].any() and np.array_equal(ga[dof:], g[dof:])


# ---------------------------------------------------------------------------------------------------------------
# the vector-solve hook on the host
# ---------------------------------------------------------------------------------------------------------------
INPUTS = ["arrow_wide", "arrow_tall", "arrow_edges", "arrow_edges_lap", "nested", "arrow_block4"]
_refs = {}


def rhs_of(name, second=False):
    n = fr.build_input(name)[0].shape[0]
    return np.random.default_rng(977 + 31 * INPUTS.index(name) + (7 if second else 0)).standard_normal(n)


def reference(name, second=False):
    """(x_ref in long double, the bound BOUND_C kappa_1 u |x_ref|_1) of an input of factor_restatement and rhs_of: once."""
    key = (name, second)
    if key not in _refs:
        A = fr.build_input(name, second=second)[0]
        ref = sr.ComponentReference(A)
        Xref = sr.solve_cholesky_ld(ref.A, rhs_of(name)[:, None])
        _refs[key] = (Xref[:, 0], float(ref.bound(Xref)[0]))
    return _refs[key]


def ratio(x, name, second=False):
    xref, bnd = reference(name, second)
    return float(np.abs(np.asarray(x, sr.LD) - xref).sum()) / bnd


def vsolve(name, host, second=False, refactor=False, csr=None, chunk=None):
    spec = fr.INPUTS[name]
    if csr is None:
        csr = fr.build_input(name, second=second)[1]
    values2 = fr.build_input(name, second=True)[1].data if refactor else None
    return dpgo_amd.spd_vsolve_debug(csr, rhs_of(name), spec["leaf"], spec["collapse"], spec["block"], host=host,
                                     refactor_values=values2, chunk=chunk)


def planted_pivot(name="arrow_wide"):
    """arrow_wide with -1 on the first pivot of its 5-wide leaf (tests/test_covariance_host.py): a non-positive pivot whatever
    the arithmetic."""
    spec = fr.INPUTS[name]
    good = dpgo_amd.spd_selinv_debug(fr.build_input(name)[1], spec["leaf"], spec["collapse"], spec["block"], host=True)
    s = int(np.flatnonzero(good["w"] == 5)[0])
    v = int(good["piv_idx"][s][0])
    B = fr.build_input(name)[0].copy()
    B[v, v] = -1.0
    return fr.to_csr(B, spec["pattern"]())


def untouched(a):
    return bool(np.all(sr.bits(a) == sr.bits(np.array([sr.SENT_OUT]))[0]))


@pytest.mark.parametrize("name", INPUTS)
def test_host_solve_against_the_long_double_solve(name):
    res = vsolve(name, host=True)
    assert res["status"] == 0 and not res["on_device"]
    r = ratio(res["out"], name)
    print("%s: host %.3g of the bound" % (name, r))
    assert r < 1.0, (name, r)
    assert np.array_equal(sr.bits(res["out"]), sr.bits(res["out_again"]))
    assert untouched(res["raw"][2 * len(res["out"]):])   # (no second values: the third part is not written)


def test_host_refactorisation_gives_the_bits_of_a_fresh_handle():
    name = "nested"
    kept = vsolve(name, host=True, refactor=True)
    fresh = vsolve(name, host=True, second=True)
    assert kept["status2"] == 0 and fresh["status"] == 0
    assert np.array_equal(sr.bits(kept["out2"]), sr.bits(fresh["out"]))
    assert not np.array_equal(sr.bits(kept["out2"]), sr.bits(kept["out"]))
    assert ratio(kept["out2"], name, second=True) < 1.0


def test_host_planted_pivot_solves_nothing():
    res = vsolve("arrow_wide", host=True, csr=planted_pivot())
    assert res["status"] == 1 and res["out"] is None and untouched(res["raw"])


def test_vsolve_bad_arguments_return_minus_one():
    L = dpgo_amd.lib()
    _, csr = fr.build_input("arrow_edges")
    n = csr.shape[0]
    ptr, col, val = csr.indptr.astype(np.int32), csr.indices.astype(np.int32), csr.data.astype(np.float64)
    b, out, status, piv = np.ones(n), np.zeros(3 * n), np.zeros(2, np.int32), np.zeros(4)
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))

    def call(n_=n, ptr_=ptr, col_=col, val_=val, leaf=64, collapse=1, block=1, rhs_=b, out_=out, status_=status, piv_=piv):
        return L.dpgo_debug_spd_vsolve(n_, ip(ptr_), ip(col_), dp(val_), None, leaf, collapse, block, 1, dp(rhs_), dp(out_),
                                       ip(status_), dp(piv_))

    assert call() == 0
    assert call(ptr_=None) == -1 and call(col_=None) == -1 and call(val_=None) == -1
    assert call(rhs_=None) == -1 and call(out_=None) == -1 and call(status_=None) == -1 and call(piv_=None) == -1
    assert call(n_=0) == -1 and call(n_=-3) == -1
    assert call(leaf=0) == -1 and call(block=0) == -1 and call(collapse=-1) == -1
    assert call(block=7) == -1                       # n is no multiple of the block
    bad = col.copy()
    bad[5] = n
    assert call(col_=bad) == -1
    bad = ptr.copy()
    bad[3] = bad[2] - 1
    assert call(ptr_=bad) == -1


# ---------------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------------
def test_polish_abi():
    o = dpgo_amd.PolishOptions()
    assert (o.max_steps, o.max_tries, o.rel_tol, o.grad_tol, o.anchor) == (20, 8, 1e-9, 0.0, 0)
    assert (dpgo_amd.POLISH_CONVERGED, dpgo_amd.POLISH_MAX_STEPS, dpgo_amd.POLISH_STALLED, dpgo_amd.POLISH_SKIPPED) == (0, 1, 2, 3)
    assert (nr.CONVERGED, nr.MAX_STEPS, nr.STALLED, nr.SKIPPED) == (0, 1, 2, 3)
    assert (nr.DEFAULTS["max_steps"], nr.DEFAULTS["max_tries"], nr.DEFAULTS["rel_tol"], nr.DEFAULTS["grad_tol"]) == (20, 8, 1e-9, 0.0)
    # two ints, two doubles, an int (padded to 8); four ints, eight doubles, four ints, a long long, five doubles
    assert C.sizeof(dpgo_amd.PolishOptions) == 32
    assert C.sizeof(dpgo_amd.PolishResult) == 16 + 64 + 16 + 8 + 40
    L = dpgo_amd.lib()
    X = np.zeros((8, 3), order="F")
    dp = X.ctypes.data_as(C.POINTER(C.c_double))
    r = dpgo_amd.PolishResult()
    fake = C.c_void_p(0)
    assert L.dpgo_group_polish(None, dp, 8, C.byref(o), 0, dp, 8, None, 0, C.byref(r)) == -1
    assert L.dpgo_group_polish(fake, dp, 8, C.byref(o), 0, dp, 8, None, 0, C.byref(r)) == -1
    L.dpgo_polish_options_default(None)   # (no crash)
    header = open(os.path.join(os.path.dirname(dpgo_amd.__file__), "..", "include", "dpgo_amd.h")).read()
    assert L.dpgo_debug_spd_vsolve_chunk(64) == 2048 and L.dpgo_debug_spd_vsolve_chunk(0) == 64   # (out of range: the default)
    assert L.dpgo_debug_spd_vsolve_chunk(4096) == 2048 and L.dpgo_debug_spd_vsolve_chunk(2048) == 2048
    for sym in ("dpgo_polish_options_default", "dpgo_group_polish", "dpgo_debug_spd_vsolve", "dpgo_debug_spd_vsolve_chunk"):
        assert sym + "(" in header and sym in dpgo_amd.SYMBOLS and hasattr(L, sym)
    with pytest.raises(TypeError):
        dpgo_amd.PolishOptions(no_such_field=1)
