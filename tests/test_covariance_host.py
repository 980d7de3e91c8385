"""Selected inversion on the host (spd_selinv_host through dpgo_amd.spd_selinv_debug(host=True)) against the dense
long-double inverse, on the inputs of tests/factor_restatement.py (imported, not edited): fronts with w = 1 ... 300, u = 0,
u > w, three tree levels, four trees side by side, unknowns in groups of four.

The bound is tests/cov_restatement.py's  C u kappa_2(A) ||A^-1||_2  per entry.  It is fixed on the CPU, before any device is
asked: test_bound_leaves_the_restatement_a_quarter holds the plain fp64 restatement of the recursion within a quarter of
it, and the long-double restatement far below (which shows that what is left is rounding, not the recursion).  The host
twin's index maps -- child update rows to parent positions, read the other way than the assembly reads them -- are what
these tests check on a machine without a GPU.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_restatement as cr  # noqa: E402
import factor_restatement as fr  # noqa: E402

import dpgo_amd  # noqa: E402

INPUTS = ["arrow_wide", "arrow_tall", "arrow_edges", "arrow_edges_lap", "nested", "arrow_block4"]

_host = {}


def host_result(name, refactor=False):
    key = (name, refactor)
    if key not in _host:
        spec = fr.INPUTS[name]
        _, csr = fr.build_input(name)
        second = fr.build_input(name, second=True)[1].data if refactor else None
        _host[key] = dpgo_amd.spd_selinv_debug(csr, spec["leaf"], spec["collapse"], spec["block"], host=True,
                                               refactor_values=second)
    return _host[key]


@pytest.mark.parametrize("name", INPUTS)
def test_bound_leaves_the_restatement_a_quarter(name):
    res = host_result(name)
    ref, Sref, bnd = cr.reference(name, res)
    r64 = cr.worst_ratio(res, cr.recursion(res, ref.W_fp64, np.float64), Sref, bnd)
    rld = cr.worst_ratio(res, cr.recursion(res, ref.W, cr.LD), Sref, bnd)
    print("%s: kappa_2 %.3g, bound %.3g, restatement fp64 %.3g, long double %.3g of the bound" % (name, ref.kappa, bnd, r64, rld))
    assert r64 <= 0.25, (name, r64)
    assert rld <= 0.25 / 500, (name, rld)   # (long double: eps 2 000 times below fp64)


@pytest.mark.parametrize("name", INPUTS)
def test_host_twin_against_the_long_double_inverse(name):
    res = host_result(name)
    assert res["status"] == 0 and res["selinv_status"] == 0 and not res["on_device"]
    fr.check_structure(dict(res, height=_heights(res), ldw=res["w"], ldm=res["w"] + res["u"], w_off=_offs(res, "w"),
                            wt_off=_offs(res, "wt")), fr.build_input(name)[0].shape[0])
    ref, Sref, bnd = cr.reference(name, res)
    ratio = cr.worst_ratio(res, res["sigma"], Sref, bnd)
    print("%s: host twin %.3g of the bound" % (name, ratio))
    assert ratio < 1.0, (name, ratio)
    assert cr.symmetric_bits(res["sigma"])            # both triangles are stored from one product
    assert cr.same_bits(res["sigma"], res["sigma_again"])


def _heights(res):
    h = np.zeros(res["nfronts"], np.int64)
    for s in range(res["nfronts"]):
        if res["parent"][s] >= 0:
            h[res["parent"][s]] = max(h[res["parent"][s]], h[s] + 1)
    return h


def _offs(res, which):
    w, u = res["w"].astype(np.int64), res["u"].astype(np.int64)
    sizes = (w + u) * w
    return np.concatenate([[0], np.cumsum(sizes)])[:-1]


def test_host_twin_after_a_refactorisation():
    """Second values (another seed, the diagonal times 3) through spd_refactor: the blocks of a fresh handle on them."""
    name = "nested"
    spec = fr.INPUTS[name]
    kept = host_result(name, refactor=True)
    fresh = dpgo_amd.spd_selinv_debug(fr.build_input(name, second=True)[1], spec["leaf"], spec["collapse"], spec["block"], host=True)
    assert kept["status2"] == 0 and kept["selinv_status2"] == 0
    assert cr.same_bits(kept["sigma2"], fresh["sigma"])
    assert not cr.same_bits(kept["sigma2"], kept["sigma"])


def test_a_non_positive_pivot_is_not_inverted():
    """The first pivot of the 5-wide leaf of arrow_wide is its own diagonal entry: set to -1 it is the first non-positive
    pivot whatever the arithmetic."""
    name = "arrow_wide"
    spec = fr.INPUTS[name]
    good = host_result(name)
    s = int(np.flatnonzero(good["w"] == 5)[0])
    v = int(good["piv_idx"][s][0])
    A, _ = fr.build_input(name)
    B = A.copy()
    B[v, v] = -1.0
    res = dpgo_amd.spd_selinv_debug(fr.to_csr(B, spec["pattern"]()), spec["leaf"], spec["collapse"], spec["block"], host=True)
    assert res["status"] == 1 and res["selinv_status"] == 1
    assert res["sigma"] is None and res["sigma_again"] is None


def test_bad_arguments_return_minus_one():
    L = dpgo_amd.lib()
    _, csr = fr.build_input("arrow_edges")
    n = csr.shape[0]
    ptr, col, val = csr.indptr.astype(np.int32), csr.indices.astype(np.int32), csr.data.astype(np.float64)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))

    def call(n_=n, ptr_=ptr, col_=col, val_=val, leaf=64, collapse=1, block=1, out=True):
        h = C.c_void_p()
        rc = L.dpgo_debug_spd_selinv(n_, None if ptr_ is None else ip(ptr_), None if col_ is None else ip(col_),
                                     None if val_ is None else dp(val_), None, leaf, collapse, block, 1,
                                     C.byref(h) if out else None)
        assert rc != 0 and not h.value
        return rc

    assert call(out=False) == -1
    assert call(ptr_=None) == -1 and call(col_=None) == -1 and call(val_=None) == -1
    assert call(n_=0) == -1 and call(n_=-3) == -1
    assert call(leaf=0) == -1 and call(block=0) == -1 and call(collapse=-1) == -1
    assert call(block=7) == -1                       # n is no multiple of the block
    bad = col.copy()
    bad[5] = n
    assert call(col_=bad) == -1
    bad = ptr.copy()
    bad[3] = bad[2] - 1
    assert call(ptr_=bad) == -1
    assert L.dpgo_debug_spd_selinv_get(None, None, None, None, None, None, None, None, None, None, None, None) == -1
    L.dpgo_debug_spd_selinv_free(None)


# ---------------------------------------------------------------------------------------------------------------
# the matrix: the restated tangent-space Hessian at the converged points of tests/test_certify_host.py
# ---------------------------------------------------------------------------------------------------------------
import cert_restatement as cert  # noqa: E402
import test_certify_host as tch  # noqa: E402  (its converged points; none of its tests is imported)

_H = {}


def restated(fixtures_dir, name):
    """(GlobalProblem, converged X, H, ||H||_2) from the oracle's M."""
    if name not in _H:
        gp, _, Xc = tch.points(fixtures_dir, name)
        H = cr.hessian(cert.S_matrix(gp.M, Xc, gp.d), Xc, gp.d)
        _H[name] = (gp, Xc, H, float(np.linalg.norm(H, 2)))
    return _H[name]


@pytest.mark.parametrize("name", ["tinyGrid3D", "smallGrid3D"])
def test_restated_hessian_is_symmetric_and_the_second_difference_of_F(fixtures_dir, name):
    gp, X, H, nH = restated(fixtures_dir, name)
    d = gp.d
    assert np.max(np.abs(H - H.T)) <= 1e-12 * nH
    M = gp.M
    F = lambda Z: 0.5 * float(np.sum(Z * (M @ Z)))
    rng = np.random.default_rng(11)
    h = 1e-4
    for _ in range(5):
        v = rng.standard_normal(H.shape[0])
        v /= np.linalg.norm(v)
        fd = (F(cr.retract(X, h * v, d)) - 2.0 * F(X) + F(cr.retract(X, -h * v, d))) / (h * h)
        q = float(v @ H @ v)
        print("%s: v'Hv %.9g, second difference %.9g, relative %.2e" % (name, q, fd, abs(fd - q) / abs(q)))
        assert abs(fd - q) <= 1e-5 * abs(q)


# smallest / largest eigenvalue of the anchored H (anchor 0) at the converged points, as the issue that asked for the feature
# measured them with a script of its own
ANCHORED_SPECTRUM = {"tinyGrid3D": (0.459, 659.0), "smallGrid3D": (0.078, 1177.0)}


@pytest.mark.parametrize("name", ["tinyGrid3D", "smallGrid3D"])
def test_gauge_directions_and_the_anchor(fixtures_dir, name):
    """H has exactly dof eigenvalues below 1e-4 ||H||_2 -- the gauge: a rigid motion of all poses -- and none below
    -1e-4 ||H||_2; anchored at pose 0 or at pose N - 1 it is positive definite.  Its extreme eigenvalues at anchor 0 are
    held to the independently measured ones within 2 %.  (Not asserted: "no eigenvalue below 1e-4 ||H||_2 after anchoring".
    The measured spectrum itself rules that out on smallGrid3D, 0.078 < 1e-4 * 1177 = 0.118; the gauge eigenvalues are below
    1e-7 ||H||_2, so the smallest anchored eigenvalue is orders of magnitude above them all the same.)"""
    gp, X, H, nH = restated(fixtures_dir, name)
    dof = cr.dof_of(gp.d)
    lam = np.linalg.eigvalsh(H)
    assert int(np.sum(np.abs(lam) < 1e-4 * nH)) == dof and lam[0] > -1e-4 * nH
    assert np.max(np.abs(lam[:dof])) < 1e-7 * nH   # (not exactly zero: the points are converged to |grad F| = 2e-4 and 1e-6)
    la = np.linalg.eigvalsh(cr.anchored(H, 0, dof))
    lo, hi = ANCHORED_SPECTRUM[name]
    print("%s: anchored spectrum %.4g ... %.5g, kappa_2 %.3g" % (name, la[0], la[-1], la[-1] / la[0]))
    assert abs(la[0] - lo) <= 0.02 * lo and abs(la[-1] - hi) <= 0.02 * hi
    assert np.linalg.eigvalsh(cr.anchored(H, gp.num_poses - 1, dof))[0] > 1e3 * np.max(np.abs(lam[:dof]))


@pytest.mark.parametrize("name", ["tinyGrid3D", "smallGrid3D"])
def test_the_point_with_random_rotations_is_no_minimum(fixtures_dir, name):
    """The point tests/test_gpu_covariance.py expects COV_NOT_PD at: an eigenvalue below -1e-3 ||H||_2 after anchoring."""
    gp, X, _, _ = restated(fixtures_dir, name)
    Z = cr.random_rotations_point(X, gp.d, 5)
    H = cr.anchored(cr.hessian(cert.S_matrix(gp.M, Z, gp.d), Z, gp.d), 0, cr.dof_of(gp.d))
    lam = np.linalg.eigvalsh(H)
    print("%s: lambda_min / ||H||_2 = %.3g" % (name, lam[0] / max(abs(lam[0]), abs(lam[-1]))))
    assert lam[0] < -1e-3 * max(abs(lam[0]), abs(lam[-1]))


def test_covariance_null_arguments():
    L = dpgo_amd.lib()
    X = np.zeros((8, 3), order="F")
    dp = X.ctypes.data_as(C.POINTER(C.c_double))
    r = dpgo_amd.CovResult()
    nnz = C.c_longlong(0)
    fake = C.c_void_p(0)
    assert L.dpgo_group_covariance(None, dp, 8, 0, 0, None, 0, dp, None, C.byref(r)) == -1
    assert L.dpgo_group_covariance(fake, dp, 8, 0, 0, None, 0, dp, None, C.byref(r)) == -1
    assert L.dpgo_group_cov_hessian(None, dp, 8, 0, None, None, None, 0, C.byref(nnz)) == -1
    assert L.dpgo_graph_covariance_reweighted(None, 0, dp, 8, 0, 0.25, 0, 0, None, 0, dp, None, C.byref(r), None) == -1
    assert (dpgo_amd.COV_OK, dpgo_amd.COV_NOT_PD, dpgo_amd.COV_SKIPPED) == (0, 1, 2)
