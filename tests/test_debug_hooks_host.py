"""The CSR reader of the test hooks (capi_debug.cpp: read_csr), through every hook that takes a matrix and runs without a
device: a malformed matrix is refused with -1 before anything is written, a well-formed one goes through with host=1.
dpgo_debug_spd_solver_create is not here: it answers -2 without a device before it reads the matrix."""
import ctypes as C

import numpy as np
import pytest

import dpgo_amd
from dpgo_amd import _dp, _ip

N, LEAF, COLLAPSE, BLOCK = 4, 2, 1, 1
PTR = np.array([0, 2, 5, 8, 10], np.int32)                      # the 4 x 4 tridiagonal (-1, 4, -1)
COL = np.array([0, 1, 0, 1, 2, 1, 2, 3, 2, 3], np.int32)
VAL = np.array([4, -1, -1, 4, -1, -1, 4, -1, -1, 4], np.float64)
UNTOUCHED = -7.0                                                # what the output arrays hold before a call


def _malformed():
    ptr1, down, col_n = PTR.copy(), PTR.copy(), COL.copy()
    ptr1[0] = 1
    down[2] = 1                                                 # 0 2 1 8 10
    col_n[4] = N
    return {"n = 0": (0, PTR, COL, VAL), "ptr[0] = 1": (N, ptr1, COL, VAL), "decreasing ptr": (N, down, COL, VAL),
            "col = n": (N, PTR, col_n, VAL), "null val": (N, PTR, COL, None)}


CASES = dict(_malformed(), **{"well-formed": (N, PTR, COL, VAL)})


def _csr(case):
    n, ptr, col, val = CASES[case]
    return n, _ip(ptr), _ip(col), None if val is None else _dp(val)


# each hook: case -> (rc, the outputs it was handed, the handle it gave out or None)
def _solve(case):
    X = np.full((N, 2), UNTOUCHED)
    return dpgo_amd.lib().dpgo_debug_spd_solve(*_csr(case), _dp(X), 2, LEAF), [X], None


def _stats(case):
    nnz, lv, mf = C.c_long(-7), C.c_int(-7), C.c_int(-7)
    rc = dpgo_amd.lib().dpgo_debug_spd_stats(*_csr(case), LEAF, C.byref(nnz), C.byref(lv), C.byref(mf))
    return rc, [np.array([nnz.value, lv.value, mf.value], np.float64)], None


def _handle(name, last):
    def call(case):
        h = C.c_void_p()
        rc = getattr(dpgo_amd.lib(), name)(*_csr(case), None, LEAF, COLLAPSE, BLOCK, last, C.byref(h))
        if h.value:
            getattr(dpgo_amd.lib(), name + "_free")(h)
        return rc, [], h.value
    return call


def _vsolve(case):
    out, status, piv = np.full(3 * N, UNTOUCHED), np.full(2, -7, np.int32), np.full(4, UNTOUCHED)
    rc = dpgo_amd.lib().dpgo_debug_spd_vsolve(*_csr(case), None, LEAF, COLLAPSE, BLOCK, 1, _dp(np.ones(N)), _dp(out), _ip(status),
                                              _dp(piv))
    return rc, [out, status.astype(np.float64), piv], None


def _msolve(case):
    out, status, piv = np.full((3, N, 2), UNTOUCHED), np.full(2, -7, np.int32), np.full(4, UNTOUCHED)
    rc = dpgo_amd.lib().dpgo_debug_spd_msolve(*_csr(case), None, LEAF, COLLAPSE, BLOCK, 1, 0, _dp(np.ones((N, 2))), 2, 2, _dp(out),
                                              _ip(status), _dp(piv))
    return rc, [out, status.astype(np.float64), piv], None


HOOKS = {"solve": _solve, "stats": _stats, "factor": _handle("dpgo_debug_spd_factor", 0),
         "selinv": _handle("dpgo_debug_spd_selinv", 1), "vsolve": _vsolve, "msolve": _msolve}
# (the six above and dpgo_debug_spd_solver_create are the seven hooks that take a CSR matrix)


@pytest.mark.parametrize("case", sorted(_malformed()))
@pytest.mark.parametrize("hook", sorted(HOOKS))
def test_a_malformed_matrix_is_refused_and_nothing_is_written(hook, case):
    rc, outputs, handle = HOOKS[hook](case)
    assert rc == -1
    assert handle is None
    for a in outputs:
        assert np.all(a == UNTOUCHED)


@pytest.mark.parametrize("hook", sorted(HOOKS))
def test_the_well_formed_matrix_goes_through_on_the_host(hook):
    rc, outputs, handle = HOOKS[hook]("well-formed")
    assert rc == 0
    if hook in ("factor", "selinv"):
        assert handle is not None
    elif hook == "stats":
        assert np.all(outputs[0] > 0)                         # entries of the factor, tree levels, the largest front
    else:                                                     # the first solution solves A x = rhs (a few ulps: kappa < 3)
        A = np.diag(np.full(N, 4.0)) - np.diag(np.ones(N - 1), 1) - np.diag(np.ones(N - 1), -1)
        x = outputs[0].reshape(-1)[:N * (1 if hook == "vsolve" else 2)].reshape(N, -1)
        rhs = UNTOUCHED if hook == "solve" else 1.0           # (dpgo_debug_spd_solve works in place: what X held)
        np.testing.assert_allclose(A @ x, rhs, rtol=1e-14, atol=0)
