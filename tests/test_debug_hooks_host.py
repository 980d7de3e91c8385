"""The CSR reader of the test hooks (capi_debug.cpp: read_csr), through every hook that takes a matrix and runs without a
device: a malformed matrix is refused with -1 before anything is written, a well-formed one goes through with host=1.
dpgo_debug_spd_solver_create is not here: it answers -2 without a device before it reads the matrix.
At the end: the hooks that work on a group (the gate's launch kinds of dpgo_group_debug_cg_scalars, dpgo_group_debug_star_sums,
dpgo_group_debug_gated_update) answer -1 on the host and write nothing."""
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


# ---- the hooks of the speculative update's gate, the master's sums and the gated launches (capi_debug.cpp): they work on a
# group, which only a device can hold; on the host their argument checks answer -1 before anything is touched.  (The checks
# that need a group to compare with -- bits outside it, nslots outside (0, MAX_SLOTS] -- are in tests/test_gpu_gate.py.)
def _gate_script(nslots=15, n=1):
    L = 1
    keep = [np.zeros(L), np.zeros(L, np.int32)]
    g = dpgo_amd.GateDebug()
    g.nslots = nslots
    for k in ("f", "Fk0", "Fk1", "fobj"):
        setattr(g, k, _dp(keep[0]))
    g.hits0 = g.hits1 = _ip(keep[1])
    arr = (dpgo_amd.CgDebugLaunch * n)()
    arr[0].kind = dpgo_amd.CG_DEBUG_KINDS.index("reduce_gate")
    arr[0].gate = C.addressof(g)
    return arr, keep + [g]


@pytest.mark.parametrize("case", ["no group", "no group, no script", "no group, nslots = 0", "no group, nslots = 33"])
def test_the_gate_hook_refuses_on_the_host(case):
    arr, keep = _gate_script({"no group, nslots = 0": 0, "no group, nslots = 33": 33}.get(case, 15))
    out = [np.full(64, UNTOUCHED) for _ in range(5)]
    words = [np.full(8, 7, np.uint64) for _ in range(3)]
    arrived = np.full(2, 7, np.uint32)
    U = C.POINTER(C.c_ulonglong)
    rc = dpgo_amd.lib().dpgo_group_debug_cg_scalars(None, None if "no script" in case else arr, 1, _dp(out[0]), words[0].ctypes.data_as(U),
                                                    _dp(out[1]), _dp(out[2]), _dp(out[3]), words[1].ctypes.data_as(U),
                                                    arrived.ctypes.data_as(C.POINTER(C.c_uint)), _dp(out[4]), words[2].ctypes.data_as(U))
    assert rc == -1
    assert all(np.all(a == UNTOUCHED) for a in out) and all(np.all(w == 7) for w in words) and np.all(arrived == 7)


@pytest.mark.parametrize("valid", [0x3f, 0x40, 0xffffffff])
@pytest.mark.parametrize("null", ["group", "group and partials", "group and out"])
def test_the_star_sums_hook_refuses_on_the_host(null, valid):
    P, out, seq = np.zeros((32, 4)), np.full(8, UNTOUCHED), np.full(2, 7, np.uint64)
    rc = dpgo_amd.lib().dpgo_group_debug_star_sums(None, None if "partials" in null else _dp(P), valid, None if "out" in null else _dp(out),
                                                   seq.ctypes.data_as(C.POINTER(C.c_ulonglong)))
    assert rc == -1 and np.all(out == UNTOUCHED) and np.all(seq == 7)


@pytest.mark.parametrize("word", [0, 1, 0xFFFFFFFFFFFFFFFF])
def test_the_gated_update_hook_refuses_on_the_host(word):
    rep = np.full(36, -7, np.int32)
    assert dpgo_amd.lib().dpgo_group_debug_gated_update(None, word, _ip(rep)) == -1 and np.all(rep == -7)
    assert dpgo_amd.lib().dpgo_group_debug_gated_update(None, word, None) == -1
