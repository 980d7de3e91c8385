"""Host side of the solve for a block of plain vectors (dpgo_amd/csrc/spd.h: spd_msolve_*): the hook dpgo_debug_spd_msolve
on the host (spd_solve_host(F, X, k) through dpgo_amd.spd_msolve_debug(host=True)) against the long-double solve, column by
column within tests/solve_restatement.py's bound, on the six inputs of tests/factor_restatement.py; the hook's argument
checks; the C ABI.  No GPU.

The right-hand sides and references defined here are shared with tests/test_gpu_msolve_fronts.py: per input one block of
KMAX = 65 seeded standard-normal columns and one of 65 unit columns at seeded distinct unknowns; a call with k columns takes
the first k of a block, so one long-double solve per block serves every k.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import factor_restatement as fr  # noqa: E402
import solve_restatement as sr  # noqa: E402
import test_polish_host as tph  # noqa: E402  (its planted pivot and sentinel check; none of its tests is imported)

import dpgo_amd  # noqa: E402

INPUTS = tph.INPUTS
KS = (1, 15, 16, 17, 33, 64, 65)   # the edges of a column tile (16) and of a batch (64)
KMAX = 65
KINDS = ("dense", "unit")
_rhs, _refs = {}, {}


def rhs_block(name, kind):
    """n x KMAX: seeded standard-normal columns, or unit columns at seeded distinct unknowns."""
    key = (name, kind)
    if key not in _rhs:
        n = fr.build_input(name)[0].shape[0]
        rng = np.random.default_rng(4201 + 37 * INPUTS.index(name) + (5 if kind == "unit" else 0))
        if kind == "dense":
            B = rng.standard_normal((n, KMAX))
        else:
            B = np.zeros((n, KMAX))
            B[rng.choice(n, KMAX, replace=False), np.arange(KMAX)] = 1.0
        B.setflags(write=False)
        _rhs[key] = B
    return _rhs[key]


def reference(name, kind, second=False):
    """(X_ref n x KMAX in long double, per column the bound BOUND_C kappa_1 u |x_ref|_1) for the input's first or second
    values and rhs_block(name, kind): once."""
    key = (name, kind, second)
    if key not in _refs:
        ref = sr.ComponentReference(fr.build_input(name, second=second)[0])
        Xref = ref.solve(rhs_block(name, kind), route="cholesky")
        Xref.setflags(write=False)
        _refs[key] = (Xref, ref.bound(Xref))
    return _refs[key]


def ratios(X, name, kind, second=False, cols=None):
    """Per column of X (the block's columns `cols`, default the first X.shape[1]): |x - x_ref|_1 / bound."""
    Xref, bnd = reference(name, kind, second)
    cols = np.arange(X.shape[1]) if cols is None else np.asarray(cols)
    err = np.asarray(np.abs(np.asarray(X, sr.LD) - Xref[:, cols]).sum(axis=0), np.float64)
    return err / bnd[cols]


def msolve(name, k, kind="dense", host=False, second=False, refactor=False, csr=None, chunk=None, ldx=None, cols=None):
    """spd_msolve_debug on a named input with the block's first k columns (or its columns `cols`); refactor: the second
    values through the kept context, with the same right-hand sides."""
    spec = fr.INPUTS[name]
    if csr is None:
        csr = fr.build_input(name, second=second)[1]
    values2 = fr.build_input(name, second=True)[1].data if refactor else None
    B = rhs_block(name, kind)
    B = B[:, :k] if cols is None else B[:, np.asarray(cols)]
    return dpgo_amd.spd_msolve_debug(csr, B, spec["leaf"], spec["collapse"], spec["block"], host=host, refactor_values=values2,
                                     chunk=chunk, ldx=ldx)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", INPUTS)
def test_host_solve_with_k_columns_against_the_long_double_solve(name, kind):
    res = msolve(name, KMAX, kind, host=True)
    assert res["status"] == 0 and not res["on_device"]
    r = ratios(res["out"], name, kind)
    print("%s %s: host, worst column %.3g of the bound" % (name, kind, r.max()))
    assert r.max() < 1.0, (name, kind, r)
    assert np.array_equal(sr.bits(res["out"]), sr.bits(res["out_again"]))
    assert tph.untouched(res["raw"][2])   # (no second values: the third part is not written)


@pytest.mark.parametrize("name", ["arrow_edges", "nested"])
def test_host_row_length_and_fewer_columns(name):
    """ldx > k: the host path writes the first k columns alone; k = 17 of the block solves to the bound as well."""
    res = msolve(name, 17, host=True, ldx=23)
    assert res["status"] == 0 and res["raw"].shape[1:] == (fr.build_input(name)[0].shape[0], 23)
    assert ratios(res["out"], name, "dense").max() < 1.0
    assert tph.untouched(res["raw"][:2, :, 17:]) and not np.isnan(res["raw"][:2, :, :17]).any()


def test_host_refactorisation_and_planted_pivot():
    name = "nested"
    kept = msolve(name, 17, host=True, refactor=True)
    fresh = msolve(name, 17, host=True, second=True)
    assert kept["status2"] == 0 and fresh["status"] == 0
    assert np.array_equal(sr.bits(kept["out2"]), sr.bits(fresh["out"]))
    assert not np.array_equal(sr.bits(kept["out2"]), sr.bits(kept["out"]))
    assert ratios(kept["out2"], name, "dense", second=True).max() < 1.0
    res = msolve("arrow_wide", 17, host=True, csr=tph.planted_pivot())
    assert res["status"] == 1 and res["out"] is None and tph.untouched(res["raw"])


def test_msolve_bad_arguments_return_minus_one():
    L = dpgo_amd.lib()
    _, csr = fr.build_input("arrow_edges")
    n = csr.shape[0]
    ptr, col, val = csr.indptr.astype(np.int32), csr.indices.astype(np.int32), csr.data.astype(np.float64)
    b, out, status, piv = np.ones((n, 3)), np.zeros(3 * n * 4), np.zeros(2, np.int32), np.zeros(4)
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))

    def call(n_=n, ptr_=ptr, col_=col, val_=val, leaf=64, collapse=1, block=1, rhs_=b, k=3, ldx=4, out_=out, status_=status,
             piv_=piv):
        return L.dpgo_debug_spd_msolve(n_, ip(ptr_), ip(col_), dp(val_), None, leaf, collapse, block, 1, 0, dp(rhs_), k, ldx,
                                       dp(out_), ip(status_), dp(piv_))

    assert call() == 0
    assert call(ptr_=None) == -1 and call(col_=None) == -1 and call(val_=None) == -1
    assert call(rhs_=None) == -1 and call(out_=None) == -1 and call(status_=None) == -1 and call(piv_=None) == -1
    assert call(n_=0) == -1 and call(n_=-3) == -1
    assert call(leaf=0) == -1 and call(block=0) == -1 and call(collapse=-1) == -1
    assert call(block=7) == -1                       # n is no multiple of the block
    assert call(k=0) == -1 and call(k=-1) == -1 and call(k=3, ldx=2) == -1
    bad = col.copy()
    bad[5] = n
    assert call(col_=bad) == -1
    bad = ptr.copy()
    bad[3] = bad[2] - 1
    assert call(ptr_=bad) == -1
    with pytest.raises(ValueError):
        dpgo_amd.spd_msolve_debug(csr, np.ones(n), 64)           # one vector is spd_vsolve_debug's
    with pytest.raises(ValueError):
        dpgo_amd.spd_msolve_debug(csr, np.ones((n, 3)), 64, ldx=2)


def test_msolve_abi():
    L = dpgo_amd.lib()
    header = open(os.path.join(os.path.dirname(dpgo_amd.__file__), "..", "include", "dpgo_amd.h")).read()
    assert "dpgo_debug_spd_msolve(" in header and "dpgo_debug_spd_msolve" in dpgo_amd.SYMBOLS and hasattr(L, "dpgo_debug_spd_msolve")
