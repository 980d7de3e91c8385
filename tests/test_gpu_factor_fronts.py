"""The device factorisation (spd_dev.hip) front by front on every elimination path, against an extended-precision Cholesky
(tests/factor_restatement.py).  Inputs, references, bounds and checks are those of tests/test_factor_fronts_host.py, which
validates them on the host numeric path; here the same hook (dpgo_amd.spd_factor_debug) runs the device numeric phase.

The library reads its settings once per process, so every path is a child process (tests/factor_fronts_child.py) that
factors all inputs and writes what the hook returned to a file; the parent compares.  A child that ends by a signal, by
its timeout or with an error fails the module's remaining tests without another child being started.

  tag            environment                                               what runs at these sizes
  default        --                                                        k_fa_panel_ll (left-looking), k_fa_extend_rows
  right_fused    DPGO_SPD_LEFT_LOOKING=0                                   k_fa_potrf_panel<true>, narrow and wide k_fa_abt<0>
  right_unfused  DPGO_SPD_LEFT_LOOKING=0 DPGO_SPD_FUSE_POTRF_WGS=0         k_fa_potrf_reg + k_fa_potrf_panel<false>
  extend_slots   DPGO_SPD_EXTEND_SLOTS=1                                   k_fa_extend, one launch per child slot

Per path and input: the structure, W^T and the padding (bit for bit); every front's W against the reference within
(w + u_rows) u kappa_2(A) max|W_ref| entrywise; the pivot range against diag(L_ref)^2 within n u kappa_2(A); the same bits
on a second call; the kept context (Rescale::Dynamic, the certificate) against a fresh call, bit for bit, and against a
reference of its own; factor_only against the full factorisation; a non-positive pivot where the reference puts it.
The right-looking paths are another order of the same sums: they are held to the reference, not to `default`;
extend_slots equals default bit for bit.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import factor_restatement as fr  # noqa: E402
import test_factor_fronts_host as th  # noqa: E402  (its helpers, caches and bounds; none of its tests is imported)
from test_factor_fronts_host import fronts_tmp  # noqa: E402,F401  (the session's scratch directory)

pytestmark = pytest.mark.gpu

PATHS = {
    "default": {},
    "right_fused": {"DPGO_SPD_LEFT_LOOKING": "0"},
    "right_unfused": {"DPGO_SPD_LEFT_LOOKING": "0", "DPGO_SPD_FUSE_POTRF_WGS": "0"},
    "extend_slots": {"DPGO_SPD_EXTEND_SLOTS": "1"},
}
INPUTS = th.INPUTS
CASES = ["small_leaf", "wide_column", "root_schur"]


def device_results(tmp_dir, path):
    """The child of one path: every input, then the indefinite ones.  (A few seconds: the interpreter, the library, the HIP
    runtime; the factorisations themselves are milliseconds.  The timeout is for a process that hangs.)"""
    fails = th.fails_file(tmp_dir)   # (needs the host child's structure and the references: made before the GPU is asked)
    r = th.child("gpu_" + path, PATHS[path], tmp_dir, fails=fails, timeout=180)
    assert bool(r[INPUTS[0]]["first"]["on_device"]), "the device numeric phase did not run"
    return r


def same_bits(a, b, keys=("W", "WT", "pivot_min", "pivot_max")):
    return all(np.array_equal(np.asarray(a[k]).view(np.int64), np.asarray(b[k]).view(np.int64)) for k in keys)


@pytest.mark.parametrize("name", INPUTS)
@pytest.mark.parametrize("path", list(PATHS))
def test_structure_and_layout(fronts_tmp, path, name):
    runs = device_results(fronts_tmp, path)[name]
    host = th.host_results(fronts_tmp)[name]["first"]
    n = fr.build_input(name)[0].shape[0]
    for k in ("w", "u", "parent", "height", "ldw", "ldm", "w_off", "wt_off", "piv_idx", "upd_idx"):
        assert np.array_equal(runs["first"][k], host[k]), k   # the analysis does not depend on where the numeric phase runs
    for run in ("first", "again", "kept", "fresh"):
        res = th.as_result(runs[run], runs["first"])
        assert res["on_device"]
        fr.check_structure(res, n)
        fr.check_layout(res)


@pytest.mark.parametrize("name", INPUTS)
@pytest.mark.parametrize("path", list(PATHS))
def test_factor_against_extended_precision(fronts_tmp, path, name):
    runs = device_results(fronts_tmp, path)[name]
    th.check_factor(th.as_result(runs["first"], runs["first"]), th.reference(fronts_tmp, name), "%s %s" % (path, name))


@pytest.mark.parametrize("name", INPUTS)
@pytest.mark.parametrize("path", list(PATHS))
def test_pivot_range(fronts_tmp, path, name):
    runs = device_results(fronts_tmp, path)[name]
    th.check_pivots(th.as_result(runs["first"], runs["first"]), th.reference(fronts_tmp, name), "%s %s" % (path, name))
    th.check_pivots(th.as_result(runs["kept"], runs["first"]), th.reference(fronts_tmp, name, second=True),
                    "%s %s, second values" % (path, name))


def test_extend_slots_has_the_bits_of_default(fronts_tmp):
    a, b = device_results(fronts_tmp, "default"), device_results(fronts_tmp, "extend_slots")
    for name in INPUTS:
        for run in ("first", "kept"):
            assert same_bits(a[name][run], b[name][run]), (name, run)


@pytest.mark.parametrize("path", list(PATHS))
def test_same_bits_twice(fronts_tmp, path):
    r = device_results(fronts_tmp, path)
    for name in INPUTS:
        assert same_bits(r[name]["first"], r[name]["again"]), name


@pytest.mark.parametrize("name", INPUTS)
@pytest.mark.parametrize("path", list(PATHS))
def test_kept_context_refactors_like_a_fresh_call(fronts_tmp, path, name):
    """spd_refactor_device on the context the first factorisation left (outputs_zeroed skips the memset of W / WT, the fail
    word and the pivot slots are re-armed): the bits of a fresh call, and the reference of the second values."""
    runs = device_results(fronts_tmp, path)[name]
    assert int(runs["kept"]["status"]) == 0
    assert same_bits(runs["kept"], runs["fresh"])
    th.check_factor(th.as_result(runs["kept"], runs["first"]), th.reference(fronts_tmp, name, second=True),
                    "%s %s, kept context" % (path, name))


@pytest.mark.parametrize("path", list(PATHS))
def test_factor_only_gives_the_verdict_and_pivots_of_the_full_factorisation(fronts_tmp, path):
    r = device_results(fronts_tmp, path)
    full = r["arrow_wide"]
    for only, whole in (("only", "first"), ("onlykept", "kept")):
        assert "W" not in full[only]
        assert int(full[only]["status"]) == int(full[whole]["status"]) == 0
        assert same_bits(full[only], full[whole], ("pivot_min", "pivot_max"))
    for case in CASES:   # ... and of an indefinite one
        assert int(r[case]["failonly"]["status"]) == int(r[case]["fail"]["status"]) == 1
        assert same_bits(r[case]["failonly"], r[case]["fail"], ("pivot_min", "pivot_max")), case


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("path", list(PATHS))
def test_non_positive_pivot_where_the_reference_puts_it(fronts_tmp, path, case):
    """A verdict, not a fault: 'not positive definite', the named front holds k* or is an ancestor of the one that does,
    nothing is printed, and the SPD input factored next -- by a call of its own and through the very context that met the
    pivot -- has the bits it had before the failure."""
    c = th.failure_cases(fronts_tmp)[case]   # (the reference has decided k* before the device is asked)
    th.check_failure(device_results(fronts_tmp, path), case, c, "%s %s" % (path, case))
