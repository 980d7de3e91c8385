"""The device solve for a block of plain vectors (spd_msolve_device: k_ms_forward, k_ms_backward) on the inputs of
tests/factor_restatement.py (n <= 718): fronts w = 1 ... 300 and u = 0 ... 300 -- a row item of 64 partly filled and several
per front, fronts of one row, fronts with and without update rows, pull lists from one child and from several -- three tree
levels, four trees side by side, unknowns in groups of four.

Columns.  k = 1, 15, 16, 17, 33, 64, 65: a column tile of 16 partly filled, full, and one column into the next; the batch of
64 full, and one column into a second batch.  Right-hand sides: seeded standard-normal columns and unit columns (what the
joint covariances solve with), the first k of one block of 65 per input (tests/test_msolve_host.py), so that the call with
65 columns, the calls with fewer and the calls with one column alone solve the same vectors and their BITS can be compared:
a column's bits must not depend on its companions, its position in a tile or the batch it falls into.

Slabs.  The kernels stage a front's input block 32 rows at a time, so the slab loop runs on every front deeper than that; with
the slab set to 4 (the MFMA depth: 73 slabs in the 290-wide front) and to 28 (a multiple of it that does not divide 32) every
instruction still sums the same four terms, and the bits of the default are demanded; 7 pads every slab with a zero row and
regroups the terms: held to the bound.

The reference is the long-double Cholesky solve and the bound tests/solve_restatement.py's BOUND_C kappa_1 u |x_ref|_1 per
column, both through tests/test_msolve_host.py, where the host twin is held to the same.  The device defines nothing of its
own: its worst column per input is printed and held below 1.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import factor_restatement as fr  # noqa: E402
import solve_restatement as sr  # noqa: E402
import test_msolve_host as tmh  # noqa: E402  (its right-hand sides and references; none of its tests is imported)
import test_polish_host as tph  # noqa: E402  (its planted pivot; none of its tests is imported)

import dpgo_amd  # noqa: E402

pytestmark = pytest.mark.gpu

INPUTS, KS, KMAX, KINDS = tmh.INPUTS, tmh.KS, tmh.KMAX, tmh.KINDS


@pytest.fixture(scope="module")
def full():
    """Per (input, kind): the references first (CPU), then the call with all 65 columns, the second values behind it."""
    out = {}
    for name in INPUTS:
        for kind in KINDS:
            tmh.reference(name, kind)
        tmh.reference(name, "dense", second=True)
    for name in INPUTS:
        for kind in KINDS:
            out[name, kind] = tmh.msolve(name, KMAX, kind, refactor=True)
            assert out[name, kind]["on_device"], "the device path did not run"
    return out


def test_inputs_cover_the_item_and_slab_edges():
    w, u = [], []
    for name in INPUTS:
        spec = fr.INPUTS[name]
        t = dpgo_amd.spd_selinv_debug(fr.build_input(name)[1], spec["leaf"], spec["collapse"], spec["block"], host=True)
        w.append(t["w"]); u.append(t["u"])
    w, u = np.concatenate(w), np.concatenate(u)
    for v in (1, 5, 31, 32, 33, 64, 127, 128, 129, 160, 161, 257, 290, 300):
        assert v in w, v
    for v in (0, 1, 63, 65, 300):
        assert v in u, v
    # more than one row item per front in both sweeps, more than one slab of 32, slabs of every residue modulo 4
    assert w.max() > 4 * 64 and (w + u).max() > 8 * 64
    assert {int(v) % 4 for v in w} == {0, 1, 2, 3} and {int(v) % 4 for v in w + u} == {0, 1, 2, 3}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", INPUTS)
def test_every_k_against_the_long_double_solve(full, name, kind):
    worst = 0.0
    for k in KS:
        res = full[name, kind] if k == KMAX else tmh.msolve(name, k, kind)
        assert res["on_device"] and res["status"] == 0
        assert not np.isnan(res["raw"][:2]).any()   # (the arrays were filled with a NaN sentinel: every unknown is some front's pivot)
        r = tmh.ratios(res["out"], name, kind)
        assert r.shape == (k,) and r.max() < 1.0, (name, kind, k, r)
        worst = max(worst, float(r.max()))
        # the same bits twice, and the bits of the same columns among 65
        assert np.array_equal(sr.bits(res["out"]), sr.bits(res["out_again"]))
        assert np.array_equal(sr.bits(res["out"]), sr.bits(full[name, kind]["out"][:, :k])), (name, kind, k)
    print("%s %s: device, worst column over k = %s: %.3g of the bound" % (name, kind, list(KS), worst))


@pytest.mark.parametrize("name", INPUTS)
def test_a_column_alone_and_in_reverse_order_has_the_bits_of_the_65_column_call(full, name):
    want = sr.bits(full[name, "dense"]["out"])
    rev = tmh.msolve(name, KMAX, cols=np.arange(KMAX)[::-1])
    assert rev["status"] == 0 and np.array_equal(sr.bits(rev["out"][:, ::-1]), want)
    for c in range(KMAX):
        one = tmh.msolve(name, 1, cols=[c])
        assert one["status"] == 0 and np.array_equal(sr.bits(one["out"][:, 0]), want[:, c]), (name, c)
    for kind, cols in (("unit", [0, 15, 16, 63, 64]),):
        wantu = sr.bits(full[name, kind]["out"])
        for c in cols:
            one = tmh.msolve(name, 1, kind, cols=[c])
            assert np.array_equal(sr.bits(one["out"][:, 0]), wantu[:, c]), (name, kind, c)


@pytest.mark.parametrize("name", INPUTS)
def test_slab_edges(full, name):
    """Slabs of 4 and 28 rows give the default's bits, on the second values through the kept context too; 7 stays within the
    bound; the default is back afterwards."""
    res = full[name, "dense"]
    for chunk in (4, 28):
        c = tmh.msolve(name, KMAX, refactor=True, chunk=chunk)
        assert c["on_device"] and c["status"] == 0 and c["status2"] == 0
        assert np.array_equal(sr.bits(c["out"]), sr.bits(res["out"])) and np.array_equal(sr.bits(c["out2"]), sr.bits(res["out2"]))
        assert np.array_equal(sr.bits(c["out_again"]), sr.bits(res["out"]))
    c7 = tmh.msolve(name, KMAX, refactor=True, chunk=7)
    assert c7["status"] == 0 and not np.isnan(c7["raw"]).any()
    r, r2 = tmh.ratios(c7["out"], name, "dense").max(), tmh.ratios(c7["out2"], name, "dense", second=True).max()
    print("%s: slab 7: device %.3g and %.3g of the bound" % (name, r, r2))
    assert r < 1.0 and r2 < 1.0
    assert np.array_equal(sr.bits(c7["out"]), sr.bits(c7["out_again"]))
    again = tmh.msolve(name, 17)
    assert np.array_equal(sr.bits(again["out"]), sr.bits(res["out"][:, :17]))


@pytest.mark.parametrize("k,ldx", [(17, 23), (65, 70), (1, 2)])
@pytest.mark.parametrize("name", INPUTS)
def test_row_length_beyond_k_keeps_the_padding(full, name, k, ldx):
    res = tmh.msolve(name, k, ldx=ldx)
    assert res["status"] == 0 and res["raw"].shape[2] == ldx
    assert tph.untouched(res["raw"][:2, :, k:]) and not np.isnan(res["raw"][:2, :, :k]).any()
    assert np.array_equal(sr.bits(res["out"]), sr.bits(full[name, "dense"]["out"][:, :k]))


@pytest.mark.parametrize("name", INPUTS)
def test_kept_context_solves_like_a_fresh_handle(full, name):
    kept = full[name, "dense"]
    fresh = tmh.msolve(name, KMAX, second=True)
    assert kept["status2"] == 0 and fresh["status"] == 0
    assert np.array_equal(sr.bits(kept["out2"]), sr.bits(fresh["out"]))
    assert not np.array_equal(sr.bits(kept["out2"]), sr.bits(kept["out"]))
    r = tmh.ratios(kept["out2"], name, "dense", second=True)
    print("%s: second values: device, worst column %.3g of the bound" % (name, r.max()))
    assert r.max() < 1.0


def test_a_non_positive_pivot_is_not_solved_with(full):
    """The planted pivot of tests/test_covariance_host.py: the verdict, -1 from the solve, nothing written; the second values
    through the context that met it solve to the bits of a fresh handle."""
    name = "arrow_wide"
    res = tmh.msolve(name, 33, csr=tph.planted_pivot(name), refactor=True, ldx=35)
    assert res["on_device"] and res["status"] == 1 and res["out"] is None and tph.untouched(res["raw"][:2])
    assert res["status2"] == 0
    assert np.array_equal(sr.bits(res["out2"]), sr.bits(full[name, "dense"]["out2"][:, :33]))
    assert tph.untouched(res["raw"][2, :, 33:])
