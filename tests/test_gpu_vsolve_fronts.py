"""The device solve for one plain vector (spd_vsolve_device: k_vs_forward, k_vs_backward) on the inputs of
tests/factor_restatement.py (n <= 718): fronts w = 1, 5, 31, 32, 33, 64, 127, 128, 129, 160, 161, 257, 290, 300 and
u = 0 ... 300 -- a row tile of 32 partly filled and several per front, rows of one entry, fronts with and without update
rows, pull lists from one child and from several -- three tree levels, four trees side by side, unknowns in groups of four.

The kernels stage a front's input vector in LDS 2048 entries at a time, more than any of these fronts has.  So that the
chunk loop -- partial sums carried from chunk to chunk, the re-staging barriers, the row offset of a later chunk, the split
between pivots and update rows falling inside a later chunk of the backward sweep -- runs on them, every input is solved again
with the chunk set to 64 (through dpgo_debug_spd_vsolve_chunk: edges at w = 64, 127 / 128 / 129, 257 = 4 x 64 + 1, up to five
chunks forward and nine backward; a lane's terms and their order are those of one chunk, so the BITS of the default are
demanded) and to 48 (no multiple of the wave: lanes idle, another summation order, tails of 1 ... 47; held to the bound).

The reference is the long-double Cholesky solve and the bound tests/solve_restatement.py's BOUND_C kappa_1 u |x_ref|_1, both
imported through tests/test_polish_host.py, where the host twin is held to the same.  The device defines nothing of its own:
its figure per input is printed and held below 1.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import factor_restatement as fr  # noqa: E402
import solve_restatement as sr  # noqa: E402
import test_polish_host as tph  # noqa: E402  (its inputs, right-hand sides and references; none of its tests is imported)

import dpgo_amd  # noqa: E402

pytestmark = pytest.mark.gpu

INPUTS = tph.INPUTS


@pytest.fixture(scope="module")
def results():
    """Per input: the references first (CPU), then one handle with the second values behind it and a fresh one on them."""
    out = {}
    for name in INPUTS:
        tph.reference(name)
        tph.reference(name, second=True)
    for name in INPUTS:
        out[name] = dict(kept=tph.vsolve(name, host=False, refactor=True), fresh2=tph.vsolve(name, host=False, second=True))
        assert out[name]["kept"]["on_device"] and out[name]["fresh2"]["on_device"], "the device path did not run"
    return out


def test_inputs_cover_the_tile_edges():
    w, u, depth = [], [], []
    for name in INPUTS:
        spec = fr.INPUTS[name]
        t = dpgo_amd.spd_selinv_debug(fr.build_input(name)[1], spec["leaf"], spec["collapse"], spec["block"], host=True)
        w.append(t["w"]); u.append(t["u"]); depth.append(t["depth"].max())
    w, u = np.concatenate(w), np.concatenate(u)
    for v in (1, 5, 31, 32, 33, 64, 127, 128, 129, 160, 161, 257, 290, 300):
        assert v in w, v
    for v in (0, 1, 63, 65, 300):
        assert v in u, v
    assert max(depth) == 2
    # with the chunk at 64 (test_chunk_edges): pivots over more than four chunks, fronts over more than eight
    assert w.max() > 4 * 64 and (w + u).max() > 8 * 64


@pytest.mark.parametrize("name", INPUTS)
def test_device_against_the_long_double_solve(results, name):
    res = results[name]["kept"]
    assert res["status"] == 0
    assert not np.isnan(res["out"]).any()   # (the output was filled with a NaN sentinel: every unknown is some front's pivot)
    r = tph.ratio(res["out"], name)
    print("%s: device %.3g of the bound" % (name, r))
    assert r < 1.0, (name, r)


@pytest.mark.parametrize("name", INPUTS)
def test_chunk_edges(results, name):
    """The chunk loop of both sweeps on fronts of a few hundred rows: chunk 64 gives the default's bits, chunk 48 stays within
    the bound; the kept context behind a refactorisation likewise."""
    res = results[name]["kept"]
    c64 = tph.vsolve(name, host=False, refactor=True, chunk=64)
    assert c64["on_device"] and c64["status"] == 0 and c64["status2"] == 0
    assert np.array_equal(sr.bits(c64["out"]), sr.bits(res["out"])) and np.array_equal(sr.bits(c64["out2"]), sr.bits(res["out2"]))
    assert np.array_equal(sr.bits(c64["out_again"]), sr.bits(res["out"]))
    c48 = tph.vsolve(name, host=False, refactor=True, chunk=48)
    assert c48["status"] == 0 and not np.isnan(c48["raw"]).any()
    r, r2 = tph.ratio(c48["out"], name), tph.ratio(c48["out2"], name, second=True)
    print("%s: chunk 48: device %.3g and %.3g of the bound" % (name, r, r2))
    assert r < 1.0 and r2 < 1.0
    assert np.array_equal(sr.bits(c48["out"]), sr.bits(c48["out_again"]))
    # the default is back
    again = tph.vsolve(name, host=False)
    assert np.array_equal(sr.bits(again["out"]), sr.bits(res["out"]))
    assert dpgo_amd.lib().dpgo_debug_spd_vsolve_chunk(0) == 2048


@pytest.mark.parametrize("name", INPUTS)
def test_same_bits_twice(results, name):
    res = results[name]["kept"]
    assert np.array_equal(sr.bits(res["out"]), sr.bits(res["out_again"]))


@pytest.mark.parametrize("name", INPUTS)
def test_kept_context_solves_like_a_fresh_handle(results, name):
    kept, fresh = results[name]["kept"], results[name]["fresh2"]
    assert kept["status2"] == 0 and fresh["status"] == 0
    assert np.array_equal(sr.bits(kept["out2"]), sr.bits(fresh["out"]))
    assert not np.array_equal(sr.bits(kept["out2"]), sr.bits(kept["out"]))
    assert tph.ratio(kept["out2"], name, second=True) < 1.0


def test_a_non_positive_pivot_is_not_solved_with(results):
    """The planted pivot of tests/test_covariance_host.py: the verdict, nothing written; the second values through the context
    that met it solve to the bits of a fresh handle."""
    name = "arrow_wide"
    spec = fr.INPUTS[name]
    res = dpgo_amd.spd_vsolve_debug(tph.planted_pivot(name), tph.rhs_of(name), spec["leaf"], spec["collapse"], spec["block"],
                                    refactor_values=fr.build_input(name, second=True)[1].data)
    n = len(tph.rhs_of(name))
    assert res["on_device"] and res["status"] == 1 and res["out"] is None and tph.untouched(res["raw"][:2 * n])
    assert res["status2"] == 0
    assert np.array_equal(sr.bits(res["out2"]), sr.bits(results[name]["fresh2"]["out"]))
