"""Selected inversion on the device (spd_selinv_device: k_si_gather, k_si_abt<0>, k_si_abt<1>) front by front, against the dense
long-double inverse, on the inputs of tests/factor_restatement.py (n <= 718): w = 1, 5, 31, 32, 33, 64, 127, 128, 129, 160,
161, 257, 290, 300 and u = 0, 1, 63, 65, 161, 300 with u > w -- one tile and many, full tiles and partly filled ones, fronts
of one column, three tree levels, four trees side by side, unknowns in groups of four.

The bound, the references and the restatements are those of tests/test_covariance_host.py; the bound's constant was fixed
there, on the CPU.  The device defines nothing of its own: its figure per input is printed and held below 1.
S_front is symmetric BIT FOR BIT: S_pp is computed on and below the diagonal and mirrored, T and T^T are one product stored
twice, S_uu is a copy of a symmetric block.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_restatement as cr  # noqa: E402
import factor_restatement as fr  # noqa: E402

import dpgo_amd  # noqa: E402

pytestmark = pytest.mark.gpu

INPUTS = ["arrow_wide", "arrow_tall", "arrow_edges", "arrow_edges_lap", "nested", "arrow_block4"]


def run(name, second=False, refactor=False, csr=None):
    spec = fr.INPUTS[name]
    if csr is None:
        csr = fr.build_input(name, second=second)[1]
    values2 = fr.build_input(name, second=True)[1].data if refactor else None
    return dpgo_amd.spd_selinv_debug(csr, spec["leaf"], spec["collapse"], spec["block"], refactor_values=values2)


@pytest.fixture(scope="module")
def results():
    """Per input: the references first (CPU), then one handle with the second values behind it and a fresh one on them."""
    out = {}
    for name in INPUTS:
        spec = fr.INPUTS[name]
        host = dpgo_amd.spd_selinv_debug(fr.build_input(name)[1], spec["leaf"], spec["collapse"], spec["block"], host=True)
        cr.reference(name, host)
    for name in INPUTS:
        out[name] = dict(kept=run(name, refactor=True), fresh2=run(name, second=True))
        assert out[name]["kept"]["on_device"], "the device path did not run"
    return out


def test_inputs_cover_the_tile_edges(results):
    w = np.concatenate([results[n]["kept"]["w"] for n in INPUTS])
    u = np.concatenate([results[n]["kept"]["u"] for n in INPUTS])
    for v in (1, 31, 32, 33, 64, 127, 128, 129, 160, 161, 257, 290, 300):
        assert v in w, v
    for v in (0, 1, 63, 65):
        assert v in u, v
    assert (u > w).any() and results["nested"]["kept"]["depth"].max() == 2


@pytest.mark.parametrize("name", INPUTS)
def test_device_against_the_long_double_inverse(results, name):
    res = results[name]["kept"]
    assert res["status"] == 0 and res["selinv_status"] == 0
    ref, Sref, bnd = cr.reference(name, res)
    ratio = cr.worst_ratio(res, res["sigma"], Sref, bnd)
    print("%s: device %.3g of the bound" % (name, ratio))
    assert ratio < 1.0, (name, ratio)


@pytest.mark.parametrize("name", INPUTS)
def test_symmetric_bit_for_bit(results, name):
    assert cr.symmetric_bits(results[name]["kept"]["sigma"])
    assert cr.symmetric_bits(results[name]["kept"]["sigma2"])


@pytest.mark.parametrize("name", INPUTS)
def test_same_bits_twice(results, name):
    assert cr.same_bits(results[name]["kept"]["sigma"], results[name]["kept"]["sigma_again"])


@pytest.mark.parametrize("name", INPUTS)
def test_kept_context_inverts_like_a_fresh_handle(results, name):
    kept, fresh = results[name]["kept"], results[name]["fresh2"]
    assert kept["status2"] == 0 and kept["selinv_status2"] == 0 and fresh["selinv_status"] == 0
    assert cr.same_bits(kept["sigma2"], fresh["sigma"])
    assert not cr.same_bits(kept["sigma2"], kept["sigma"])


@pytest.mark.parametrize("name", INPUTS)
def test_a_factorisation_behind_an_inversion_keeps_its_bits(results, name):
    res = results[name]["kept"]
    assert res["W_before"] is not None and np.abs(res["W_before"]).max() > 0
    assert np.array_equal(res["W_before"].view(np.int64), res["W_after"].view(np.int64))


def test_a_non_positive_pivot_is_not_inverted(results):
    """The first pivot of the 5-wide leaf of arrow_wide is its own diagonal entry: -1 there is a non-positive pivot whatever
    the arithmetic.  The verdict, no inversion; the second values through the context that met it invert to the bits of a
    fresh handle."""
    name = "arrow_wide"
    good = results[name]["kept"]
    s = int(np.flatnonzero(good["w"] == 5)[0])
    v = int(good["piv_idx"][s][0])
    B = fr.build_input(name)[0].copy()
    B[v, v] = -1.0
    spec = fr.INPUTS[name]
    res = dpgo_amd.spd_selinv_debug(fr.to_csr(B, spec["pattern"]()), spec["leaf"], spec["collapse"], spec["block"],
                                    refactor_values=fr.build_input(name, second=True)[1].data)
    assert res["on_device"] and res["status"] == 1 and res["selinv_status"] == 1
    assert res["sigma"] is None and res["sigma_again"] is None
    assert res["status2"] == 0 and res["selinv_status2"] == 0
    assert cr.same_bits(res["sigma2"], results[name]["fresh2"]["sigma"])
