"""The inputs, references and the bound of the device solve's tests (tests/solve_restatement.py), validated without a GPU:
tests/test_gpu_solve_tiles.py holds k_spd_level, k_root_sym, k_root_combine and k_pack_panels to them, so a wrong input, a
wrong reference or a bound that ordinary fp64 arithmetic cannot meet is found here first -- through dpgo_amd.spd_solve_host,
whose sweeps are the host's.

  * every new input has the front shapes it was made for (dpgo_amd.spd_factor_debug; the device plan's part of the
    structure -- tile classes, counts per node -- is asserted from the plan read-back in the GPU test);
  * the refinement route of the reference agrees with the long-double Cholesky route to 1e-3 of the bound on every component
    small enough for both;
  * the host sweeps are within the bound of the reference, for d = 2, 3 and dof = 1, d;
  * plain fp64 restatements of the two routes the device takes -- two sweeps; the roots through L11^-T L11^-1 formed in
    fp64 -- stay at least 4x below the bound's constant (the figures are printed, and recorded in DESIGN.md);
  * the checks of the GPU test catch the two slips they were aimed at (a mutation of the restated sweeps).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dpgo_amd  # noqa: E402
import solve_restatement as sr  # noqa: E402

INPUTS = list(sr.INPUTS)
COMBOS = [(3, 1), (3, 3), (2, 1), (2, 2)]
_tables = {}


def table(name):
    """The front table of an input (the analysis does not depend on where the numeric phase runs)."""
    if name not in _tables:
        inp = sr.build_input(name)
        _tables[name] = dpgo_amd.spd_factor_debug(inp.csr, *inp.args)
        assert _tables[name]["status"] == 0
    return _tables[name]


@pytest.mark.parametrize("name", INPUTS)
def test_inputs_have_the_fronts_they_were_made_for(name):
    t = table(name)
    print(name, " ".join("%d/%d@%d" % (w, u, h) for w, u, h in zip(t["w"], t["u"], t["height"]))[:2000])
    sr.check_input_structure(name, t)
    inp = sr.build_input(name)
    for s in range(t["nfronts"]):   # a front never spans two nodes
        assert len(set(inp.nodes[np.asarray(t["piv_idx"][s], np.int64)].tolist())) <= 1


def test_pull_lists_cover_every_residue():
    """pull_updates fetches PULLB = 2 (64-row and narrow tiles) or 4 (16-row tiles) rows per round: list lengths of every
    residue, and lists of several rounds, among the positions of a narrow root and of wide fronts."""
    t = table("narrow_only")
    root = int(np.flatnonzero(np.asarray(t["parent"]) < 0)[0])
    assert set((sr.pull_lengths(t, root) % 4).tolist()) == {0, 1, 2, 3}
    t = table("nested")
    wide = [f for f in range(t["nfronts"]) if t["height"][f] > 0]
    assert {int(v) % 2 for f in wide for v in sr.pull_lengths(t, f)} == {0, 1}


def test_refinement_route_agrees_with_the_cholesky_route():
    """On every component of up to CHOLESKY_MAX unknowns: scipy's LU + three rounds of long-double refinement against the
    long-double Cholesky, within 1e-3 of the bound."""
    worst = 0.0
    for name in INPUTS:
        inp = sr.build_input(name)
        B = sr.rhs(name, 3, 1)[0]
        for idx, ref in zip(inp.comps, inp.reference()):
            if ref.n > sr.CHOLESKY_MAX:
                continue
            Xc, Xr = ref.solve(B[idx], "cholesky"), ref.solve(B[idx], "refined")
            err = np.asarray(np.abs(Xc - Xr).sum(axis=0), np.float64)
            worst = max(worst, float((err / ref.bound(Xc)).max()))
    print("refinement against Cholesky: worst difference / bound %.3g" % worst)
    assert worst <= 1e-3
    assert any(ref.n > sr.CHOLESKY_MAX for name in INPUTS for ref in sr.build_input(name).reference())   # (the route is used)


@pytest.mark.parametrize("name", INPUTS)
def test_host_sweeps_within_the_bound(name):
    inp = sr.build_input(name)
    for d, dof in COMBOS:
        B = sr.rhs(name, d, dof)[0]
        X = dpgo_amd.spd_solve_host(inp.csr, B, leaf=inp.args[0])
        r = sr.solve_ratios(X, name, d, dof)
        print("host %s d %d dof %d: worst error / bound %.3g, kappa_1 up to %.3g" % (name, d, dof, r.max(),
                                                                                     max(c.kappa1 for c in inp.reference())))
        assert r.max() <= 1.0


def _restated(name, d, dof, fused):
    return sr.restated_solve(name, table(name), sr.rhs(name, d, dof)[0], fused=fused)


def test_fp64_restatements_leave_four_times_the_bound():
    """The constant of the bound against ordinary fp64 arithmetic on both routes: worst error / (kappa_1 u |x_ref|_1)."""
    worst = {False: (0.0, ""), True: (0.0, "")}
    for name in INPUTS:
        for fused in (False, True):
            r = float(sr.solve_ratios(_restated(name, 3, 1, fused), name, 3, 1).max()) * sr.BOUND_C
            print("fp64 restatement, %s, %s: error / (kappa_1 u |x|_1) = %.3g" % ("fused roots" if fused else "two sweeps", name, r))
            worst[fused] = max(worst[fused], (r, name))
    print("worst: two sweeps %.3g (%s), fused roots %.3g (%s); constant %g" % (worst[False] + worst[True] + (sr.BOUND_C,)))
    assert 4.0 * max(worst[False][0], worst[True][0]) <= sr.BOUND_C


@pytest.mark.parametrize("mutation", ["backward_scale_undo", "asm_ptr_off_by_one"])
def test_the_checks_catch_the_slips_they_aim_at(mutation):
    """The restated sweeps with the slip built in (solve_restatement.sweeps, mutate=...), judged as the GPU test judges the
    device: scale = -1 must give the negated bits of scale = +1, and the solution must be within the bound."""
    name = "nested"
    B = sr.rhs(name, 3, 1)[0]
    plus, minus = (sr.restated_solve(name, table(name), B, scale=sc) for sc in (1.0, -1.0))
    assert np.array_equal(sr.bits(-minus), sr.bits(plus)) and sr.solve_ratios(plus, name, 3, 1).max() <= 1.0
    bad_plus, bad_minus = (sr.restated_solve(name, table(name), B, scale=sc, mutate=mutation) for sc in (1.0, -1.0))
    caught_by_scale = not np.array_equal(sr.bits(-bad_minus), sr.bits(bad_plus))
    caught_by_bound = sr.solve_ratios(bad_plus, name, 3, 1).max() > 1.0
    print(mutation, "scale check:", caught_by_scale, "bound:", caught_by_bound)
    if mutation == "backward_scale_undo":
        assert caught_by_scale      # (with scale = +1 the slip is invisible: only the scale check sees it)
        assert not caught_by_bound
    else:
        assert caught_by_bound
