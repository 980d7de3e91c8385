"""The pieces of the candidate sets on the device, on GIVEN arrays and without a graph (dpgo_amd/csrc/cand.h):
dpgo_debug_cand_innov -- k_cand_innov and k_cand_resid -- bit for bit against its host twin and against the long-double
restatement (tests/cand_restatement.py), and dpgo_debug_cand_select -- k_cand_score / k_cand_update -- against the long-double
greedy.

Bounds; nothing in them comes from the device.
  cov, S        cand_restatement.margin_cov with bS = 0 (the given Sigma_KK is exact; J's error and the sums remain) and bound_S
  selection     cand_restatement.step_bounds per step; every decision of every input meets check_decisions on the CPU first
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cand_restatement as cd  # noqa: E402
import cov_restatement as cr  # noqa: E402
import marg_restatement as mr  # noqa: E402
import test_cand_host as tch  # noqa: E402  (its comparisons; none of its tests is imported)
import test_pairs_host as tph  # noqa: E402

import dpgo_amd  # noqa: E402

pytestmark = pytest.mark.gpu

LD, U = cd.LD, cd.U


def seeded_pairs(m, nK, anchor_pos, rng):
    """m pairs over nK listed poses: two that share p, one with p_i = q_j, a repeated pair, a reversed pair and an end at the
    anchor first (as many as m allows), then seeded ones; every listed pose appears, in order of first appearance."""
    special = [(0, 1), (0, 2), (3, 0), (0, 1), (1, 0), (anchor_pos, 2)]
    out = special[:m] if m >= 3 else [(0, 1), (1, 0)][:m]
    while len(out) < m:
        p, q = (int(v) for v in rng.integers(0, nK, 2))
        if p != q:
            out.append((p, q))
    K, kpos = cd.pose_list(out)
    return [(K.index(p), K.index(q)) for p, q in out], len(K)   # (renumbered: the list IS 0 ... |K| - 1)


def seeded_sigma(dof, nK, anchor_pos, rng):
    B = rng.standard_normal((dof * nK, dof * nK))
    S = B @ B.T / (dof * nK)
    S = np.tril(S) + np.tril(S, -1).T
    return mr.zero_anchor(S, dof, list(range(nK)), anchor_pos)


# m = 65: 2145 blocks of 4225 lanes, more than one workgroup and an odd tail
@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("m", [1, 2, 3, 12, 65])
def test_innovation_kernel_against_the_restatement_and_its_host_twin(d, m):
    dof = cr.dof_of(d)
    rng = np.random.default_rng(5000 + 100 * d + m)
    pairs, nK = seeded_pairs(m, max(m // 2 + 3, 4), 2, rng)
    anchor = 2 if nK > 2 else -1
    rec = cd.seeded_records(d, nK, rng)
    X = cd.layout_of(rec, d)
    sig = seeded_sigma(dof, nK, anchor, rng)
    cands = [tph.seeded_candidate(X, d, p, q, rng) for p, q in pairs]
    kappa, tau = np.array([c[2] for c in cands]), np.array([c[3] for c in cands])
    packed = dpgo_amd.pack_candidates(d, m, [c[0] for c in cands], [c[1] for c in cands], kappa, tau)
    K = list(range(nK))
    got = dpgo_amd.cand_innov_debug(d, rec, sig, pairs, packed, device=0)
    host = dpgo_amd.cand_innov_debug(d, rec, sig, pairs, packed)
    # explicit fma in one order on both sides, IEEE reciprocals, one add (cand_math.h): the host twin has the same bits
    assert np.array_equal(got["cov"], host["cov"]) and np.array_equal(got["S"], host["S"])
    assert np.array_equal(got["cov"], got["cov"].T) and np.array_equal(got["S"], got["S"].T)
    cov_ld = cd.cov_of(cd.jacobian_cand(X, d, pairs, K, LD), np.asarray(sig, LD))
    S_ld = cd.innovation(cov_ld, d, kappa, tau, LD)
    m_cov = cd.margin_cov(X, d, pairs, K, anchor, sig, 0.0)
    wc = tch.worst(got["cov"], cov_ld, m_cov)
    wS = tch.worst(got["S"], S_ld, cd.bound_S(m_cov, got["S"], d, kappa, tau))
    wr = tch.worst(got["residual"], cd.residuals(X, d, pairs, cands, LD), cd.margin_residuals(X, d, pairs, cands))
    print("d = %d, m = %d, %d poses: cov %.3g, S %.3g, r %.3g of their margins" % (d, m, nK, wc, wS, wr))
    assert max(wc, wS, wr) < 1.0 and np.abs(got["cov"]).max() > 1e6 * m_cov.max()
    assert np.abs(got["residual"] - host["residual"]).max() <= 2 * cd.margin_residuals(X, d, pairs, cands).max()


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("K,bpos,anchor_pos", [(3, 0, 0), (12, 4, 7), (12, 11, None)])
def test_star_sets_are_the_relative_joint_marginal_bit_for_bit(d, K, bpos, anchor_pos):
    dof = cr.dof_of(d)
    rng = np.random.default_rng(7000 + 10 * K + bpos + d)
    rec = cd.seeded_records(d, K, rng)
    sig = seeded_sigma(dof, K, -1 if anchor_pos is None else anchor_pos, rng)
    pairs = [(bpos, k) for k in range(K) if k != bpos]
    # the list of a star set in order of first appearance: the base, then the others -- Sigma_KK and the records in that order
    order = [bpos] + [k for k in range(K) if k != bpos]
    rows = mr.unknowns(dof, order)
    kpos = [(0, i + 1) for i in range(K - 1)]
    X = cd.layout_of(rec, d)
    cands = [tph.seeded_candidate(X, d, p, q, rng) for p, q in pairs]
    packed = dpgo_amd.pack_candidates(d, K - 1, [c[0] for c in cands], [c[1] for c in cands], [c[2] for c in cands], [c[3] for c in cands])
    got = dpgo_amd.cand_innov_debug(d, rec[order], sig[np.ix_(rows, rows)], kpos, packed, device=0)
    assert np.array_equal(got["cov"], dpgo_amd.marg_rel_debug(d, rec, sig, bpos, device=0))


_sel = {}


def selection_input(d, m):
    if (d, m) not in _sel:
        S, r, kappa, tau = cd.synthetic_selection(d, m, 300 + 10 * d + m)
        _sel[(d, m)] = (S, r, kappa, tau, tch.select_reference(d, S, r, kappa, tau, m + 3))
    return _sel[(d, m)]


# n = dof m: 3 ... 420, either side of 64 and of 256 for both d
@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("m", [1, 2, 12, 70])
def test_selection_kernels_against_the_long_double_greedy(d, m):
    S, r, kappa, tau, ref = selection_input(d, m)
    w = np.stack([kappa, tau], 1)
    for budget in (0, 1, m, m + 3):
        out = dpgo_amd.cand_select_debug(d, S, r, w, budget, device=0)
        tch.select_compare(out, ref, budget)
        assert out["n_selected"] == min(budget, m)
    again = dpgo_amd.cand_select_debug(d, S, r, w, m + 3, device=0)
    assert np.array_equal(again["steps"], out["steps"]) and np.array_equal(again["selected"], out["selected"])
    assert again["gain_selected"] == out["gain_selected"] and again["d2_selected"] == out["d2_selected"]
    # the host twin walks the same steps with the same functions: the same order, and the same bits of d2 (no logarithm in it)
    host = dpgo_amd.cand_select_debug(d, S, r, w, m + 3)
    assert np.array_equal(host["selected"], out["selected"]) and np.array_equal(host["steps"][:, 2], out["steps"][:, 2])


def test_entries_past_n_selected_are_untouched():
    d, m = 3, 12
    S, r, kappa, tau, ref = selection_input(d, m)
    mark_sel, mark_steps = np.full(m + 3, -7, np.int32), np.full((m + 3, 4), 123.5)
    out = dpgo_amd.cand_select_debug(d, S, r, np.stack([kappa, tau], 1), m + 3, device=0, selected=mark_sel, steps=mark_steps)
    assert out["n_selected"] == m and out["selected"][:m].tolist() == ref[0]
    assert (out["selected"][m:] == -7).all() and (out["steps"][m:] == 123.5).all()
    # a gate that excludes everything: nothing is written at all
    out = dpgo_amd.cand_select_debug(d, S, r, np.stack([kappa, tau], 1), m, 1e-12, device=0, selected=mark_sel, steps=mark_steps)
    assert out["n_selected"] == 0 and (out["selected"] == -7).all() and (out["steps"] == 123.5).all()
    assert out["gain_selected"] == 0.0 and out["d2_selected"] == 0.0


def test_gate_acts_on_the_conditional_d2():
    """A gate found on the CPU under which gating the unconditioned d2 would select differently: a candidate eligible at the first
    step is excluded only from some later step on, or becomes eligible only there."""
    d, m = 3, 10
    S, r, kappa, tau = cd.synthetic_selection(d, m, 91)
    r = 3.0 * r
    for mutant in ("gate_unconditioned", "rho_not_updated"):
        g = cd.find_gate(S, r, d, kappa, tau, m, lambda g, sel: len(sel) >= 2 and cd.greedy(S, r, d, kappa, tau, m, g, mutant=mutant)[0] != sel)
        assert g is not None
        out, sel = tch.select_eval(d, S, r, kappa, tau, m, g, device=0)
        assert 0 < out["n_selected"] < m
        _, _, trace = cd.greedy(S, r, d, kappa, tau, m, g)
        el = np.array([t["eligible"] | t["taken"] for t in trace])
        assert (el[0] != el[-1]).any()   # some candidate's eligibility changes between the first and the last step


def test_duplicate_tie_and_indefinite_block():
    S, r, kappa, tau = cd.synthetic_selection(3, 8, 77, dup=(2, 5))
    out, sel = tch.select_eval(3, S, r, kappa, tau, 8, tie=(2, 5), device=0)
    assert sel.index(2) < sel.index(5) and out["n_selected"] == 8
    S, r, kappa, tau = cd.synthetic_selection(2, 7, 78, bad=3)
    out, sel = tch.select_eval(2, S, r, kappa, tau, 7, device=0)
    assert 3 not in out["selected"].tolist() and out["n_selected"] == 6
