"""Host side of the candidate sets (dpgo_amd/csrc/cand.h): the restatement (tests/cand_restatement.py) held to its identities in
long double, the host hooks against it within its bounds, seven mistakes a kernel could make, and the C ABI.  No GPU.

The points are those of tests/test_pairs_host.py and the reference those of tests/test_marg_host.py; bS is the factorisation's part
of the blocks' bound alone (C u kappa_2 |A^-1|_2), as there.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cand_restatement as cd  # noqa: E402
import cov_restatement as cr  # noqa: E402
import factor_restatement as fr  # noqa: E402
import marg_restatement as mr  # noqa: E402
import pairs_restatement as pr  # noqa: E402
import test_marg_host as tmh  # noqa: E402  (its reference; none of its tests is imported)
import test_pairs_host as tph  # noqa: E402

import dpgo_amd  # noqa: E402
from dpgo_amd import CandResult, cand_innov_debug, cand_select_debug  # noqa: E402,F401  (the subject of every test here)

LD, U = cd.LD, cd.U
FIXTURES = ["tinyGrid3D", "smallGrid3D", "ladder2"]


def seeded_set(N, anchor, seed, m):
    """m seeded candidates: random pairs, then two that share p, one with p_i = q_j, a repeated pair, a reversed pair and one
    with an end at the anchor."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < max(m - 6, 1):
        p, q = (int(v) for v in rng.integers(0, N, 2))
        if p != q and anchor not in (p, q):
            out.append((p, q))
    p0, q0 = out[0]
    free = [g for g in range(N) if g not in (anchor, p0, q0)]
    extra = [(p0, free[0]), (p0, free[1]), (free[2], p0), (p0, q0), (q0, p0), (anchor, free[3])]
    return (out + extra)[:m]


def problem(fixtures_dir, name, anchor, m, seed):
    """The restated quantities of a seeded candidate set, long double, and what the fp64 route has for them."""
    d, N, X, A, L, S64, bS = tmh.reference(fixtures_dir, name, anchor)
    dof = cr.dof_of(d)
    pairs = seeded_set(N, anchor, seed, m)
    rng = np.random.default_rng(seed + 1)
    cands = [tph.seeded_candidate(X, d, p, q, rng) for p, q in pairs]
    kappa, tau = np.array([c[2] for c in cands]), np.array([c[3] for c in cands])
    K, kpos = cd.pose_list(pairs)
    sig_ld = mr.sigma_kk(A, dof, K, anchor, L)
    sig_64 = mr.sigma_from_dense(S64, dof, K, anchor)
    cov_ld = cd.cov_of(cd.jacobian_cand(X, d, pairs, K, LD), sig_ld)
    S_ld = cd.innovation(cov_ld, d, kappa, tau, LD)
    r_ld = cd.residuals(X, d, pairs, cands, LD)
    return dict(d=d, dof=dof, N=N, X=X, A=A, L=L, bS=bS, pairs=pairs, cands=cands, kappa=kappa, tau=tau, K=K, kpos=kpos, sig_ld=sig_ld,
                sig_64=sig_64, cov_ld=cov_ld, S_ld=S_ld, r_ld=r_ld, anchor=anchor)


def packed(P):
    d = P["d"]
    return dpgo_amd.pack_candidates(d, len(P["pairs"]), [c[0] for c in P["cands"]], [c[1] for c in P["cands"]], P["kappa"], P["tau"])


def worst(got, want, bound):
    return float(np.max(np.abs(np.asarray(got, LD) - want) / (bound + 1e-300)))


# ---------------------------------------------------------------------------------------------------------------
# the identities of the restatement, in long double
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_full_budget_sums_to_the_joint_test_and_prefixes_to_principal_submatrices(fixtures_dir, name):
    P = problem(fixtures_dir, name, 0, 7, 21)
    d, dof, m = P["d"], P["dof"], 7
    _, logdet, d2j, gain_all, _ = cd.joint(P["S_ld"], P["r_ld"], d, P["kappa"], P["tau"])
    sel, steps, _ = cd.greedy(P["S_ld"], P["r_ld"], d, P["kappa"], P["tau"], m)
    assert sorted(sel) == list(range(m))
    g, q = np.cumsum([s[1] for s in steps]), np.cumsum([s[2] for s in steps])
    assert abs(g[-1] - gain_all) <= 1e-15 * m * max(1, abs(gain_all)) and abs(q[-1] - d2j) <= 1e-14 * max(1, abs(d2j))
    lw = cd.logdet_omega_inv(d, P["kappa"], P["tau"])
    for t in range(m):
        idx = mr.unknowns(dof, sel[:t + 1])
        _, ld_t, d2_t, _, _ = cd.joint(P["S_ld"][np.ix_(idx, idx)], P["r_ld"][idx], d, P["kappa"][sel[:t + 1]], P["tau"][sel[:t + 1]])
        assert abs(g[t] - (ld_t - lw[sel[:t + 1]].sum()) / 2) <= 1e-14 * max(1, abs(g[t])) and abs(q[t] - d2_t) <= 1e-14 * max(1, abs(q[t]))


@pytest.mark.parametrize("name", ["tinyGrid3D", "ladder2"])
def test_determinant_lemma(fixtures_dir, name):
    """gain_all = 1/2 [log det (H + J^T Omega J) - log det H]: the information the candidates would add, as edges, to the anchored H."""
    P = problem(fixtures_dir, name, 0, 6, 5)
    d, dof, N = P["d"], P["dof"], P["N"]
    Jf = np.zeros((dof * 6, dof * N), LD)
    Jk = cd.jacobian_cand(P["X"], d, P["pairs"], P["K"], LD)
    for k, g in enumerate(P["K"]):
        if g != 0:   # (the anchor does not move)
            Jf[:, dof * g:dof * g + dof] = Jk[:, dof * k:dof * k + dof]
    Om = np.diag(1 / cd.omega_inv(d, P["kappa"], P["tau"], LD))
    A = np.asarray(P["A"], LD)
    Lp, kstar, _ = fr.cholesky_ld(A + Jf.T @ Om @ Jf)
    assert kstar < 0
    lhs = (2 * np.log(np.diag(Lp)).sum() - 2 * np.log(np.diag(P["L"])).sum()) / 2
    gain_all = cd.joint(P["S_ld"], P["r_ld"], d, P["kappa"], P["tau"])[3]
    print("%s: gain_all %.15g, by the determinant lemma %.15g" % (name, float(gain_all), float(lhs)))
    assert abs(lhs - gain_all) <= 1e-12 * max(1, abs(gain_all))


@pytest.mark.parametrize("name", FIXTURES)
def test_two_anchors_and_the_diagonal_blocks(fixtures_dir, name):
    """cov and gain_all under anchors 0 and N - 1 agree to first order at a critical point; the difference the restatement shows
    at these points (the solver's iterates, not polished ones) is printed and held to two digits, as tests/test_marg_host.py
    does.  The diagonal blocks of cov are pairs_restatement.rel_cov."""
    N = tmh.reference(fixtures_dir, name, 0)[1]
    out = {}
    for a in (0, N - 1):
        P = problem(fixtures_dir, name, a, 5, 33)   # (the same seeded pairs only where they avoid both anchors)
        out[a] = P
    pairs = [pq for pq in out[0]["pairs"] if N - 1 not in pq and 0 not in pq]
    assert len(pairs) >= 3
    res = {}
    for a in (0, N - 1):
        d, _, X, A, L, _, _ = tmh.reference(fixtures_dir, name, a)
        dof = cr.dof_of(d)
        K, _ = cd.pose_list(pairs)
        sig = mr.sigma_kk(A, dof, K, a, L)
        cov = cd.cov_of(cd.jacobian_cand(X, d, pairs, K, LD), sig)
        rng = np.random.default_rng(2)
        cands = [tph.seeded_candidate(X, d, p, q, rng) for p, q in pairs]
        kap, tau = np.array([c[2] for c in cands]), np.array([c[3] for c in cands])
        S = cd.innovation(cov, d, kap, tau, LD)
        res[a] = (cov, cd.joint(S, cd.residuals(X, d, pairs, cands, LD), d, kap, tau)[3])
        full = np.zeros((A.shape[0], A.shape[0]), LD)
        for i, (p, q) in enumerate(pairs):
            cols = mr.unknowns(dof, [p, q])
            full[:, cols] = mr.columns_ld(A, dof, [p, q], L)
            rel = pr.rel_cov(pr.jacobian(X, d, p, q, LD), pr.joint_of(full, dof, p, q, a))
            assert np.abs(cov[dof * i:dof * i + dof, dof * i:dof * i + dof] - rel).max() <= 1e-16 * max(1, float(np.abs(rel).max()))
    dc = float(np.abs(res[0][0] - res[N - 1][0]).max())
    dg = float(abs(res[0][1] - res[N - 1][1]))
    print("%s: under anchors 0 and %d cov differs by %.3g (largest entry %.3g), gain_all by %.3g (of %.6g)"
          % (name, N - 1, dc, float(np.abs(res[0][0]).max()), dg, float(res[0][1])))
    assert dc <= 1e-2 * float(np.abs(res[0][0]).max()) and dg <= 1e-2 * abs(float(res[0][1]))


# ---------------------------------------------------------------------------------------------------------------
# the host hooks and the fp64 evaluation inside the bounds, the mutants outside
# ---------------------------------------------------------------------------------------------------------------
def innov_eval(P, mutant=None, hook=False):
    d, X, pairs, K = P["d"], P["X"], P["pairs"], P["K"]
    m_cov = cd.margin_cov(X, d, pairs, K, P["anchor"], P["sig_64"], P["bS"])
    if hook:
        rec = np.stack([tph.record_of(X, d, g) for g in K])
        out = dpgo_amd.cand_innov_debug(d, rec, P["sig_64"], P["kpos"], packed(P))
        cov, S, r = out["cov"], out["S"], out["residual"]
    else:
        cov, S = cd.innovation_fp64(X, d, pairs, K, P["sig_64"], P["kappa"], P["tau"], mutant)
        r = cd.residuals(X, d, pairs, P["cands"])
    bS_ = cd.bound_S(m_cov, S, d, P["kappa"], P["tau"])
    m_r = cd.margin_residuals(X, d, pairs, P["cands"])
    return worst(cov, P["cov_ld"], m_cov), worst(S, P["S_ld"], bS_), worst(r, P["r_ld"], m_r), cov, S, r, bS_, m_r


@pytest.mark.parametrize("name", FIXTURES)
def test_block_hook_and_fp64_evaluation_lie_inside_the_bounds(fixtures_dir, name):
    for anchor, m in ((0, 9), (tmh.reference(fixtures_dir, name, 0)[1] - 1, 7)):
        P = problem(fixtures_dir, name, anchor, m, 40 + m)
        for hook in (False, True):
            wc, wS, wr, cov, S, r, bS_, m_r = innov_eval(P, hook=hook)
            print("%s anchor %d m %d%s: cov %.3g, S %.3g, r %.3g of their bounds" % (name, anchor, m, " (host hook)" if hook else "", wc, wS, wr))
            assert max(wc, wS, wr) < 1.0 and np.array_equal(cov, cov.T) and np.array_equal(S, S.T)
        # the joint test's bounds hold for numpy's fp64 route on the hook's S, under the condition rho <= 0.1
        rho = mr.rho_of(P["S_ld"], bS_)
        assert rho <= 0.1, rho
        Sinv_ld, logdet_ld, d2j_ld, gain_ld, sal = cd.joint(P["S_ld"], P["r_ld"], P["d"], P["kappa"], P["tau"])
        bI = mr.info_bound(P["S_ld"], bS_)
        Sinv = np.linalg.inv(S)
        assert worst(Sinv, Sinv_ld, bI) < 1.0
        assert abs(LD(np.linalg.slogdet(S)[1]) - logdet_ld) < mr.logdet_bound(P["S_ld"], bS_, sal)
        assert abs(LD(r @ Sinv @ r) - d2j_ld) < cd.d2_joint_bound(Sinv_ld, P["r_ld"], m_r, bI)


@pytest.mark.parametrize("mutant", cd.INNOV_MUTANTS)
def test_each_block_mutant_is_flagged_by_a_bound(fixtures_dir, mutant):
    for name in ("smallGrid3D", "ladder2"):
        P = problem(fixtures_dir, name, 0, 9, 49)
        assert max(innov_eval(P)[:3]) < 1.0
        w = innov_eval(P, mutant)
        assert max(w[:2]) > 1.0, (name, mutant, w[:3])


def select_reference(d, S, r, kappa, tau, budget, d2_max=0.0, tie=None, E_in=0.0, er_in=0.0):
    """The long-double greedy of an input with its per-step bounds, its decisions checked: (selected, steps, bg, bd).  Without a
    gate the run of a smaller budget is a prefix of this one.  E_in, er_in: the 2-norm bounds of the input's own error."""
    sel, steps, trace = cd.greedy(S, r, d, kappa, tau, budget, d2_max)
    bg, bd = cd.step_bounds(S, r, d, kappa, tau, sel, trace, E_in, er_in)
    cd.check_decisions(trace, bg, bd, d2_max, tie)
    return sel, steps, bg, bd


def select_compare(out, ref, budget):
    """A hook's output against the first `budget` steps of the reference: the order, the records and the sums within their bounds,
    the entries past n_selected as the call found them (-1 and zeros)."""
    sel, steps, bg, bd = ref[0][:budget], ref[1][:budget], ref[2], ref[3]
    assert out["n_selected"] == len(sel) and out["selected"][:len(sel)].tolist() == sel
    for t, (s, g, q, ne) in enumerate(steps):
        rec = out["steps"][t]
        assert int(rec[0]) == s and int(rec[3]) == ne
        assert abs(LD(rec[1]) - g) < bg[t, s] and abs(LD(rec[2]) - q) < bd[t, s], (t, s, float(rec[1] - g), bg[t, s], float(rec[2] - q), bd[t, s])
    assert (out["selected"][len(sel):] == -1).all() and not out["steps"][len(sel):].any()
    assert abs(LD(out["gain_selected"]) - sum(s[1] for s in steps)) <= sum(bg[t, s[0]] for t, s in enumerate(steps)) + 1e-300
    assert abs(LD(out["d2_selected"]) - sum(s[2] for s in steps)) <= sum(bd[t, s[0]] for t, s in enumerate(steps)) + 1e-300


def select_eval(d, S, r, kappa, tau, budget, d2_max=0.0, tie=None, device=None):
    """The hook against the long-double greedy; returns (hook output, selected)."""
    ref = select_reference(d, S, r, kappa, tau, budget, d2_max, tie)
    out = dpgo_amd.cand_select_debug(d, S, r, np.stack([kappa, tau], 1), budget, d2_max, device=device)
    select_compare(out, ref, budget)
    return out, ref[0]


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("m", [1, 2, 12])
def test_selection_hook_against_the_long_double_greedy(d, m):
    S, r, kappa, tau = cd.synthetic_selection(d, m, 300 + 10 * d + m)
    ref = select_reference(d, S, r, kappa, tau, m + 3)
    for budget in (0, 1, m, m + 3):
        out = dpgo_amd.cand_select_debug(d, S, r, np.stack([kappa, tau], 1), budget)
        select_compare(out, ref, budget)
        assert out["n_selected"] == min(budget, m)


def test_selection_hook_on_a_graph(fixtures_dir):
    P = problem(fixtures_dir, "smallGrid3D", 0, 9, 49)
    S, r = innov_eval(P, hook=True)[4:6]
    select_eval(P["d"], S, r, P["kappa"], P["tau"], 9)


def test_duplicate_tie_goes_to_the_lower_index_and_an_indefinite_block_is_never_chosen():
    S, r, kappa, tau = cd.synthetic_selection(3, 8, 77, dup=(2, 5))
    dof = 6
    assert np.array_equal(S[dof * 2:dof * 3], S[dof * 5:dof * 6][:, np.r_[0:dof * 2, dof * 5:dof * 6, dof * 3:dof * 5, dof * 2:dof * 3, dof * 6:dof * 8]])
    out, sel = select_eval(3, S, r, kappa, tau, 8, tie=(2, 5))
    assert sel.index(2) < sel.index(5)
    hi = cd.greedy(S, r, 3, kappa, tau, 8, mutant="tie_high")[0]
    assert hi != sel and hi.index(5) < hi.index(2)
    S, r, kappa, tau = cd.synthetic_selection(2, 7, 78, bad=3)
    out, sel = select_eval(2, S, r, kappa, tau, 7)
    assert 3 not in sel and len(sel) == 6


def test_gate_acts_on_the_conditional_d2_and_rho_is_updated():
    """Two inputs found on the CPU: a gate under which a candidate that was eligible at the start is excluded from some later step
    on -- or the other way round -- so that gating the unconditioned d2 selects differently; and one under which a residual
    that is not conditioned selects differently."""
    d, m = 3, 10
    S, r, kappa, tau = cd.synthetic_selection(d, m, 91)
    r = 3.0 * r
    for mutant in ("gate_unconditioned", "rho_not_updated"):
        found = cd.find_gate(S, r, d, kappa, tau, m, lambda g, sel: len(sel) >= 2 and cd.greedy(S, r, d, kappa, tau, m, g, mutant=mutant)[0] != sel)
        assert found is not None, mutant
        out, sel = select_eval(d, S, r, kappa, tau, m, found)
        assert cd.greedy(S, r, d, kappa, tau, m, found, mutant=mutant)[0] != sel
        print("%s: d2_max %.6g selects %s" % (mutant, found, sel))
    # a gate below every d2 excludes everything
    out = dpgo_amd.cand_select_debug(d, S, r, np.stack([kappa, tau], 1), m, 1e-12)
    assert out["n_selected"] == 0 and (out["selected"] == -1).all() and out["gain_selected"] == 0.0


# ---------------------------------------------------------------------------------------------------------------
# arguments and symbols
# ---------------------------------------------------------------------------------------------------------------
def test_cand_abi():
    assert (dpgo_amd.CAND_OK, dpgo_amd.CAND_NOT_PD, dpgo_amd.CAND_SKIPPED) == (0, 1, 2)
    # twelve ints, a long long, ten doubles
    assert C.sizeof(dpgo_amd.CandResult) == 48 + 8 + 80
    L = dpgo_amd.lib()
    header = open(os.path.join(os.path.dirname(dpgo_amd.__file__), "..", "include", "dpgo_amd.h")).read()
    for sym in ("dpgo_group_candidate_set", "dpgo_graph_candidate_set_reweighted", "dpgo_debug_cand_innov_host", "dpgo_debug_cand_innov",
                "dpgo_debug_cand_select_host", "dpgo_debug_cand_select"):
        assert sym + "(" in header and sym in dpgo_amd.SYMBOLS and hasattr(L, sym)
    for name in ("DPGO_CAND_OK 0", "DPGO_CAND_NOT_PD 1", "DPGO_CAND_SKIPPED 2"):
        assert "#define " + name in header
    for name in ("candidate_set_reweighted", "cand_innov_debug", "cand_select_debug", "CandResult"):
        assert hasattr(dpgo_amd, name)
    assert hasattr(dpgo_amd.NodeGroup, "candidate_set")
    X = np.zeros((64, 3), order="F")
    dp = X.ctypes.data_as(C.POINTER(C.c_double))
    ints = np.array([0, 1, 1, 0], np.int32)
    ip = ints.ctypes.data_as(C.POINTER(C.c_int))
    r = dpgo_amd.CandResult()
    assert L.dpgo_group_candidate_set(None, dp, 8, ip, 1, dp, 0, 0, 0.0, 1, 0, dp, dp, dp, dp, dp, ip, dp, ip, C.byref(r)) == -1
    assert L.dpgo_graph_candidate_set_reweighted(None, 0, dp, 8, 0, 0.25, ip, 1, dp, 0, 0, 0.0, 1, 0, dp, dp, dp, dp, dp, ip, dp, ip,
                                                 C.byref(r), None) == -1
    # the hooks: d, sizes, positions outside the list, missing arrays, weights that are not positive, a negative budget
    assert L.dpgo_debug_cand_innov_host(4, 1, 2, ip, dp, dp, dp, dp, dp, dp) == -1
    assert L.dpgo_debug_cand_innov_host(3, 0, 2, ip, dp, dp, dp, dp, dp, dp) == -1
    assert L.dpgo_debug_cand_innov_host(3, 1, 1, ip, dp, dp, dp, dp, dp, dp) == -1
    assert L.dpgo_debug_cand_innov_host(3, 1, 2, None, dp, dp, dp, dp, dp, dp) == -1
    bad = np.array([0, 2], np.int32)
    assert L.dpgo_debug_cand_innov_host(3, 1, 2, bad.ctypes.data_as(C.POINTER(C.c_int)), dp, dp, dp, dp, dp, dp) == -1
    n1 = np.zeros(1, np.int32)
    np_ = n1.ctypes.data_as(C.POINTER(C.c_int))
    assert L.dpgo_debug_cand_select_host(3, 1, 1, 0.0, dp, dp, dp, ip, dp, dp, np_) == -1      # (weights of zero)
    w = np.ones(2)
    wp = w.ctypes.data_as(C.POINTER(C.c_double))
    assert L.dpgo_debug_cand_select_host(3, 1, -1, 0.0, dp, dp, wp, ip, dp, dp, np_) == -1
    assert L.dpgo_debug_cand_select_host(3, 0, 1, 0.0, dp, dp, wp, ip, dp, dp, np_) == -1
    assert L.dpgo_debug_cand_select_host(3, 1, 1, 0.0, None, dp, wp, ip, dp, dp, np_) == -1
    assert L.dpgo_debug_cand_select_host(3, 1, 1, 0.0, dp, dp, wp, None, dp, dp, np_) == -1
    with pytest.raises(ValueError):
        dpgo_amd.cand_select_debug(3, np.eye(5), np.zeros(5), np.ones((1, 2)), 1)
    with pytest.raises(ValueError):
        dpgo_amd.cand_innov_debug(3, np.zeros((2, 12)), np.zeros((12, 12)), [[0, 2]], np.zeros((1, 14)))
    with pytest.raises(ValueError):
        dpgo_amd.cand_innov_debug(3, np.zeros((2, 12)), np.zeros((12, 12)), [[0, 1]], np.zeros((1, 13)))
