"""Joint covariances of arbitrary pose pairs and the loop-closure gate on the device (dpgo_amd/csrc/pairs.h):
NodeGroup.pair_covariance on tinyGrid3D x {1, 2} nodes, smallGrid3D x {1, 5} and the d = 2 ladder x 6, anchors 0 and N - 1, at
POLISHED points: the converged points of tests/test_gpu_covariance.py taken through NodeGroup.polish (anchor 0) once per
fixture.  The reference is built at that point, once per (fixture, anchor), as tests/test_gpu_covariance.py builds its own
-- the restated anchored H, the bound of the matrix, the bound bSigma of an entry of the inverse -- except that of the
long-double inverse only the columns of the poses a test asks about are solved for (the long-double Cholesky factor is
kept; a column costs two substitutions).

Bounds; nothing in them comes from the device.
  joint blocks     bSigma (tests/test_gpu_covariance.py's formula), entrywise, against the long-double inverse
  Sigma_rel, r, d2 the margins of tests/pairs_restatement.py with bS = bSigma, against the long-double restatement
  against covariance's own blocks (pairs that are edges): 2 bSigma, each side being within bSigma of the same inverse
The device's worst figure per case is printed and held below 1.
"""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cert_restatement as cert  # noqa: E402
import cov_restatement as cr  # noqa: E402
import factor_restatement as fr  # noqa: E402
import solve_restatement as sr  # noqa: E402
import pairs_restatement as pr  # noqa: E402
import test_gpu_certify as tc  # noqa: E402  (its inputs; none of its tests is imported)
import test_gpu_covariance as tgc  # noqa: E402  (its points, references and groups; none of its tests is imported)
import test_gpu_cert_proof as tp  # noqa: E402
import test_pairs_host as tph  # noqa: E402  (its seeded candidates; none of its tests is imported)

import dpgo_amd  # noqa: E402
from oracle.problem import LOSS_NONE  # noqa: E402

pytestmark = pytest.mark.gpu

LD, U = pr.LD, pr.U
CASES = [("tinyGrid3D", 1), ("tinyGrid3D", 2), ("smallGrid3D", 1), ("smallGrid3D", 5), ("ladder2", 6)]


_polished, _ref = {}, {}


def polished(fixtures_dir, name):
    """The converged point of tests/test_gpu_covariance.py after NodeGroup.polish (pose 0 held fixed): a critical point to
    rounding."""
    if name not in _polished:
        X, res, _ = tgc.make_group(fixtures_dir, name, 2).polish(tgc.converged(fixtures_dir, name))
        assert res.outcome == dpgo_amd.POLISH_CONVERGED, res.outcome
        _polished[name] = np.array(X)
    return _polished[name]


def reference(fixtures_dir, name, anchor):
    """At the polished point, computed once: X, the restated anchored H, the long-double Cholesky factor of it, bSigma by the
    formula of tests/test_gpu_covariance.py (C u kappa_2 |A^-1|_2 plus |A^-1|_2^2 | bound of the matrix |_2), the graph's edges;
    Sigma starts empty and need() fills the columns of the poses asked about."""
    key = (name, anchor)
    if key not in _ref:
        N, mm, gp, _, _ = tp.instance(fixtures_dir, name)
        d = mm.d
        dof = cr.dof_of(d)
        X = polished(fixtures_dir, name)
        n = (d + 1) * N
        S = cert.S_matrix(gp.M, X, d).toarray()
        A = cr.anchored(cr.hessian(S, X, d), anchor, dof)
        bS = np.zeros((n, n))
        Mabs = np.abs(sp.csr_matrix(gp.M).toarray())
        Lam = np.abs(cert.lambda_blocks(gp.M, X, d))
        for nn in sorted({c[1] for c in CASES if c[0] == name} | {2}):
            opt = dpgo_amd.Options.driver(LOSS_NONE, True, max_iterations=0)
            Aabs, k = tp.abs_terms_operator(N, mm, nn, opt.regularizer)
            bM = 2 * k[:, None] * U * Aabs.toarray()
            bL = tc.lambda_bound(Aabs, k, gp.M, X, d)
            b = bM.copy()
            for g in range(N):
                r = slice(N + d * g, N + d * g + d)
                b[r, r] = (1 + 2 * U) * (bM[r, r] + bL[g]) + 2 * U * (Mabs[r, r] + Lam[g])
            bS = np.maximum(bS, b)
        Sabs = Mabs.copy()
        for g in range(N):
            r = slice(N + d * g, N + d * g + d)
            Sabs[r, r] += Lam[g]
        J = np.abs(cr.tangent_basis(X, d))
        kk = 4 * d
        bH = sum(J[c].T @ bS @ J[c] for c in range(d)) + 2 * (kk + 2) * U * sum(J[c].T @ Sabs @ J[c] for c in range(d))
        lam = np.linalg.eigvalsh(A)
        assert lam[0] > 0, "the restated anchored Hessian is not positive definite at this point"
        L, kstar, _ = fr.cholesky_ld(A)
        assert kstar < 0
        bSigma = cr.C * U * float(lam[-1] / lam[0]) / float(lam[0]) + float(np.linalg.norm(bH, 2)) / float(lam[0]) ** 2
        edges = np.unique(np.stack([np.asarray(mm.ipose), np.asarray(mm.jpose)], axis=1), axis=0).astype(np.int32)
        _ref[key] = dict(N=N, d=d, dof=dof, X=X, A=A, L=L, Sigma=np.zeros(A.shape, LD), have=set(), bSigma=bSigma, edges=edges)
    return _ref[key]


def need(R, pairs):
    """Fill the columns of R["Sigma"] that belong to the poses of `pairs` (long-double solves with the kept factor)."""
    poses = sorted({int(g) for pq in pairs for g in pq} - R["have"])
    if poses:
        dof = R["dof"]
        cols = np.concatenate([np.arange(dof * g, dof * g + dof) for g in poses])
        E = np.zeros((R["A"].shape[0], len(cols)))
        E[cols, np.arange(len(cols))] = 1.0
        R["Sigma"][:, cols] = sr.solve_cholesky_ld(R["A"], E, R["L"])
        R["have"].update(poses)
    return R["Sigma"]


def node_of(grp, p):
    """The node that hosts global pose p (nodes hold consecutive ranges)."""
    off = [grp.graph.node_offset(a) for a in range(grp.graph.num_nodes)]
    return int(np.searchsorted(off, p, side="right")) - 1


def non_edge_pairs(R, anchor, seed, count=6):
    """Seeded pairs that are no edges and do not touch the anchor -- the first from the two ends of the pose range, which lie on
    different nodes of every partition -- then p == q, a pair with the anchor, and the first pair again."""
    N = R["N"]
    have = {(int(p), int(q)) for p, q in R["edges"]} | {(int(q), int(p)) for p, q in R["edges"]}
    rng = np.random.default_rng(seed)
    out = []
    lo, hi = (1, N - 1) if anchor == 0 else (0, N - 2)
    if (lo, hi) not in have:
        out.append((lo, hi))
    while len(out) < count:
        p, q = (int(v) for v in rng.integers(0, N, 2))
        if p != q and anchor not in (p, q) and (p, q) not in have and (p, q) not in out:
            out.append((p, q))
    other = (anchor + 1 + int(rng.integers(0, N - 1))) % N
    return out + [(out[1][0], out[1][0]), (anchor, other), out[0]]


def candidates_of(X, d, pairs, seed, angle=0.05):
    rng = np.random.default_rng(seed)
    c = [tph.seeded_candidate(X, d, p, q, rng, angle=angle) for p, q in pairs]
    return tuple(np.stack([np.asarray(v[i]) for v in c]) for i in range(4))


def check_against_restatement(R, anchor, pairs, cand, out):
    """The worst error / bound of the joint blocks, Sigma_rel, r and d2 of a pair_covariance result."""
    d, dof, X = R["d"], R["dof"], R["X"]
    need(R, pairs)
    worst = np.zeros(4)
    for k, (p, q) in enumerate(pairs):
        Sj = pr.joint_of(R["Sigma"], dof, p, q, anchor)
        want = pr.blocks_of(Sj, dof)
        worst[0] = max(worst[0], float(np.abs(np.asarray(out["joint"][k], LD) - want).max()) / R["bSigma"])
        if anchor in (p, q):
            zero = [b for b, hit in ((0, p == anchor), (1, True), (2, q == anchor)) if hit]
            assert not out["joint"][k][zero].any()
        ck = tuple(c[k] for c in cand)
        rel_ld = pr.rel_cov(pr.jacobian(X, d, p, q, LD), Sj)
        r_ld = pr.residual(X, d, p, q, ck, LD)
        d2_ld = pr.gate(rel_ld, r_ld, d, ck[2], ck[3], LD)[2]
        m_rel = pr.margin_rel(X, d, p, q, np.asarray(Sj, np.float64), R["bSigma"])
        m_r = pr.margin_residual(X, d, p, q, ck)
        m_d2 = pr.margin_d2(rel_ld, r_ld, d, ck[2], ck[3], m_rel, m_r)
        assert not out["not_pd"][k]
        worst[1] = max(worst[1], float(np.max(np.abs(np.asarray(out["rel"][k], LD) - rel_ld) / (m_rel + 1e-300))))
        worst[2] = max(worst[2], float(np.max(np.abs(np.asarray(out["residual"][k], LD) - r_ld) / (m_r + 1e-300))))
        worst[3] = max(worst[3], float(abs(LD(out["d2"][k]) - d2_ld) / (m_d2 + 1e-300)))
    return worst


_first = {}


@pytest.mark.parametrize("name,nn", CASES)
def test_blocks_relative_covariance_and_gate_against_the_restatement(fixtures_dir, name, nn):
    grp = tgc.make_group(fixtures_dir, name, nn)
    N = tp.instance(fixtures_dir, name)[0]
    for a in (0, N - 1):
        R = reference(fixtures_dir, name, a)
        pairs = non_edge_pairs(R, a, 41 + a)
        cand = candidates_of(R["X"], R["d"], pairs, 43 + a)
        if nn > 1:   # at least one pair whose poses lie on two nodes
            assert any(node_of(grp, p) != node_of(grp, q) for p, q in pairs), pairs
        out = grp.pair_covariance(R["X"], pairs, anchor=a, candidates=cand, threshold=16.8)
        res = out["result"]
        assert res.outcome == dpgo_amd.PAIRS_OK and res.unknowns == R["dof"] * N and res.fronts >= 1 and res.device_bytes > 0
        nposes = len({g for pq in pairs for g in pq if g != a})
        assert res.columns == R["dof"] * nposes and res.batches == (res.columns + 63) // 64 and res.pivot_min > 0
        worst = check_against_restatement(R, a, pairs, cand, out)
        print("%s x %d, anchor %d: %d columns in %d batches; joint %.3g, rel %.3g, r %.3g, d2 %.3g of their bounds"
              % ((name, nn, a, res.columns, res.batches) + tuple(worst)))
        assert worst.max() < 1.0, worst
        assert out["accept"].shape == (len(pairs),) and np.array_equal(out["accept"], out["d2"] <= 16.8)
        # the pair listed twice: the same bits; p == q: the marginal three times, no relative uncertainty beyond rounding
        assert np.array_equal(out["joint"][-1], out["joint"][0]) and np.array_equal(out["rel"][-1], out["rel"][0])
        k = len(pairs) - 3
        assert np.array_equal(out["joint"][k][0], out["joint"][k][1]) and np.array_equal(out["joint"][k][0], out["joint"][k][2])
        # every partition: other orderings, other fronts, the same blocks
        first = _first.setdefault((name, a), out)
        assert np.abs(out["joint"] - first["joint"]).max() <= 2 * R["bSigma"]
        # the same bits on a second call, with and without the candidates
        again = grp.pair_covariance(R["X"], pairs, anchor=a)
        assert "d2" not in again and np.array_equal(again["joint"], out["joint"]) and np.array_equal(again["rel"], out["rel"])


@pytest.mark.parametrize("name,nn", [("tinyGrid3D", 2), ("smallGrid3D", 5), ("ladder2", 6)])
def test_edge_pairs_agree_with_the_selected_inversion(fixtures_dir, name, nn):
    grp = tgc.make_group(fixtures_dir, name, nn)
    R = reference(fixtures_dir, name, 0)
    edges = R["edges"][::max(len(R["edges"]) // 24, 1)]
    marg, cross, res = grp.covariance(R["X"], pairs=edges)
    out = grp.pair_covariance(R["X"], edges)
    assert res.outcome == dpgo_amd.COV_OK and out["result"].outcome == dpgo_amd.PAIRS_OK
    tol = 2 * R["bSigma"]
    assert np.abs(out["joint"][:, 1] - cross).max() <= tol
    assert np.abs(out["joint"][:, 0] - marg[edges[:, 0]]).max() <= tol and np.abs(out["joint"][:, 2] - marg[edges[:, 1]]).max() <= tol
    assert np.abs(cross).max() > 100 * tol   # (an orientation that is wrong would show)


def test_a_pair_alone_and_among_forty_others_has_the_same_bits(fixtures_dir):
    R = reference(fixtures_dir, "smallGrid3D", 0)
    grp = tgc.make_group(fixtures_dir, "smallGrid3D", 5)
    N = R["N"]
    rng = np.random.default_rng(77)
    p, q = 17, 101
    cand = candidates_of(R["X"], 3, [(p, q)], 5)
    alone = grp.pair_covariance(R["X"], [(p, q)], candidates=cand)
    others = [tuple(int(v) for v in rng.integers(1, N, 2)) for _ in range(40)]
    pairs = others[:23] + [(p, q)] + others[23:]
    many_c = candidates_of(R["X"], 3, pairs, 6)
    for i in range(4):
        many_c[i][23] = cand[i][0]
    many = grp.pair_covariance(R["X"], pairs, candidates=many_c)
    assert many["result"].batches >= 3 and alone["result"].batches == 1
    for key in ("joint", "rel", "d2", "residual"):
        assert np.array_equal(many[key][23], alone[key][0]), key


def test_candidates_equal_to_the_estimate_and_rotated_by_half_a_radian(fixtures_dir):
    for name, nn in (("smallGrid3D", 5), ("ladder2", 6)):
        R = reference(fixtures_dir, name, 0)
        d, dof, X = R["d"], R["dof"], R["X"]
        grp = tgc.make_group(fixtures_dir, name, nn)
        pairs = non_edge_pairs(R, 0, 3)[:4]
        own = [pr.relative(X, d, p, q) for p, q in pairs]
        kappa, tau = np.full(len(pairs), 20.0), np.full(len(pairs), 10.0)
        same = grp.pair_covariance(X, pairs, candidates=(np.stack([o[0] for o in own]), np.stack([o[1] for o in own]), kappa, tau))
        # r: twice the rounding of R~^T R_pq and t_pq (tests/pairs_restatement.py: m_r) -- the candidate is numpy's fp64 relative
        # pose, the device's is its own, each within m_r of the exact one; and S >= Omega^-1, so d2 <= max(tau, 2 kappa) |r|^2
        for k, (p, q) in enumerate(pairs):
            m_r = 2 * pr.margin_residual(X, d, p, q, (own[k][0], own[k][1]))
            assert np.all(np.abs(same["residual"][k]) <= m_r) and same["d2"][k] <= 40.0 * float(m_r @ m_r)
        cand = candidates_of(X, d, pairs, 9, angle=0.5)
        rot = grp.pair_covariance(X, pairs, candidates=cand)
        need(R, pairs)
        for k, (p, q) in enumerate(pairs):
            ck = tuple(c[k] for c in cand)
            Sj = pr.joint_of(R["Sigma"], dof, p, q, 0)
            rel_ld = pr.rel_cov(pr.jacobian(X, d, p, q, LD), Sj)
            r_ld = pr.residual(X, d, p, q, ck, LD)
            d2_ld = pr.gate(rel_ld, r_ld, d, ck[2], ck[3], LD)[2]
            m_rel = pr.margin_rel(X, d, p, q, np.asarray(Sj, np.float64), R["bSigma"])
            m_d2 = pr.margin_d2(rel_ld, r_ld, d, ck[2], ck[3], m_rel, pr.margin_residual(X, d, p, q, ck))
            assert abs(float(np.linalg.norm(rot["residual"][k][d:])) - 0.5) <= 1e-9
            assert rot["d2"][k] >= float(d2_ld) - m_d2 and rot["d2"][k] > same["d2"][k] + 1e-3


def test_a_point_that_is_no_minimum(fixtures_dir):
    R = reference(fixtures_dir, "smallGrid3D", 0)
    grp = tgc.make_group(fixtures_dir, "smallGrid3D", 2)
    pairs = non_edge_pairs(R, 0, 3)
    cand = candidates_of(R["X"], 3, pairs, 4)
    before = grp.pair_covariance(R["X"], pairs, candidates=cand)
    Z = cr.random_rotations_point(R["X"], R["d"], 5)
    bad = grp.pair_covariance(Z, pairs, candidates=cand, threshold=10.0)
    assert bad["result"].outcome == dpgo_amd.PAIRS_NOT_PD and not bad["accept"].any()
    assert not bad["joint"].any() and not bad["rel"].any() and not bad["d2"].any()
    after = grp.pair_covariance(R["X"], pairs, candidates=cand)
    assert after["result"].outcome == dpgo_amd.PAIRS_OK
    for key in ("joint", "rel", "d2", "residual"):
        assert np.array_equal(before[key], after[key])


def device_free_bytes():
    """hipMemGetInfo of the HIP runtime the library itself is linked against, behind a device synchronise."""
    import ctypes as C
    L = dpgo_amd.lib()
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert L.hipDeviceSynchronize() == 0 and L.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_skipped_allocates_nothing_and_runs_where_covariance_is_skipped(fixtures_dir):
    R = reference(fixtures_dir, "smallGrid3D", 0)
    grp = tgc.make_group(fixtures_dir, "smallGrid3D", 2)
    pairs = non_edge_pairs(R, 0, 3)[:2]
    grp.pair_covariance(R["X"], pairs, max_bytes=1)   # (the certificate's buffers and M's values come here)
    free0 = device_free_bytes()
    out = grp.pair_covariance(R["X"], pairs, max_bytes=1)
    assert device_free_bytes() == free0
    res = out["result"]
    assert res.outcome == dpgo_amd.PAIRS_SKIPPED and not out["joint"].any() and not out["rel"].any()
    assert res.unknowns == 6 * R["N"] and res.fronts >= 4 and res.device_bytes > 1 and res.stationarity > 0 and 0 < res.columns <= 24
    cov_bytes = grp.covariance(R["X"], max_bytes=1)[2].device_bytes
    print("smallGrid3D, 2 pairs: pair_covariance predicts %d bytes, covariance %d" % (res.device_bytes, cov_bytes))
    assert res.device_bytes < cov_bytes
    between = (res.device_bytes + cov_bytes) // 2
    assert grp.covariance(R["X"], max_bytes=between)[2].outcome == dpgo_amd.COV_SKIPPED
    assert grp.pair_covariance(R["X"], pairs, max_bytes=res.device_bytes - 1)["result"].outcome == dpgo_amd.PAIRS_SKIPPED
    ok = grp.pair_covariance(R["X"], pairs, max_bytes=between)
    assert ok["result"].outcome == dpgo_amd.PAIRS_OK and ok["result"].device_bytes == res.device_bytes
    assert check_joint(R, pairs, ok) < 1.0


def check_joint(R, pairs, out):
    need(R, pairs)
    return max(float(np.abs(np.asarray(out["joint"][k], LD) - pr.blocks_of(pr.joint_of(R["Sigma"], R["dof"], p, q, 0), R["dof"])).max())
               for k, (p, q) in enumerate(pairs)) / R["bSigma"]


def test_refusals(fixtures_dir):
    path, N, mm, gp, X0 = tc.problem(fixtures_dir, "smallGrid3D")
    R = reference(fixtures_dir, "smallGrid3D", 0)
    X = R["X"]
    G = dpgo_amd.read_g2o(path, 2)
    hub = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(dpgo_amd.LOSS_HUBER, True), X0=X0)
    with pytest.raises(RuntimeError):
        hub.group.pair_covariance(X, [(1, 5)])          # a robust loss
    part = dpgo_amd.NodeGroup(G, [0], dpgo_amd.Options.driver(LOSS_NONE, True))
    with pytest.raises(RuntimeError):
        part.pair_covariance(X, [(1, 5)])               # a group that does not host every node
    grp = tgc.make_group(fixtures_dir, "smallGrid3D", 2)
    for bad in (dict(anchor=N), dict(anchor=-1)):
        with pytest.raises(RuntimeError):
            grp.pair_covariance(X, [(1, 5)], **bad)
    for pairs in ([(0, N)], [(-1, 0)]):
        with pytest.raises(RuntimeError):
            grp.pair_covariance(X, pairs)
    with pytest.raises(RuntimeError):
        grp.pair_covariance(X[:-1], [(1, 5)])
    c = candidates_of(X, 3, [(1, 5)], 1)
    for kappa, tau in ((0.0, 1.0), (1.0, -2.0)):
        with pytest.raises(RuntimeError):
            grp.pair_covariance(X, [(1, 5)], candidates=(c[0], c[1], [kappa], [tau]))
    # a null output behind a valid group: joint, rel, the gate of a call with candidates, the result
    import ctypes as C
    L = dpgo_amd.lib()
    Xf = np.asfortranarray(X)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    P = np.array([[1, 5]], np.int32)
    ip = P.ctypes.data_as(C.POINTER(C.c_int))
    joint, rel, gate, res = np.zeros(3 * 36), np.zeros(36), np.zeros(8), dpgo_amd.PairsResult()
    cc = dpgo_amd.pack_candidates(3, 1, *c)
    call = lambda j, r, cand, g, out: L.dpgo_group_pair_covariance(grp._h, dp(Xf), Xf.shape[0], 0, 0, ip, 1, cand, j, r, g, out)
    assert call(dp(joint), dp(rel), dp(cc), dp(gate), C.byref(res)) == 0 and res.outcome == dpgo_amd.PAIRS_OK
    assert call(None, dp(rel), None, None, C.byref(res)) == -1 and call(dp(joint), None, None, None, C.byref(res)) == -1
    assert call(dp(joint), dp(rel), dp(cc), None, C.byref(res)) == -1 and call(dp(joint), dp(rel), None, None, None) == -1
    assert L.dpgo_group_pair_covariance(grp._h, dp(Xf), Xf.shape[0], 0, 0, None, 1, None, dp(joint), dp(rel), None, C.byref(res)) == -1
    assert grp.pair_covariance(X, [(1, 5)])["result"].outcome == dpgo_amd.PAIRS_OK


def test_pair_covariance_does_not_disturb_the_optimiser(fixtures_dir):
    """30 AMM-PGO# iterations with a call on a sibling trivial-loss group after every fifth: bit for bit the run without."""
    path = tc.problem(fixtures_dir, "smallGrid3D")[0]
    runs = []
    for with_call in (False, True):
        drv = dpgo_amd.DistPGO(dpgo_amd.read_g2o(path, 2), dpgo_amd.Options.driver(LOSS_NONE, True))
        sib = tc.group(path, 2)[0] if with_call else None
        trace = []
        for it in range(30):
            assert drv.step() == 0
            if with_call and it % 5 == 4:
                assert sib.pair_covariance(drv.X(), [(3, 90), (7, 7)])["result"].outcome in (dpgo_amd.PAIRS_OK, dpgo_amd.PAIRS_NOT_PD)
            trace.append([getattr(drv.group.results(a), f) for a in range(2) for f in ("fobj", "gamma", "gradFnorm", "Gk")])
        runs.append((np.array(drv.X()), [drv.group[a].Xk() for a in range(2)], np.array(trace)))
    assert np.array_equal(runs[0][0], runs[1][0])
    for a in range(2):
        assert np.array_equal(runs[0][1][a], runs[1][1][a])
    assert np.array_equal(runs[0][2], runs[1][2])


def test_reweighted_with_unit_weights_is_the_group_call(fixtures_dir):
    path = tc.problem(fixtures_dir, "smallGrid3D")[0]
    R = reference(fixtures_dir, "smallGrid3D", 0)
    G = dpgo_amd.read_g2o(path, 2)
    pairs = non_edge_pairs(R, 0, 3)
    cand = candidates_of(R["X"], 3, pairs, 4)
    got = dpgo_amd.pair_covariance_reweighted(G, R["X"], LOSS_NONE, pairs, candidates=cand)
    want = tgc.make_group(fixtures_dir, "smallGrid3D", 2).pair_covariance(R["X"], pairs, candidates=cand)
    assert got["result"].outcome == dpgo_amd.PAIRS_OK and got["summary"].num_downweighted == 0
    for key in ("joint", "rel", "d2", "residual"):
        assert np.array_equal(got[key], want[key])


# ---------------------------------------------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------------------------------------------
INFO = "100 0 0 0 0 0   100 0 0 0 0   100 0 0 0   25 0 0   25 0   25"
CANDIDATES = [(3, 90, "2.0 1.0 -1.0   0.1 -0.2 0.3 0.9273618495495703"), (10, 77, "0.5 -3.0 1.0   0 0 0 1"),
              (0, 124, "4.0 4.0 4.0   0.5 0.5 0.5 0.5"), (61, 61, "0 0 0   0 0 0 1"), (3, 90, "2.0 1.0 -1.0   0.1 -0.2 0.3 0.9273618495495703")]


def test_dist_pgo_gate_candidates_flag(fixtures_dir, tmp_path):
    """--gate_candidates FILE --gate_report FILE adds the report and one line after the summary; the report holds
    NodeGroup.pair_covariance's d2 and Sigma_rel bit for bit (the candidates read by the same loader)."""
    import subprocess
    exe = os.path.join(tc.ROOT, "dpgo_amd", "dist_pgo")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    cand = tmp_path / "cand.g2o"
    cand.write_text("".join("EDGE_SE3:QUAT %d %d   %s   %s\n" % (p, q, pose, INFO) for p, q, pose in CANDIDATES))
    path = os.path.join(fixtures_dir, "smallGrid3D.g2o")
    base = [exe, "--dataset", path, "--num_nodes", "2", "--iters", "200", "--dist_init", "false", "--save", "false"]
    run = subprocess.run(base + ["--gate_candidates", str(cand), "--gate_report", "gate.txt"], capture_output=True, text=True,
                         cwd=tmp_path, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = [l for l in run.stdout.splitlines() if l.startswith("gate: ")]
    assert len(lines) == 1 and run.stdout.rstrip().splitlines()[-1] == lines[0]
    drv = dpgo_amd.DistPGO(dpgo_amd.read_g2o(path, 2), dpgo_amd.Options.driver(LOSS_NONE, True))
    for _ in range(200):
        assert drv.step() == 0
    I, J, R, t, kappa, tau = dpgo_amd.read_g2o(str(cand), 1).edges()
    assert I.tolist() == [c[0] for c in CANDIDATES] and J.tolist() == [c[1] for c in CANDIDATES]
    want = drv.group.pair_covariance(drv.X(), np.stack([I, J], axis=1), candidates=(R, t, kappa, tau))
    res = want["result"]
    f = lines[0].split()
    assert f[1] == "OK" and int(f[2]) == len(CANDIDATES) and int(f[3]) == res.columns and int(f[5]) == res.device_bytes
    rows = np.loadtxt(tmp_path / "gate.txt")
    iu = np.triu_indices(6)
    assert np.array_equal(rows[:, 0], I) and np.array_equal(rows[:, 1], J) and np.all(rows[:, 3] == 6)
    assert np.array_equal(rows[:, 2], want["d2"]) and np.array_equal(rows[:, 4], want["not_pd"].astype(float))
    assert np.array_equal(rows[:, 5:], np.stack([m[iu] for m in want["rel"]]))
    assert want["d2"][3] <= 1e-20 and want["d2"][0] > 1.0 and np.array_equal(rows[0], rows[4])
    # a robust loss: the line says why there is no gate; one flag without the other is an error
    hub = subprocess.run(base[:-6] + ["--iters", "5", "--dist_init", "false", "--save", "false", "--loss", "huber", "--gate_candidates",
                                      str(cand), "--gate_report", "g2.txt"], capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert hub.returncode == 0 and "gate: not computed" in hub.stdout and not (tmp_path / "g2.txt").exists()
    one = subprocess.run(base[:-6] + ["--iters", "1", "--dist_init", "false", "--save", "false", "--gate_candidates", str(cand)],
                         capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert one.returncode != 0


def test_cpp_facade_pair_covariances(fixtures_dir, tmp_path):
    """examples/facade_mm.cpp with `pairs FILE`: DPGOHashGroup::pair_covariances after the loop, on stderr; stdout the same trace
    as without; joint, rel and gate those of NodeGroup.pair_covariance bit for bit; candidates of the wrong length refused."""
    import subprocess
    exe = os.path.join(tc.ROOT, "dpgo_amd", "facade_mm")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    cand = tmp_path / "cand.g2o"
    cand.write_text("".join("EDGE_SE3:QUAT %d %d   %s   %s\n" % (p, q, pose, INFO) for p, q, pose in CANDIDATES))
    path = os.path.join(fixtures_dir, "smallGrid3D.g2o")
    args = [exe, path, "2", "200", "trivial", "1"]
    plain = subprocess.run(args, check=True, capture_output=True, text=True, timeout=300)
    out = subprocess.run(args + ["pairs", str(cand)], check=True, capture_output=True, text=True, timeout=300)
    assert out.stdout == plain.stdout and "pairs" not in plain.stderr
    lines = [l.split() for l in out.stderr.splitlines() if l.startswith("pairs: ")]
    drv = dpgo_amd.DistPGO(dpgo_amd.read_g2o(path, 2), dpgo_amd.Options.driver(LOSS_NONE, True))
    for _ in range(200):
        assert drv.step() == 0
    I, J, R, t, kappa, tau = dpgo_amd.read_g2o(str(cand), 1).edges()
    want = drv.group.pair_covariance(drv.X(), np.stack([I, J], axis=1), candidates=(R, t, kappa, tau))
    res = want["result"]
    m = len(CANDIDATES)
    assert len(lines) == 3 * m + 2 and lines[-2][1] == "OK" and int(lines[-2][2]) == res.columns and int(lines[-2][3]) == res.batches
    got = {w: np.array([[float(v) for v in l[3:]] for l in lines if l[1] == w]) for w in ("joint", "rel", "gate")}
    assert [int(l[2]) for l in lines if l[1] == "gate"] == list(range(m))
    assert np.array_equal(got["joint"], want["joint"].reshape(m, -1)) and np.array_equal(got["rel"], want["rel"].reshape(m, -1))
    assert np.array_equal(got["gate"][:, 0], want["d2"]) and np.array_equal(got["gate"][:, 1], want["not_pd"].astype(float))
    assert np.array_equal(got["gate"][:, 2:], want["residual"])
    assert lines[-1][1:] == ["short", "candidates", "-1", "0"]
