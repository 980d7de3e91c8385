"""Host side of the joint pair covariances and the gate (dpgo_amd/csrc/pairs.h): the restatement (tests/pairs_restatement.py)
against central differences along cov_restatement.retract, the column plan and the per-pair arithmetic through their debug
hooks, the margins of Sigma_rel, r and d^2 against the long-double restatement, and the C ABI.  No GPU.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cert_restatement as cert  # noqa: E402
import cov_restatement as cr  # noqa: E402
import factor_restatement as fr  # noqa: E402
import pairs_restatement as pr  # noqa: E402
import solve_restatement as sr  # noqa: E402
import test_certify_host as tch  # noqa: E402  (its converged points; none of its tests is imported)
import test_covariance_host as tcov  # noqa: E402  (its restated Hessians; none of its tests is imported)
import test_gpu_cert_proof as tp  # noqa: E402  (the d = 2 graph; none of its tests is imported)
import test_polish_host as tph  # noqa: E402  (its points of the d = 2 graph; none of its tests is imported)

import dpgo_amd  # noqa: E402

LD, U = pr.LD, pr.U
FIXTURES = ["tinyGrid3D", "smallGrid3D", "ladder2"]
_fx = {}


def fixture(fixtures_dir, name):
    """(d, N, converged X, the restated H) of a fixture: the points of tests/test_certify_host.py, and for the d = 2 ladder the
    oracle's iterate after 300 iterations (tests/test_polish_host.py)."""
    if name not in _fx:
        if name == "ladder2":
            gp, X = tph.start_point(fixtures_dir, name, 300)
            H = cr.hessian(cert.S_matrix(gp.M, X, gp.d), X, gp.d)
        else:
            gp, X, H, _ = tcov.restated(fixtures_dir, name)
        _fx[name] = (gp.d, X.shape[0] // (gp.d + 1), X, H)
    return _fx[name]


def seeded_pairs(N, anchor, seed, count=6):
    """`count` seeded pairs p != q away from the anchor, then p == q, a pair with the anchor, and the first pair again."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        p, q = (int(v) for v in rng.integers(0, N, 2))
        if p != q and anchor not in (p, q):
            out.append((p, q))
    other = (anchor + 1 + int(rng.integers(0, N - 1))) % N
    return out + [(out[0][0], out[0][0]), (anchor, other), out[0]]


def seeded_candidate(X, d, p, q, rng, angle=0.05, shift=0.05):
    """(R~, t~, kappa, tau): the estimate's own relative pose moved by a seeded rotation of `angle` rad and a seeded
    translation of length `shift`."""
    dof = cr.dof_of(d)
    Rpq, tpq = pr.relative(X, d, p, q, LD)
    w = rng.standard_normal(dof - d)
    w *= angle / max(np.linalg.norm(w), 1e-300)
    s = rng.standard_normal(d)
    s *= shift / max(np.linalg.norm(s), 1e-300)
    Rt = np.asarray(Rpq @ pr.exp_so(w, d, LD), np.float64)
    return Rt, np.asarray(tpq, np.float64) + s, float(rng.uniform(5, 50)), float(rng.uniform(5, 50))


# ---------------------------------------------------------------------------------------------------------------
# the restatement against central differences
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tinyGrid3D", "ladder2"])
def test_jacobian_is_the_central_difference_along_the_retraction(fixtures_dir, name):
    """d/de (t_pq, vee Log(R_pq(X)^T R_pq(retract(X, e v)))) at e = 0 against J [v_p ; v_q], seeded pairs and directions, at the
    converged point and at a point with seeded random rotations.  The difference quotient with step h carries h^2 times a
    third derivative of order (1 + |t_pq|) |v|^3 and the rounding 10 u (1 + |t_pq|) / h of the two points; a sign or a frame
    that is wrong moves a component by the order of |v| itself."""
    d, N, Xc, _ = fixture(fixtures_dir, name)
    dof = cr.dof_of(d)
    rng = np.random.default_rng(71)
    h = 1e-5
    for X in (Xc, cr.random_rotations_point(Xc, d, 9)):
        for p, q in seeded_pairs(N, 0, 5, count=4)[:5]:
            J = pr.jacobian(X, d, p, q)
            R0, t0 = pr.relative(X, d, p, q)
            for _ in range(3):
                vp, vq = rng.standard_normal(dof), rng.standard_normal(dof)
                v = pr.pair_tangent(N, d, p, q, vp, vq)
                f = []
                for e in (h, -h):
                    Z = cr.retract(X, e * v, d)
                    R1, t1 = pr.relative(Z, d, p, q)
                    f.append(np.concatenate([t1, pr.log_so(R0.T @ R1, d)]))
                fd = (f[0] - f[1]) / (2 * h)
                want = J @ np.concatenate([vp, vq]) if p != q else J[:, :dof] @ (vp + vq) + J[:, dof:] @ (vp + vq)
                nv = np.linalg.norm(v)
                tol = 4 * (h * h * nv ** 3 + 10 * U / h) * (1 + np.linalg.norm(t0))
                assert np.abs(fd - want).max() <= tol, (name, p, q, fd, want)
                assert p == q or np.abs(want).max() > 1e3 * tol   # (the check has teeth)


@pytest.mark.parametrize("d", [2, 3])
def test_omega_is_the_second_difference_of_the_edge_term(d):
    """One edge's own term of F, 1/2 (kappa |R_pq - R~|_F^2 + tau |t_pq - t~|^2), at zero residual along directions of
    (dt_pq, domega_pq): the second central difference in long double against v' Omega v.  Step 1e-4: truncation h^2 / 12
    times a fourth derivative of order kappa |v|^4, rounding 4 u_ld F / h^2 with F of order h^2."""
    dof = cr.dof_of(d)
    rng = np.random.default_rng(5 + d)
    kappa, tau = 7.5, 3.25
    Om = pr.omega(d, kappa, tau)
    Rt = pr.exp_so(rng.standard_normal(dof - d), d, LD)
    tt = np.asarray(rng.standard_normal(d), LD)
    h = LD(1e-4)
    for _ in range(5):
        v = rng.standard_normal(dof)
        v /= np.linalg.norm(v)

        def term(e):
            R = Rt @ pr.exp_so(e * np.asarray(v[d:], LD), d, LD)
            t = tt + e * np.asarray(v[:d], LD)
            return 0.5 * (kappa * np.sum((R - Rt) ** 2) + tau * np.sum((t - tt) ** 2))

        fd = float((term(h) - 2 * term(LD(0)) + term(-h)) / (h * h))
        want = float(v @ Om @ v)
        assert abs(fd - want) <= 1e-7 * (kappa + tau), (d, fd, want)
    assert np.array_equal(np.diag(Om), [tau] * d + [2 * kappa] * (dof - d))


# ---------------------------------------------------------------------------------------------------------------
# the column plan
# ---------------------------------------------------------------------------------------------------------------
def test_column_plan():
    # distinct poses, ascending, the anchor dropped, a pair listed twice, p == q
    pl = dpgo_amd.pairs_plan_debug(6, 4, [[9, 2], [4, 7], [7, 7], [2, 9], [9, 2], [4, 4]])
    assert pl["poses"].tolist() == [2, 7, 9] and pl["columns"] == 18 and pl["batches"] == 1 and pl["kb"] == 32
    assert pl["pair_col"].tolist() == [[12, 0], [-1, 6], [6, 6], [0, 12], [12, 0], [-1, -1]]
    # dof = 6: ten poses fill 60 columns, the eleventh straddles the batches (columns 60 ... 65): the third pose of the second
    # group of 16 columns that is not whole -- and 22 poses need three batches
    pairs = [[2 * i + 1, 2 * i + 3] for i in range(10)]
    pl = dpgo_amd.pairs_plan_debug(6, 0, pairs)
    assert pl["poses"].tolist() == list(range(1, 23, 2)) and pl["columns"] == 66 and pl["batches"] == 2 and pl["kb"] == 64
    assert pl["pair_col"][9].tolist() == [54, 60] and 60 < 64 < 60 + 6
    pl = dpgo_amd.pairs_plan_debug(6, 0, [[i, i + 1] for i in range(1, 22)])
    assert pl["columns"] == 132 and pl["batches"] == 3
    # the third pose of a batch of 16 columns straddles its edge at dof = 6 (columns 12 ... 17)
    pl = dpgo_amd.pairs_plan_debug(6, 0, [[1, 2], [3, 3]])
    assert pl["pair_col"].tolist() == [[0, 6], [12, 12]] and pl["columns"] == 18 and pl["kb"] == 32
    # d = 2, nothing but the anchor, no pairs
    assert dpgo_amd.pairs_plan_debug(3, 1, [[1, 1]])["columns"] == 0
    pl = dpgo_amd.pairs_plan_debug(3, 0, np.zeros((0, 2), np.int32))
    assert pl["columns"] == 0 and pl["batches"] == 0 and pl["kb"] == 16 and len(pl["poses"]) == 0
    assert dpgo_amd.pairs_plan_debug(3, 0, [[5, 6]])["kb"] == 16


# ---------------------------------------------------------------------------------------------------------------
# the margins, and the per-pair arithmetic on the host
# ---------------------------------------------------------------------------------------------------------------
_sig = {}


def inverse(fixtures_dir, name, anchor, poses):
    """(the columns of Sigma that belong to `poses` in long double, scattered into an otherwise zero n x n array; Sigma in
    fp64; bS) of the restated anchored H: the long-double Cholesky solve of the unit columns, numpy's inverse, and the
    factorisation's part of the blocks' bound (cov_restatement: C u kappa_2 |A^-1|_2)."""
    key = (name, anchor)
    if key not in _sig:
        d, N, X, H = fixture(fixtures_dir, name)
        dof = cr.dof_of(d)
        A = cr.anchored(H, anchor, dof)
        A = (A + A.T) / 2
        lam = np.linalg.eigvalsh(A)
        assert lam[0] > 0
        L, kstar, _ = fr.cholesky_ld(A)
        assert kstar < 0
        cols = np.concatenate([np.arange(dof * g, dof * g + dof) for g in sorted(set(poses))])
        E = np.zeros((A.shape[0], len(cols)))
        E[cols, np.arange(len(cols))] = 1.0
        Sld = np.zeros(A.shape, LD)
        Sld[:, cols] = sr.solve_cholesky_ld(A, E, L)
        _sig[key] = (Sld, np.linalg.inv(A), cr.C * U * float(lam[-1] / lam[0]) / float(lam[0]))
    return _sig[key]


def record_of(X, d, p):
    t, Y = pr.record(X, d, p)
    return np.concatenate([t, Y.reshape(-1)])


@pytest.mark.parametrize("name", FIXTURES)
def test_fp64_restatement_against_the_margins(fixtures_dir, name):
    """Sigma_rel, r and d^2 of the plain fp64 restatement (numpy's inverse of the restated anchored H) and of the library's
    per-pair code on the host (pairs_gate_debug, fed the same fp64 blocks) against the long-double restatement: Sigma_rel and
    d^2 use at most a quarter of pairs_restatement's margins, which are computed here with the factorisation's part of the
    blocks' bound alone.  The residual's margin is no modelled quantity but a count of d + 2 roundings, of which the one that
    rounds t_pq alone can take a fifth: r is held inside its margin (the worst seen is a third), not inside a quarter."""
    d, N, X, _ = fixture(fixtures_dir, name)
    dof = cr.dof_of(d)
    worst = np.zeros(6)
    for anchor in (0, N - 1):
        pairs = seeded_pairs(N, anchor, 17 + anchor)
        Sld, S64, bS = inverse(fixtures_dir, name, anchor, [g for pq in pairs for g in pq])
        rng = np.random.default_rng(313 + anchor)
        for p, q in pairs:
            cand = seeded_candidate(X, d, p, q, rng)
            Jl = pr.jacobian(X, d, p, q, LD)
            rel_ld = pr.rel_cov(Jl, pr.joint_of(Sld, dof, p, q, anchor))
            r_ld = pr.residual(X, d, p, q, cand, LD)
            d2_ld = pr.gate(rel_ld, r_ld, d, cand[2], cand[3], LD)[2]
            Sj = pr.joint_of(S64, dof, p, q, anchor)
            assert np.abs(np.asarray(Sj, LD) - pr.joint_of(Sld, dof, p, q, anchor)).max() <= bS / 4
            m_rel = pr.margin_rel(X, d, p, q, Sj, bS)
            m_r = pr.margin_residual(X, d, p, q, cand)
            m_d2 = pr.margin_d2(rel_ld, r_ld, d, cand[2], cand[3], m_rel, m_r)
            # the numpy restatement in fp64
            rel = pr.rel_cov(pr.jacobian(X, d, p, q), Sj)
            r = pr.residual(X, d, p, q, cand)
            d2 = pr.gate(rel, r, d, cand[2], cand[3])[2]
            # the library's arithmetic on the host
            rel_h, (d2_h, not_pd, r_h) = dpgo_amd.pairs_gate_debug(d, record_of(X, d, p), record_of(X, d, q), pr.blocks_of(Sj, dof), cand)
            assert not not_pd
            tiny = 1e-300
            got = [np.max(np.abs(np.asarray(rel, LD) - rel_ld) / (m_rel + tiny)), np.max(np.abs(np.asarray(r, LD) - r_ld) / (m_r + tiny)),
                   abs(LD(d2) - d2_ld) / (m_d2 + tiny),
                   np.max(np.abs(np.asarray(rel_h, LD) - rel_ld) / (m_rel + tiny)), np.max(np.abs(np.asarray(r_h, LD) - r_ld) / (m_r + tiny)),
                   abs(LD(d2_h) - d2_ld) / (m_d2 + tiny)]
            worst = np.maximum(worst, np.asarray(got, np.float64))
            if p == q:
                assert np.abs(rel_h).max() <= m_rel.max()   # (T_pp is the identity: no uncertainty)
    print("%s: worst error / margin -- numpy fp64: rel %.3g, r %.3g, d2 %.3g; host twin: rel %.3g, r %.3g, d2 %.3g" % ((name,) + tuple(worst)))
    assert max(worst[0], worst[2], worst[3], worst[5]) <= 0.25 and max(worst[1], worst[4]) < 1.0, worst


def test_gate_hook_edge_cases():
    """The logarithm next to pi and next to the identity, a candidate equal to the relative pose, S that is not positive
    definite, bad arguments."""
    rng = np.random.default_rng(3)
    for d in (2, 3):
        dof = cr.dof_of(d)
        recp = np.concatenate([np.zeros(d), np.eye(d).reshape(-1)])
        for angle in (1e-10, 1e-3, 1.0, 3.0, np.pi - 1e-10, np.pi):
            w = rng.standard_normal(dof - d)
            w *= angle / np.linalg.norm(w)
            if d == 2:
                w = np.abs(w)
            Rq = np.asarray(pr.exp_so(w, d, LD), np.float64)
            recq = np.concatenate([np.ones(d), Rq.T.reshape(-1)])
            rel, (d2, not_pd, r) = dpgo_amd.pairs_gate_debug(d, recp, recq, np.zeros((3, dof, dof)), (np.eye(d), np.zeros(d), 2.0, 4.0))
            assert not not_pd and not rel.any()
            # |w| is the angle; its direction is w's up to the sign at pi itself
            assert abs(np.linalg.norm(r[d:]) - angle) <= 1e-9 * max(angle, 1) and np.array_equal(r[:d], np.ones(d))
            if angle < np.pi - 1e-12:
                assert np.abs(r[d:] - w).max() <= 1e-6 * max(angle, 1e-3), (d, angle, r[d:], w)
            else:
                assert min(np.abs(r[d:] - w).max(), np.abs(r[d:] + w).max()) <= 1e-6
            # Omega^-1 alone: d^2 = tau |dt|^2 + 2 kappa |w|^2
            assert abs(d2 - (4.0 * d + 2 * 2.0 * angle ** 2)) <= 1e-9 * d2
        same = dpgo_amd.pairs_gate_debug(d, recp, recq, np.zeros((3, dof, dof)), (Rq, np.ones(d), 1.0, 1.0))[1]
        assert same[0] <= 1e-28 and np.abs(same[2]).max() <= 1e-15
        neg = np.zeros((3, dof, dof))
        neg[2] = -10 * np.eye(dof)
        bad = dpgo_amd.pairs_gate_debug(d, recp, recq, neg, (Rq, np.ones(d), 1.0, 1.0))[1]
        assert bad[1] and bad[0] == 0.0
        for kappa, tau in ((0.0, 1.0), (1.0, -1.0), (float("nan"), 1.0)):
            with pytest.raises(RuntimeError):
                dpgo_amd.pairs_gate_debug(d, recp, recq, neg, (Rq, np.ones(d), kappa, tau))
    with pytest.raises(RuntimeError):
        dpgo_amd.pairs_gate_debug(4, np.zeros(20), np.zeros(20), np.zeros(3 * 100), None)


# ---------------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------------
def test_pairs_abi():
    assert (dpgo_amd.PAIRS_OK, dpgo_amd.PAIRS_NOT_PD, dpgo_amd.PAIRS_SKIPPED) == (0, 1, 2)
    # eight ints, a long long, nine doubles
    assert C.sizeof(dpgo_amd.PairsResult) == 32 + 8 + 72
    L = dpgo_amd.lib()
    header = open(os.path.join(os.path.dirname(dpgo_amd.__file__), "..", "include", "dpgo_amd.h")).read()
    for sym in ("dpgo_group_pair_covariance", "dpgo_graph_pair_covariance_reweighted", "dpgo_debug_pairs_plan", "dpgo_debug_pairs_gate",
                "dpgo_debug_pairs_vsolve_baseline"):
        assert sym + "(" in header and sym in dpgo_amd.SYMBOLS and hasattr(L, sym)
    for name in ("DPGO_PAIRS_OK 0", "DPGO_PAIRS_NOT_PD 1", "DPGO_PAIRS_SKIPPED 2"):
        assert "#define " + name in header
    X = np.zeros((8, 3), order="F")
    dp = X.ctypes.data_as(C.POINTER(C.c_double))
    pairs = np.zeros(2, np.int32)
    ip = pairs.ctypes.data_as(C.POINTER(C.c_int))
    r = dpgo_amd.PairsResult()
    fake = C.c_void_p(0)
    assert L.dpgo_group_pair_covariance(None, dp, 8, 0, 0, ip, 1, None, dp, dp, None, C.byref(r)) == -1
    assert L.dpgo_group_pair_covariance(fake, dp, 8, 0, 0, ip, 1, None, dp, dp, None, C.byref(r)) == -1
    assert L.dpgo_graph_pair_covariance_reweighted(None, 0, dp, 8, 0, 0.25, 0, 0, ip, 1, None, dp, dp, None, C.byref(r), None) == -1
    sizes = np.zeros(4, np.int32)
    sp_ = sizes.ctypes.data_as(C.POINTER(C.c_int))
    assert L.dpgo_debug_pairs_plan(0, 0, ip, 1, ip, ip, sp_) == -1 and L.dpgo_debug_pairs_plan(6, 0, None, 1, ip, ip, sp_) == -1
    assert L.dpgo_debug_pairs_plan(6, 0, ip, -1, ip, ip, sp_) == -1 and L.dpgo_debug_pairs_plan(6, 0, ip, 1, ip, ip, None) == -1
