"""Host side of the joint marginals of a pose set (dpgo_amd/csrc/marg.h): the restatement (tests/marg_restatement.py) held to its
identities in long double, the bounds against the plain fp64 evaluation and against six mistakes a kernel could make, the
column plan and the relative form's arithmetic through their debug hooks, and the C ABI.  No GPU.

The points are those of tests/test_pairs_host.py; bS here is the factorisation's part of the blocks' bound alone
(C u kappa_2 |A^-1|_2), as there.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_restatement as cr  # noqa: E402
import factor_restatement as fr  # noqa: E402
import marg_restatement as mr  # noqa: E402
import pairs_restatement as pr  # noqa: E402
import test_pairs_host as tph  # noqa: E402  (its points and records; none of its tests is imported)

import dpgo_amd  # noqa: E402

LD, U = mr.LD, mr.U
FIXTURES = ["tinyGrid3D", "smallGrid3D", "ladder2"]
_ref = {}


def reference(fixtures_dir, name, anchor):
    """(d, N, X, A, its long-double Cholesky factor, numpy's fp64 inverse made symmetric, bS) of a fixture under an anchor, once."""
    key = (name, anchor)
    if key not in _ref:
        d, N, X, H = tph.fixture(fixtures_dir, name)
        A = cr.anchored(H, anchor, cr.dof_of(d))
        A = (A + A.T) / 2
        lam = np.linalg.eigvalsh(A)
        assert lam[0] > 0
        L, kstar, _ = fr.cholesky_ld(A)
        assert kstar < 0
        S64 = np.linalg.inv(A)
        S64 = np.tril(S64) + np.tril(S64, -1).T   # (the lower entries mirrored, as the gather hands them out)
        _ref[key] = (d, N, X, A, L, S64, cr.C * U * float(lam[-1] / lam[0]) / float(lam[0]))
    return _ref[key]


def seeded_keep(N, anchor, seed, count, with_anchor=False):
    """`count` distinct seeded poses in seeded (unsorted) order, without the anchor unless it is asked for (then it is second)."""
    rng = np.random.default_rng(seed)
    pool = [g for g in range(N) if g != anchor]
    keep = [int(g) for g in rng.permutation(pool)[:count - (1 if with_anchor else 0)]]
    if with_anchor:
        keep.insert(1, anchor)
    assert keep != sorted(keep) or count < 3
    return keep


def worst(got, want, bound):
    return float(np.max(np.abs(np.asarray(got, LD) - want) / (bound + 1e-300)))


# ---------------------------------------------------------------------------------------------------------------
# the identities of the restatement, in long double
# ---------------------------------------------------------------------------------------------------------------
def test_schur_complement_is_the_inverse_of_the_kept_block(fixtures_dir):
    for name in ("tinyGrid3D", "ladder2"):
        d, N, X, A, L, _, _ = reference(fixtures_dir, name, 0)
        dof = cr.dof_of(d)
        keep = seeded_keep(N, 0, 3, min(5, N - 1))
        S = mr.sigma_kk(A, dof, keep, 0, L)
        P = mr.schur(A, dof, keep) @ S
        assert np.abs(P - np.eye(len(P))).max() <= 1e-13, name
        info, logdet, _ = mr.inverse_ld(S)
        assert np.abs(info - mr.schur(A, dof, keep)).max() <= 1e-12 * np.abs(info).max()
        assert abs(logdet - np.linalg.slogdet(np.asarray(S, np.float64))[1]) <= 1e-9 * max(1, abs(logdet))


def test_every_other_pose_kept_gives_the_matrix_itself_and_one_pose_its_marginal(fixtures_dir):
    d, N, X, A, L, S64, _ = reference(fixtures_dir, "tinyGrid3D", 0)
    dof = cr.dof_of(d)
    keep = seeded_keep(N, 0, 4, N - 1)
    idx = mr.unknowns(dof, keep)
    info = mr.inverse_ld(mr.sigma_kk(A, dof, keep, 0, L))[0]
    assert np.abs(info - A[np.ix_(idx, idx)]).max() <= 1e-12 * np.abs(A).max()
    assert np.abs(mr.schur(A, dof, keep) - A[np.ix_(idx, idx)]).max() == 0   # (M is the anchor's identity block: nothing to take off)
    one = mr.sigma_kk(A, dof, [5], 0, L)
    assert np.abs(one - S64[dof * 5:dof * 5 + dof, dof * 5:dof * 5 + dof]).max() <= 1e-12


@pytest.mark.parametrize("name", FIXTURES)
def test_relative_form_of_two_poses_is_the_pair_restatement_and_anchors_agree(fixtures_dir, name):
    """K = 2 against pairs_restatement.rel_cov; and the relative covariance of a set under anchors 0 and N - 1: at a critical
    point the two agree to first order.  The difference the restatement itself shows at these points is printed: it is no
    rounding but the points' distance from criticality, and a test on the device has to allow for it."""
    d, N, X = reference(fixtures_dir, name, 0)[:3]
    dof = cr.dof_of(d)
    keep = seeded_keep(N, 0, 8, 4, with_anchor=True)
    rel = {}
    for a in (0, N - 1):
        _, _, _, A, L, _, _ = reference(fixtures_dir, name, a)
        S = mr.sigma_kk(A, dof, keep, a, L)
        rel[a] = mr.rel_cov(mr.jacobian_set(X, d, keep, keep[0], LD), S)
        p, q = keep[2], keep[3]
        two = mr.rel_cov(mr.jacobian_set(X, d, [p, q], p, LD), mr.sigma_kk(A, dof, [p, q], a, L))
        full = np.zeros((A.shape[0], A.shape[0]), LD)
        cols = mr.unknowns(dof, [p, q])
        full[:, cols] = mr.columns_ld(A, dof, [p, q], L)
        assert np.abs(two - pr.rel_cov(pr.jacobian(X, d, p, q, LD), pr.joint_of(full, dof, p, q, a))).max() == 0
    diff = float(np.abs(rel[0] - rel[N - 1]).max())
    print("%s: relative covariance under anchors 0 and %d differs by %.3g (largest entry %.3g)" % (name, N - 1, diff, float(np.abs(rel[0]).max())))
    # these points are the solver's iterates, not polished ones (ladder2: 300 iterations of the oracle, 1.3e-3 of the largest
    # entry; the grids below 1e-6): the figure is recorded, and held only to "the same quantity to two digits"
    assert diff <= 1e-2 * float(np.abs(rel[0]).max())


# ---------------------------------------------------------------------------------------------------------------
# the bounds: the fp64 evaluation inside, six mutants outside
# ---------------------------------------------------------------------------------------------------------------
def cases(N):
    """(anchor, keep, base): the absolute form, the relative form with the base first, with the base last and the anchor kept,
    and with the anchor as the base."""
    return [(0, seeded_keep(N, 0, 11, min(6, N - 1)), None), (0, seeded_keep(N, 0, 12, min(5, N - 1)), "first"),
            (N - 1, seeded_keep(N, N - 1, 13, min(5, N - 1), with_anchor=True), "last"),
            (0, seeded_keep(N, 0, 14, min(4, N - 1), with_anchor=True), "anchor")]


def evaluate(fixtures_dir, name, anchor, keep, base, mutant=None, hook=False):
    """(worst error / bound of cov, of info, of logdet; rho) of the fp64 evaluation against the long-double restatement."""
    d, N, X, A, L, S64, bS = reference(fixtures_dir, name, anchor)
    dof = cr.dof_of(d)
    S_ld = mr.sigma_kk(A, dof, keep, anchor, L)
    S_64 = mr.sigma_from_dense(S64, dof, keep, anchor)
    if base is None:
        cov_ld, bound = S_ld, np.full(S_ld.shape, bS)
        cov = mr.absolute_fp64(S64, dof, keep, anchor, mutant)
    else:
        cov_ld = mr.rel_cov(mr.jacobian_set(X, d, keep, base, LD), S_ld)
        bound = mr.margin_rel(X, d, keep, base, anchor, S_64, bS)
        if hook:
            rec = np.stack([tph.record_of(X, d, g) for g in keep])
            cov = dpgo_amd.marg_rel_debug(d, rec, S_64, keep.index(base))
        else:
            cov = mr.relative_fp64(X, d, keep, base, S_64, mutant)
    rho = mr.rho_of(cov_ld, bound)
    info_ld, logdet_ld, sal = mr.inverse_ld(cov_ld)
    if not np.array_equal(cov, cov.T) or np.linalg.eigvalsh(cov)[0] <= 0:
        return worst(cov, cov_ld, bound), np.inf, np.inf, rho
    info = np.linalg.inv(cov)
    logdet = np.linalg.slogdet(cov)[1]
    return (worst(cov, cov_ld, bound), worst(info, info_ld, mr.info_bound(cov_ld, bound)),
            float(abs(LD(logdet) - logdet_ld) / mr.logdet_bound(cov_ld, bound, sal)), rho)


def base_of(keep, base, anchor):
    return None if base is None else keep[0] if base == "first" else keep[-1] if base == "last" else anchor


@pytest.mark.parametrize("name", FIXTURES)
def test_fp64_evaluation_and_host_twin_lie_inside_the_bounds(fixtures_dir, name):
    N = reference(fixtures_dir, name, 0)[1]
    for anchor, keep, base in cases(N):
        b = base_of(keep, base, anchor)
        for hook in ((False,) if b is None else (False, True)):
            w = evaluate(fixtures_dir, name, anchor, keep, b, hook=hook)
            print("%s anchor %d keep %s base %s%s: cov %.3g, info %.3g, logdet %.3g of their bounds; rho %.3g"
                  % (name, anchor, keep, b, " (host twin)" if hook else "", w[0], w[1], w[2], w[3]))
            assert w[3] <= 0.1, "the kept set does not satisfy the condition rho <= 0.1"
            assert max(w[:3]) < 1.0, w


@pytest.mark.parametrize("mutant", mr.MUTANTS)
def test_each_mutant_is_flagged_by_a_bound(fixtures_dir, mutant):
    for name in ("smallGrid3D", "ladder2"):
        N = reference(fixtures_dir, name, 0)[1]
        anchor, keep, base = cases(N)[0 if mutant == "ascending_order" else 1]
        b = base_of(keep, base, anchor)
        assert max(evaluate(fixtures_dir, name, anchor, keep, b)[:3]) < 1.0
        w = evaluate(fixtures_dir, name, anchor, keep, b, mutant=mutant)
        assert w[0] > 1.0, (name, mutant, w)


# ---------------------------------------------------------------------------------------------------------------
# the column plan and the hooks
# ---------------------------------------------------------------------------------------------------------------
def python_plan(dof, anchor, keep):
    col, poses = [], []
    for g in keep:
        col.append(-1 if g == anchor else dof * len(poses))
        if g != anchor:
            poses.append(g)
    columns = dof * len(poses)
    return poses, col, columns, (columns + 63) // 64, 16 * ((min(max(columns, 1), 64) + 15) // 16)


def test_column_plan_against_the_python_plan():
    sets = [(6, 0, [9, 2, 7]), (6, 4, [9, 4, 2]), (6, 0, list(range(21, 0, -2))), (6, 5, list(range(22, 0, -1))),
            (6, 0, list(range(1, 23))), (3, 1, [1]), (3, 0, [8, 3, 5, 0, 2]), (3, 7, list(range(30, 0, -1)))]
    for dof, anchor, keep in sets:
        pl = dpgo_amd.marg_plan_debug(dof, anchor, keep)
        poses, col, columns, batches, kb = python_plan(dof, anchor, keep)
        assert pl["poses"].tolist() == poses and pl["col"].tolist() == col, keep
        assert (pl["columns"], pl["batches"], pl["kb"]) == (columns, batches, kb)
    # dof = 6: the eleventh pose of a list straddles the batches (columns 60 ... 65); 22 poses need three
    pl = dpgo_amd.marg_plan_debug(6, 0, list(range(21, 0, -2)))
    assert pl["col"][10] == 60 and pl["columns"] == 66 and pl["batches"] == 2 and pl["kb"] == 64
    assert dpgo_amd.marg_plan_debug(6, 0, list(range(1, 23)))["batches"] == 3
    # the plan's sizes are pairs_plan's for the same poses
    pp = dpgo_amd.pairs_plan_debug(6, 0, [[i, i + 1] for i in range(1, 22)])
    assert (pp["columns"], pp["batches"], pp["kb"]) == (132, 3, 64)


def test_relative_hook_for_two_poses_is_the_pair_hook(fixtures_dir):
    for name in ("tinyGrid3D", "ladder2"):
        d, N, X, A, L, S64, bS = reference(fixtures_dir, name, 0)
        dof = cr.dof_of(d)
        p, q = 3, 6
        S = mr.sigma_from_dense(S64, dof, [p, q], 0)
        rec = np.stack([tph.record_of(X, d, g) for g in (p, q)])
        rel = dpgo_amd.pairs_gate_debug(d, rec[0], rec[1], pr.blocks_of(S, dof))[0]
        got = dpgo_amd.marg_rel_debug(d, rec, S, 0)
        m = mr.margin_rel(X, d, [p, q], p, 0, S, bS)
        assert np.all(np.abs(got - rel) <= 2 * m) and np.array_equal(got, got.T)
        # the base last: the other pose's view
        back = dpgo_amd.marg_rel_debug(d, rec, S, 1)
        rel_qp = dpgo_amd.pairs_gate_debug(d, rec[1], rec[0], pr.blocks_of(S[np.ix_(np.r_[dof:2 * dof, :dof], np.r_[dof:2 * dof, :dof])], dof))[0]
        assert np.all(np.abs(back - rel_qp) <= 2 * mr.margin_rel(X, d, [p, q], q, 0, S, bS))
    with pytest.raises(ValueError):
        dpgo_amd.marg_rel_debug(3, np.zeros((1, 12)), np.zeros((6, 6)), 0)
    with pytest.raises(ValueError):
        dpgo_amd.marg_rel_debug(3, np.zeros((2, 12)), np.zeros((12, 12)), 2)


def test_marg_abi():
    assert (dpgo_amd.MARG_OK, dpgo_amd.MARG_NOT_PD, dpgo_amd.MARG_SKIPPED) == (0, 1, 2)
    # ten ints, a long long, nine doubles
    assert C.sizeof(dpgo_amd.MargResult) == 40 + 8 + 72
    L = dpgo_amd.lib()
    header = open(os.path.join(os.path.dirname(dpgo_amd.__file__), "..", "include", "dpgo_amd.h")).read()
    for sym in ("dpgo_group_joint_marginal", "dpgo_graph_joint_marginal_reweighted", "dpgo_debug_marg_plan", "dpgo_debug_marg_rel_host",
                "dpgo_debug_marg_rel", "dpgo_debug_marg_dense"):
        assert sym + "(" in header and sym in dpgo_amd.SYMBOLS and hasattr(L, sym)
    for name in ("DPGO_MARG_OK 0", "DPGO_MARG_NOT_PD 1", "DPGO_MARG_SKIPPED 2"):
        assert "#define " + name in header
    X = np.zeros((8, 3), order="F")
    dp = X.ctypes.data_as(C.POINTER(C.c_double))
    keep = np.ones(2, np.int32)
    ip = keep.ctypes.data_as(C.POINTER(C.c_int))
    r = dpgo_amd.MargResult()
    assert L.dpgo_group_joint_marginal(None, dp, 8, ip, 1, 0, -1, 1, 0, dp, dp, dp, C.byref(r)) == -1
    assert L.dpgo_group_joint_marginal(C.c_void_p(0), dp, 8, ip, 1, 0, -1, 1, 0, dp, dp, dp, C.byref(r)) == -1
    assert L.dpgo_graph_joint_marginal_reweighted(None, 0, dp, 8, 0, 0.25, ip, 1, 0, -1, 1, 0, dp, dp, dp, C.byref(r), None) == -1
    sizes = np.zeros(4, np.int32)
    sp_ = sizes.ctypes.data_as(C.POINTER(C.c_int))
    assert L.dpgo_debug_marg_plan(0, 0, ip, 1, ip, ip, sp_) == -1 and L.dpgo_debug_marg_plan(6, 0, None, 1, ip, ip, sp_) == -1
    assert L.dpgo_debug_marg_plan(6, 0, ip, 0, ip, ip, sp_) == -1
    assert L.dpgo_debug_marg_rel_host(4, 2, 0, dp, dp, dp) == -1 and L.dpgo_debug_marg_rel_host(3, 1, 0, dp, dp, dp) == -1
    assert L.dpgo_debug_marg_rel_host(3, 2, 2, dp, dp, dp) == -1 and L.dpgo_debug_marg_rel_host(3, 2, 0, None, dp, dp) == -1
    assert L.dpgo_debug_marg_dense(0, 0, dp, dp, dp, dp, C.byref(r)) == -1 and L.dpgo_debug_marg_dense(0, 4, None, dp, dp, dp, C.byref(r)) == -1
    with pytest.raises(ValueError):
        dpgo_amd.marg_dense_debug(np.zeros((3, 4)))
