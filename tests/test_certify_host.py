"""Host side of the solution certificate (dpgo_amd/csrc/cert.cpp): the Rayleigh-Ritz step against scipy, the numpy
restatement (tests/cert_restatement.py) against the definition and against dense eigvalsh, and the argument checks of
the C ABI.  No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import scipy.linalg as sla

import dpgo_amd
from oracle import g2o as og
from oracle.hash import Options as OOptions
from oracle.problem import LOSS_NONE
from oracle.star import DistPGO as ODistPGO, GlobalProblem, chordal_initialization

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cert_restatement as cr  # noqa: E402


# ---------------------------------------------------------------------------------------------------------------
# Rayleigh-Ritz
# ---------------------------------------------------------------------------------------------------------------
def _pair(rng, n, cond):
    A = rng.standard_normal((n, n))
    A = 0.5 * (A + A.T)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    B = (Q * np.logspace(0, -np.log10(cond), n)) @ Q.T
    return A, 0.5 * (B + B.T)


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("nblk", [2, 3])
@pytest.mark.parametrize("cond", [1.0, 1e2, 1e4])
def test_rayleigh_ritz_against_scipy(d, nblk, cond):
    rng = np.random.default_rng(100 * d + 10 * nblk + int(np.log10(cond)))
    for _ in range(20):
        A, B = _pair(rng, d * nblk, cond)
        theta, Cm, used = dpgo_amd.rayleigh_ritz(A, B, nblk)
        assert used == nblk
        w = sla.eigh(A, B, eigvals_only=True)
        # forward bound of a Cholesky-reduced symmetric eigenproblem, with a factor of ~50 for the Jacobi sweeps
        tol = 1e-12 * np.linalg.norm(A, 2) * np.linalg.cond(B)
        assert np.max(np.abs(theta - w[:d])) <= tol, (theta, w[:d], tol)
        assert np.max(np.abs(Cm.T @ B @ Cm - np.eye(d))) <= tol
        assert np.max(np.abs(Cm.T @ A @ Cm - np.diag(theta))) <= tol
        # the restatement's own step is held to the same
        th2, C2, u2 = cr.rayleigh_ritz(A, B, d, nblk)
        assert u2 == nblk and np.max(np.abs(th2 - w[:d])) <= tol


@pytest.mark.parametrize("d", [2, 3])
def test_rayleigh_ritz_drops_a_dependent_last_block(d):
    rng = np.random.default_rng(7 + d)
    n = 3 * d
    # a basis whose last block nearly lies in the span of the first two: pivot ~1e-14 after scaling
    Bas = rng.standard_normal((40, n))
    Bas[:, 2 * d:] = Bas[:, :d] @ rng.standard_normal((d, d)) + 1e-7 * rng.standard_normal((40, d))
    S = rng.standard_normal((40, 40))
    S = 0.5 * (S + S.T)
    A, B = Bas.T @ S @ Bas, Bas.T @ Bas
    theta, Cm, used = dpgo_amd.rayleigh_ritz(A, B, 3)
    assert used == 2
    assert np.all(Cm[2 * d:] == 0.0)
    m = 2 * d
    w = sla.eigh(A[:m, :m], B[:m, :m], eigvals_only=True)
    tol = 1e-12 * np.linalg.norm(A[:m, :m], 2) * np.linalg.cond(B[:m, :m])
    assert np.max(np.abs(theta - w[:d])) <= tol
    assert np.max(np.abs(Cm[:m].T @ B[:m, :m] @ Cm[:m] - np.eye(d))) <= tol
    assert cr.rayleigh_ritz(A, B, d, 3)[2] == 2


def test_rayleigh_ritz_rejects_a_singular_first_block():
    A, B = np.eye(4), np.zeros((4, 4))
    with pytest.raises(RuntimeError):
        dpgo_amd.rayleigh_ritz(A, B, 2)


# ---------------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------------
def test_cert_options_default_and_null_arguments():
    o = dpgo_amd.CertOptions()
    assert (o.eta, o.tau, o.max_iters, o.precondition, o.stop_on_negative, o.refresh_every, o.seed) == (1e-3, 1e-6, 2000, 1, 1, 50, 0)
    L = dpgo_amd.lib()
    X = np.zeros((8, 3), order="F")
    res = dpgo_amd.CertResult()
    dp = X.ctypes.data_as(C.POINTER(C.c_double))
    assert L.dpgo_group_certify(None, dp, 8, C.byref(o), None, 0, C.byref(res), None, 0) == -1
    fake = C.c_void_p(0)
    assert L.dpgo_group_certify(fake, dp, 8, None, None, 0, C.byref(res), None, 0) == -1
    assert L.dpgo_group_certify(fake, dp, 8, C.byref(o), None, 0, None, None, 0) == -1
    assert L.dpgo_group_cert_lambda(None, dp, 8, dp) == -1
    assert L.dpgo_group_cert_apply(None, dp, 8, dp, 8, dp, 8) == -1
    L.dpgo_cert_options_default(None)   # (no crash)
    assert (dpgo_amd.CERT_UNDECIDED, dpgo_amd.CERT_NONNEGATIVE, dpgo_amd.CERT_NEGATIVE) == (cr.UNDECIDED, cr.NONNEGATIVE, cr.NEGATIVE)


# ---------------------------------------------------------------------------------------------------------------
# the restatement against the definition
# ---------------------------------------------------------------------------------------------------------------
ITERS = {"tinyGrid3D": 100, "smallGrid3D": 200}
_points = {}


def points(fixtures_dir, name):
    """(GlobalProblem, chordal point, converged point) of a fixture on 2 nodes: AMM-PGO#, driver options, LOSS_NONE."""
    if name not in _points:
        path = os.path.join(fixtures_dir, name + ".g2o")
        num_poses, mm = og.read_g2o_file(path)
        opt = OOptions.driver(LOSS_NONE, True)
        X0 = chordal_initialization(num_poses, mm)
        drv = ODistPGO(path, 2, opt, X0=X0, mm=mm, num_poses=num_poses)
        drv.run(ITERS[name], evaluate=False)
        _points[name] = (GlobalProblem(num_poses, mm, 2, opt), X0, drv.gather())
    return _points[name]


@pytest.mark.parametrize("name", ["tinyGrid3D", "smallGrid3D"])
@pytest.mark.parametrize("which", ["chordal", "converged"])
def test_restatement_is_the_definition(fixtures_dir, name, which):
    """S symmetric, its blocks M's minus Lambda_p, apply() = S V, and |S X|_F = |grad F| to 1e-10 relative.

    The last holds at the converged points too (|grad F| = 2.2e-4 and 1.1e-6, where 1e-10 relative is 1e-16 absolute) because
    apply() forms Lambda and Lambda V with the batched products SOdProduct::SymBlockDiagProduct is restated with in
    oracle/problem.py: S X = M X - sym((M X)_Y Y^T) Y is then the oracle's tangent projection operation for operation, and the
    two norms are the same bits.  (An einsum for the same two products sums in another order and differs by 4.7e-16 at the
    converged smallGrid3D point, 4.3e-10 of the gradient.)"""
    gp, X0, Xc = points(fixtures_dir, name)
    X = X0 if which == "chordal" else Xc
    d, N = gp.d, gp.num_poses
    S = cr.S_matrix(gp.M, X, d)
    Sd = S.toarray()
    assert np.max(np.abs(Sd - Sd.T)) <= 1e-13 * np.max(np.abs(Sd))
    # the translation rows and columns are M's; the rotation blocks differ by Lambda_p
    Lam = cr.lambda_blocks(gp.M, X, d)
    Md = gp.M.toarray()
    for p in (0, N // 2, N - 1):
        r = slice(N + d * p, N + d * p + d)
        np.testing.assert_allclose(Md[r, r] - Sd[r, r], Lam[p], atol=1e-12 * np.max(np.abs(Md)))
    V = np.random.default_rng(3).standard_normal(X.shape)
    np.testing.assert_allclose(cr.apply(gp.M, X, V, d), Sd @ V, atol=1e-12 * np.linalg.norm(Sd, 2) * np.max(np.abs(V)))
    # |S X|_F is the norm of the Riemannian gradient (S X evaluated as M X - Lambda X, the way evaluate_grad projects)
    g = np.linalg.norm(gp.evaluate_grad(X))
    sx = np.linalg.norm(cr.apply(gp.M, X, X, d))
    print(name, which, "|grad F| = %.6e, | |S X| - |grad F| | / |grad F| = %.3e" % (g, abs(sx - g) / g))
    assert abs(sx - g) <= 1e-10 * g


@pytest.mark.parametrize("name", ["tinyGrid3D", "smallGrid3D"])
@pytest.mark.parametrize("which", ["chordal", "converged"])
@pytest.mark.parametrize("precondition", [True, False])
def test_restatement_lobpcg_finds_the_smallest_eigenvalue(fixtures_dir, name, which, precondition):
    gp, X0, Xc = points(fixtures_dir, name)
    X = X0 if which == "chordal" else Xc
    d = gp.d
    lam = np.linalg.eigvalsh(cr.S_matrix(gp.M, X, d).toarray())
    nS = max(abs(lam[0]), abs(lam[-1]))
    clustered = name == "smallGrid3D" and which == "converged"
    for seed in range(3):
        V0 = np.random.default_rng(seed).standard_normal(X.shape)
        r = cr.lobpcg(gp.M, X, d, V0, tau=1e-9, max_iters=3000, precondition=precondition, stop_on_negative=False, seed=seed)
        print(name, which, precondition, seed, r["iterations"], r["theta"] - lam[0], r["residual"])
        assert r["status"] != cr.UNDECIDED
        th, res = r["theta"], r["residual"]
        assert lam[0] - 1e-10 * nS <= th
        if clustered:   # d + 1 gauge directions within 3.6e-9 of zero, then a gap
            assert r["status"] == cr.NONNEGATIVE
            assert th < lam[4] and th <= lam[3] + res ** 2 / (lam[4] - th) + 1e-10 * nS
        else:           # Kato-Temple
            assert th < lam[1] and th - lam[0] <= res ** 2 / (lam[1] - th) + 1e-10 * nS
            assert r["status"] == cr.NEGATIVE


def test_restatement_decisions_on_the_small_fixtures(fixtures_dir):
    """Default options: the converged tinyGrid3D point is NOT certified, the converged smallGrid3D point is."""
    gp, _, Xc = points(fixtures_dir, "tinyGrid3D")
    V0 = np.random.default_rng(0).standard_normal(Xc.shape)
    r = cr.lobpcg(gp.M, Xc, gp.d, V0)
    assert r["status"] == cr.NEGATIVE and r["theta"] < -0.5e-3
    gp, _, Xc = points(fixtures_dir, "smallGrid3D")
    V0 = np.random.default_rng(0).standard_normal(Xc.shape)
    r = cr.lobpcg(gp.M, Xc, gp.d, V0)
    assert r["status"] == cr.NONNEGATIVE, r
