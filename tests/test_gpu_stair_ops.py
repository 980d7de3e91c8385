"""The staircase's operators on the device (dpgo_amd/csrc/stair.hip through the hooks NodeGroup.stair_eval / stair_hess /
stair_retract / stair_round) against the numpy restatement (tests/staircase_restatement.py) on the oracle's data matrix, at
seeded random feasible lifted points of rank d, d + 1 and 2d.

Entrywise bounds derived from the operation (u = 2^-53), in the terms tests/test_gpu_certify.py derives for the certificate:
  M V is S V + G V of the node's assembled operators: 2 k_i u ((|G| + |S|) |V|)_i per entry (tc.prod_bound);
  Lambda_p = sym((M X)_p.Y Y_p^T) over 2d columns: the product's bound carried through, plus 2 (2d + 1) u |(M X)_p.Y| |Y_p|^T;
  S V = M V - Lambda V.Y: the product's bound, |dLambda| |V.Y|, 2 d u |Lambda| |V.Y|, and 2 u |S V| for the difference;
  Proj_X(W) = W - sym(W.Y Y^T) Y: the bound b of W, sym(b |Y|^T) |Y| for what it moves in the symmetric part,
  2 (2d + 1) u sym(|W.Y| |Y|^T) |Y| for forming that part, 2 d u |sym| |Y| for its product, 2 u |result| for the difference;
  F = 1/2 <X, M X>: 1/2 <|X|, b(M X)> plus n u 1/2 <|X|, |M X|> for a sum of n = 2d (d+1) N terms in any order;
  |grad|: the norm of the gradient's bound, plus n u |grad|.
The retraction is held to what it has to be: Z_p.Y Z_p.Y^T = I within 64 u, the polar factor of Y + V (the restatement's, from
the SVD) within 64 u cond(A) where A = Y_p + V_p.Y -- an SVD and an eigen-decomposition of A A^T agree to that -- and
retract(Y, 0) = Y within 8 u.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import staircase_restatement as st  # noqa: E402
import test_gpu_certify as tc  # noqa: E402  (its inputs, caches and derived bounds; none of its tests is imported)
import test_gpu_cert_proof as tp  # noqa: E402  (likewise: the d = 2 graph)

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
CASES = [("tinyGrid3D", 1), ("smallGrid3D", 1), ("smallGrid3D", 2), ("smallGrid3D", 5), ("ladder2", 6)]
_groups, _pts = {}, {}


def setup(fixtures_dir, name, nn):
    """(group, N, d, M, Aabs, k) once per (input, nodes)."""
    key = (name, nn)
    if key not in _groups:
        N, mm, gp, X0, make = tp.instance(fixtures_dir, name)
        grp, opt = make(nn)
        Aabs, k = tc.abs_operator(N, mm, nn, opt.regularizer)
        _groups[key] = (grp, N, mm.d, gp.M, Aabs, k)
    return _groups[key]


def points(name, N, d):
    """Per rank: a feasible lifted point and two directions, one tangent and of unit size, one Gaussian."""
    if name not in _pts:
        rng = np.random.default_rng(311)
        out = {}
        for r in (d, d + 1, 2 * d):
            Y = st.random_lifted_point(rng, N, d, r)
            V = np.zeros_like(Y)
            V[:, :r] = rng.standard_normal((Y.shape[0], r))
            T = st.proj(Y, V, d)
            out[r] = (Y, np.asfortranarray(V), np.asfortranarray(T / np.linalg.norm(T)))
        _pts[name] = out
    return _pts[name]


def rot_abs(X, d):
    return np.abs(st.rot(X, d))


def lambda_bound(Aabs, k, M, X, d):
    bX = st.rot(tc.prod_bound(Aabs, k, X), d)
    E = np.einsum("prc,psc->prs", bX + 2 * (2 * d + 1) * U * rot_abs(M @ X, d), rot_abs(X, d))
    return st.sym(E)


def apply_bound(Aabs, k, M, X, V, d):
    N = X.shape[0] // (d + 1)
    Lam = np.abs(st.lambda_blocks(M, X, d))
    b = tc.prod_bound(Aabs, k, V)
    b[N:] += ((2 * d * U * Lam + lambda_bound(Aabs, k, M, X, d)) @ rot_abs(V, d)).reshape(N * d, V.shape[1])
    return b + 2 * U * np.abs(st.apply_S(M, X, V, d))


def proj_bound(X, W, b, d):
    N = X.shape[0] // (d + 1)
    Ya = rot_abs(X, d)
    sym_abs = st.sym(rot_abs(W, d) @ Ya.transpose(0, 2, 1))
    E = st.sym(st.rot(b, d) @ Ya.transpose(0, 2, 1)) + 2 * (2 * d + 1) * U * sym_abs
    out = np.array(b)
    out[N:] += ((E + 2 * d * U * sym_abs) @ Ya).reshape(N * d, X.shape[1])
    return out + 2 * U * np.abs(st.proj(X, W, d))


@pytest.mark.parametrize("name,nn", CASES)
def test_eval_against_the_restatement(fixtures_dir, name, nn):
    grp, N, d, M, Aabs, k = setup(fixtures_dir, name, nn)
    for r, (Y, V, T) in points(name, N, d).items():
        F, gn, Lam, G = grp.stair_eval(Y)
        n = Y.size
        MY = M @ Y
        bMY = tc.prod_bound(Aabs, k, Y)
        bF = 0.5 * float(np.sum(np.abs(Y) * bMY)) + n * U * 0.5 * float(np.sum(np.abs(Y) * np.abs(MY)))
        Fref = st.objective(M, Y)
        bL = lambda_bound(Aabs, k, M, Y, d)
        Lref = st.lambda_blocks(M, Y, d)
        Gref = st.grad(M, Y, d)
        bG = apply_bound(Aabs, k, M, Y, Y, d)
        print("%s x %d rank %d: F %.3g of its bound, Lambda %.3g, grad %.3g" %
              (name, nn, r, abs(F - Fref) / bF, np.max(np.abs(Lam - Lref) / bL), np.max(np.abs(G - Gref)[:, :r] / bG[:, :r])))
        assert abs(F - Fref) <= bF
        assert np.all(np.abs(Lam - Lref) <= bL) and np.array_equal(Lam, Lam.transpose(0, 2, 1))
        assert np.all(np.abs(G - Gref) <= bG)
        assert abs(gn - np.linalg.norm(Gref)) <= np.linalg.norm(bG) + n * U * np.linalg.norm(Gref)
        assert not G[:, r:].any()                              # the zero columns stay exactly zero
        again = grp.stair_eval(Y)
        assert (again[0], again[1]) == (F, gn) and np.array_equal(again[2], Lam) and np.array_equal(again[3], G)


@pytest.mark.parametrize("name,nn", CASES)
def test_hess_against_the_restatement(fixtures_dir, name, nn):
    grp, N, d, M, Aabs, k = setup(fixtures_dir, name, nn)
    for r, (Y, V, T) in points(name, N, d).items():
        for what, D in (("gaussian", V), ("tangent", T)):
            out = grp.stair_hess(Y, D)
            W = st.apply_S(M, Y, D, d)
            ref = st.proj(Y, W, d)
            b = proj_bound(Y, W, apply_bound(Aabs, k, M, Y, D, d), d)
            print("%s x %d rank %d %s: %.3g of the bound" % (name, nn, r, what, np.max(np.abs(out - ref)[:, :r] / b[:, :r])))
            assert np.all(np.abs(out - ref) <= b)
            assert not out[:, r:].any()
            assert np.array_equal(grp.stair_hess(Y, D), out)


def orthonormality(Z, d):
    Y = st.rot(Z, d)
    return float(np.abs(Y @ Y.transpose(0, 2, 1) - np.eye(d)).max())


@pytest.mark.parametrize("name,nn", CASES)
def test_retract(fixtures_dir, name, nn):
    grp, N, d, M, Aabs, k = setup(fixtures_dir, name, nn)
    for r, (Y, V, T) in points(name, N, d).items():
        assert np.abs(grp.stair_retract(Y, 0 * Y) - Y).max() <= 8 * U
        big = np.array(T)
        nrm = np.sqrt(np.sum(st.rot(big, d) ** 2, axis=(1, 2)))           # |V_p| = 10 for every pose
        big[N:] = (st.rot(big, d) * (10.0 / nrm)[:, None, None]).reshape(N * d, 2 * d)
        for what, D in (("unit", T), ("gaussian", V), ("large", np.asfortranarray(big))):
            Z = grp.stair_retract(Y, D)
            ref = st.retract(Y, D, d)
            cond = float(np.linalg.cond(st.rot(Y + D, d)[:, :, :r]).max())
            err = float(np.abs(Z - ref).max())
            print("%s x %d rank %d %s: orthonormal to %.3g u, polar factor to %.3g u (cond %.3g)" %
                  (name, nn, r, what, orthonormality(Z, d) / U, err / U, cond))
            assert orthonormality(Z, d) <= 64 * U
            assert err <= 64 * U * cond
            assert np.array_equal(Z[:N], (Y + D)[:N]) and not Z[:, r:].any()
            assert np.array_equal(grp.stair_retract(Y, D), Z)


def proper(X, d):
    """X with the last row of every Y_p negated where det Y_p < 0 (the QR factors of random_lifted_point are in O(d))."""
    N = X.shape[0] // (d + 1)
    X = np.array(X)
    Y = st.rot(X, d).copy()
    Y[np.linalg.det(Y) < 0, -1, :] *= -1.0
    X[N:] = Y.reshape(N * d, d)
    return X


@pytest.mark.parametrize("name,nn", CASES)
def test_round(fixtures_dir, name, nn):
    """[X | 0] for a rank-d X comes back as X Q with one orthogonal Q and every det = +1; with X's last column negated (every
    det = -1) the vote flips it back; a rank-(d+1) point comes back as the restatement's rounding."""
    grp, N, d, M, Aabs, k = setup(fixtures_dir, name, nn)
    pts = points(name, N, d)
    X = proper(pts[d][0][:, :d], d)
    s = np.ones(d)
    s[-1] = -1.0
    for what, Xin in (("proper", X), ("reflected", X * s)):
        B, sigma, Xh = grp.stair_round(st.lift(Xin, d))
        Q = B[:d]
        assert not B[d:].any() and np.abs(Q.T @ Q - np.eye(d)).max() <= 16 * U
        Yh = st.rot(Xh, d)
        print("%s x %d %s: |Xhat - X Q| %.3g, det Q %.3g" % (name, nn, what, np.abs(Xh - Xin @ Q).max(), np.linalg.det(Q)))
        assert np.abs(Xh - Xin @ Q).max() <= 64 * U * max(1.0, np.abs(Xin).max())
        assert np.all(np.linalg.det(Yh) > 0) and np.abs(Yh @ Yh.transpose(0, 2, 1) - np.eye(d)).max() <= 64 * U
        assert np.all(np.abs(sigma[:d] - np.sqrt(N)) <= 64 * U * N) and np.all(sigma[d:] <= 1e-7 * np.sqrt(N))
        again = grp.stair_round(st.lift(Xin, d))
        assert all(np.array_equal(a, b) for a, b in zip(again, (B, sigma, Xh)))
    # a rank-(d+1) point: B spans the leading eigenspace of the Gram matrix (held by its residual, which does not depend on the
    # gaps between the eigenvalues), signed as stated; Xhat is Y B with every block on SO(d): the nearest rotation moves by
    # the perturbation over the sum of the two smallest singular values (the smallest one negated where det < 0)
    Y = pts[d + 1][0]
    B, sigma, Xh = grp.stair_round(Y)
    R = Y[N:]
    G = R.T @ R
    sref = np.sqrt(np.maximum(np.sort(np.linalg.eigvalsh(G))[::-1], 0.0))
    assert np.abs(sigma[:d + 1] - sref[:d + 1]).max() <= 2 * d * N * U * sref[0] and np.all(sigma[d + 1:] <= 1e-7 * sref[0])
    assert np.abs(B.T @ B - np.eye(d)).max() <= 16 * U and not B[d + 1:].any()
    assert np.abs(G @ B - B * sigma[:d] ** 2).max() <= 64 * (2 * d * N * U) * sref[0] ** 2
    for j in range(d - 1):
        assert B[np.argmax(np.abs(B[:, j])), j] > 0
    W = Y @ B
    Wb = st.rot(W, d)
    Uu, sv, Vt = np.linalg.svd(Wb)
    neg = np.linalg.det(Wb) < 0
    assert 2 * int(np.sum(~neg)) >= N                       # the vote has been taken
    Uu[neg, :, -1] = -Uu[neg, :, -1]
    ref = Uu @ Vt
    denom = sv[:, -2] + np.where(neg, -1.0, 1.0) * sv[:, -1]
    err = np.abs(st.rot(Xh, d) - ref).max(axis=(1, 2))
    print("%s x %d rank %d: rotations %.3g of their tolerance, translations %.3g" %
          (name, nn, d + 1, np.max(err * denom / (64 * 2 * d * U)), np.abs(Xh[:N] - W[:N]).max()))
    assert np.all(err <= 64 * 2 * d * U / denom)
    assert np.abs(Xh[:N] - W[:N]).max() <= 2 * (2 * d) * U * np.abs(Y[:N]).max() * np.sqrt(2 * d)
    assert np.all(np.linalg.det(st.rot(Xh, d)) > 0)


def test_refusals(fixtures_dir):
    grp, N, d, M, Aabs, k = setup(fixtures_dir, "tinyGrid3D", 1)
    Y = points("tinyGrid3D", N, d)[d][0]
    with pytest.raises(ValueError):
        grp.stair_eval(Y[:, :d])
    with pytest.raises(RuntimeError):
        grp.stair_eval(Y[:-1])
    with pytest.raises(RuntimeError):
        grp.stair_hess(Y, Y[:-1])
