"""The pieces of the joint marginals on the device, on GIVEN arrays and without a graph (dpgo_amd/csrc/marg.h):
dpgo_debug_marg_dense -- the gather in batches of 64 columns, the one-front factorisation of a dense matrix, its inverse through
the selected inversion and the log-determinant -- and dpgo_debug_marg_rel, the relative form's kernel, against the long-double
restatement (tests/marg_restatement.py) and bit for bit against its host twin.

Bounds; nothing in them comes from the device.
  the inverse    C u kappa_2(A) |A^-1|_2 entrywise (tests/cov_restatement.py's C), against the long-double inverse
  logdet         marg_restatement.logdet_bound with no input error: the factorisation's own term
  relative cov   marg_restatement.margin_rel with bS = 0: the given Sigma_KK is exact, J's error and the sums remain
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_restatement as cr  # noqa: E402
import marg_restatement as mr  # noqa: E402

import dpgo_amd  # noqa: E402

pytestmark = pytest.mark.gpu

LD, U = mr.LD, mr.U


def seeded_spd(n, seed):
    """B B^T / n + I / 2 with seeded normal B: eigenvalues of order one, the condition number a few tens."""
    B = np.random.default_rng(seed).standard_normal((n, n))
    A = B @ B.T / n + 0.5 * np.eye(n)
    return np.tril(A) + np.tril(A, -1).T


# 6: one panel; 63, 66: either side of the 64-column batch and tile; 129, 132: past 128, three batches
@pytest.mark.parametrize("n", [6, 63, 66, 129, 132])
def test_dense_inverse_and_logdet(n):
    A = seeded_spd(n, 100 + n)
    out = dpgo_amd.marg_dense_debug(A)
    res = out["result"]
    assert res.outcome == dpgo_amd.MARG_OK and not res.info_not_pd and res.n == n and res.fronts == 1 and res.max_front == n
    assert res.columns == n and res.batches == (n + 63) // 64 and res.device_bytes > 8 * n * n and res.dense_pivot_min > 0
    assert np.array_equal(out["cov"], A)                       # the gather moves bits
    assert np.array_equal(out["info"], out["info"].T)          # exact symmetry
    inv_ld, logdet_ld, sal = mr.inverse_ld(A)
    kappa, nl = mr.spectrum(np.asarray(A, LD))
    w_inv = float(np.abs(np.asarray(out["info"], LD) - inv_ld).max()) / (cr.C * U * kappa * nl)
    w_ld = float(abs(LD(out["logdet"]) - logdet_ld)) / mr.logdet_bound(np.asarray(A, LD), 0.0, sal)
    print("n = %d: kappa %.3g; inverse %.3g, logdet %.3g of their bounds; pivots %.3g ... %.3g"
          % (n, kappa, w_inv, w_ld, res.dense_pivot_min, res.dense_pivot_max))
    assert w_inv < 1.0 and w_ld < 1.0
    again = dpgo_amd.marg_dense_debug(A)
    assert np.array_equal(again["info"], out["info"]) and again["logdet"] == out["logdet"]


def test_dense_lower_triangle_is_the_source():
    """An entry (i, j), i >= j, is read from column j at row i and written to both places: a matrix whose upper triangle is
    garbage comes out as its lower triangle mirrored."""
    A = seeded_spd(66, 7)
    G = A + np.triu(np.full(A.shape, 3.0), 1)
    out = dpgo_amd.marg_dense_debug(G)
    assert np.array_equal(out["cov"], A)
    assert np.array_equal(out["info"], dpgo_amd.marg_dense_debug(A)["info"])


@pytest.mark.parametrize("n", [6, 66])
def test_dense_matrix_with_a_negative_pivot(n):
    A = seeded_spd(n, 9)
    lam, V = np.linalg.eigh(A)
    A = A - 2 * lam[0] * np.outer(V[:, 0], V[:, 0])   # the smallest eigenvalue becomes its negative
    A = np.tril(A) + np.tril(A, -1).T
    assert np.linalg.eigvalsh(A)[0] < 0
    out = dpgo_amd.marg_dense_debug(A)
    assert out["result"].info_not_pd == 1 and np.array_equal(out["cov"], A)
    assert not out["info"].any() and out["logdet"] == 0.0


def seeded_records(d, K, rng):
    rec = np.zeros((K, (d + 1) * d))
    for i in range(K):
        Q, R = np.linalg.qr(rng.standard_normal((d, d)))
        Q = Q * np.sign(np.diag(R))
        if np.linalg.det(Q) < 0:
            Q[:, 0] = -Q[:, 0]
        rec[i, :d] = 3 * rng.standard_normal(d)
        rec[i, d:] = Q.reshape(-1)   # Y = R^T, row-major
    return rec


def layout_of(rec, d):
    """The reference layout of the restatement (row p the translation, then the rows of Y_p) from K records."""
    K = len(rec)
    return np.concatenate([rec[:, :d], rec[:, d:].reshape(K * d, d)])


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("K,bpos,anchor_pos", [(2, 0, None), (2, 1, None), (3, 0, 0), (3, 2, 1), (12, 0, 5), (12, 11, None), (12, 4, 4)])
def test_relative_kernel_against_the_restatement_and_its_host_twin(d, K, bpos, anchor_pos):
    """K = 2, 3 and 12; the base first, last and in the middle; the anchor (zero blocks of Sigma_KK) as the base, as another
    member, absent."""
    dof = cr.dof_of(d)
    rng = np.random.default_rng(1000 * d + 10 * K + bpos)
    rec = seeded_records(d, K, rng)
    B = rng.standard_normal((dof * K, dof * K))
    S = B @ B.T / (dof * K)
    S = np.tril(S) + np.tril(S, -1).T
    keep = list(range(K))
    anchor = -1 if anchor_pos is None else anchor_pos
    S = mr.zero_anchor(S, dof, keep, anchor)
    X = layout_of(rec, d)
    got = dpgo_amd.marg_rel_debug(d, rec, S, bpos, device=0)
    want = mr.rel_cov(mr.jacobian_set(X, d, keep, bpos, LD), np.asarray(S, LD))
    m = mr.margin_rel(X, d, keep, bpos, anchor, S, 0.0)
    w = float(np.max(np.abs(np.asarray(got, LD) - want) / (m + 1e-300)))
    print("d = %d, K = %d, base %d, anchor %s: %.3g of the margin" % (d, K, bpos, anchor_pos, w))
    assert w < 1.0 and np.array_equal(got, got.T) and np.abs(got).max() > 1e6 * m.max()
    # explicit fma in one order on both sides (marg_math.h): the host twin has the same bits
    assert np.array_equal(got, dpgo_amd.marg_rel_debug(d, rec, S, bpos))
