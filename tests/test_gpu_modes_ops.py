"""The kernels of the Hessian modes (dpgo_amd/csrc/modes.hip) one by one through their hooks, on the smallest shapes at which
they can go wrong: rows n in {1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 257, 1030} (below, at and above the four rows of one matrix
instruction, the 16 of a tile, the 32 of a slab, the 64 of a workgroup's pass, and -- 1030 -- more than the 512 rows of one
workgroup), blocks b in {16, 32, 64}, row lengths ld in {b, b + 3} (b: the 16-byte loads; b + 3 is odd: the scalar ones), and an
anchor block at the first, a middle and the last pose.

Bounds (u = 2^-53), against products in long double; nothing in them comes from the device.
  G, T      an entry is a sum of n products accumulated four at a time and then workgroup by workgroup:
            |G_ij - ref| <= (n + 4) u sum_r |W_ri| |W_rj|, likewise T with V
  V' = W C  a sum of b products: (b + 2) u sum_c |W_rc| |C_cj|
  sums      with eV that bound and eR = (b + 4) u (|V| |C| + |W| |C| |theta_j|)_rj the bound of an entry of
            R = V C - (W C) Theta (two such products, one multiplication, one subtraction), a column sum of squares is off by at
            most sum_r (2 |x| e + e^2) + (n + 2) u sum_r x^2
The start block is compared bit for bit with the numpy twin; a second call with the first; column j of a b = 16 call with column
j of a b = 64 call.  The columns b ... ld hold a sentinel that must come back bit for bit (and, at 1e200, would wreck every sum
that read it); the hooks put guard runs around the device copies and fail with -2 where one is written.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import modes_restatement as mr  # noqa: E402

import dpgo_amd  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
ROWS = [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 257, 1030]
BLOCKS = [16, 32, 64]
SENT = 1e200


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def lds(b):
    return (b, b + 3)


def anchors(n, dof):
    """(anchor_row0, dof): none, then the first, a middle and the last pose of the n // dof poses."""
    out = [(-1, 0)]
    P = n // dof
    for p in sorted({0, P // 2, P - 1}):
        if p >= 0 and P >= 1:
            out.append((dof * p, dof))
    return out


def block(rng, n, b, ld, scale=None):
    A = np.full((n, ld), SENT)
    A[:, :b] = rng.standard_normal((n, b)) * (1.0 if scale is None else scale)
    return A


@pytest.mark.parametrize("b", BLOCKS)
def test_start_block_is_the_numpy_twin(b):
    for n in ROWS:
        for ld in lds(b):
            for dof in (3, 6):
                for a0, adof in anchors(n, dof):
                    seed = 1 + n + ld
                    V = dpgo_amd.modes_init_debug(np.full((n, ld), SENT), b, seed=seed, anchor_row0=a0, dof=adof)
                    want = mr.start_block(n, b, seed, a0, adof)
                    assert np.array_equal(bits(V[:, :b]), bits(want)), (n, b, ld, a0)
                    assert np.all(bits(V[:, b:]) == bits(np.array([SENT]))[0])
                    if a0 >= 0:
                        assert not V[a0:a0 + adof, :b].any()
    # a column's bits depend neither on b nor on n
    V16 = dpgo_amd.modes_init_debug(np.zeros((257, 16)), 16, seed=9)
    V64 = dpgo_amd.modes_init_debug(np.zeros((1030, 64)), 64, seed=9)
    assert np.array_equal(bits(V16), bits(V64[:257, :16]))


@pytest.mark.parametrize("b", BLOCKS)
def test_gram_against_long_double(b):
    rng = np.random.default_rng(100 + b)
    worst = 0.0
    for n in ROWS:
        for ld in lds(b):
            W = block(rng, n, b, ld, np.exp(rng.uniform(-1, 1, b))[None, :])
            V = block(rng, n, b, ld)
            G, T = dpgo_amd.modes_gram_debug(W, V, b)
            Wl, Vl = np.asarray(W[:, :b], LD), np.asarray(V[:, :b], LD)
            Gref = Wl.T @ Wl
            Tref = np.tril(Wl.T @ Vl)
            Tref = Tref + np.tril(Tref, -1).T
            bG = (n + 4) * U * (np.abs(W[:, :b]).T @ np.abs(W[:, :b]))
            bT = np.tril((n + 4) * U * (np.abs(W[:, :b]).T @ np.abs(V[:, :b])))
            bT = bT + np.tril(bT, -1).T
            eG, eT = np.abs(np.asarray(G, LD) - Gref), np.abs(np.asarray(T, LD) - Tref)
            worst = max(worst, float((eG / bG).max()), float((eT / bT).max()))
            assert np.all(eG <= bG) and np.all(eT <= bT), (n, b, ld)
            assert np.array_equal(bits(G), bits(G.T)) and np.array_equal(bits(T), bits(T.T))
            G2, T2 = dpgo_amd.modes_gram_debug(W, V, b)
            assert np.array_equal(bits(G), bits(G2)) and np.array_equal(bits(T), bits(T2))
    print("b = %d: worst error / bound %.3g" % (b, worst))


def test_gram_entry_does_not_depend_on_the_block():
    """Column j of a b = 16 call against column j of a b = 64 call, in both load paths and over more than one workgroup; and the
    operands really are (W, V): an asymmetric pair gives T = W'V, not V'W."""
    rng = np.random.default_rng(7)
    for n in (17, 1030):
        for ld16, ld64 in ((16, 64), (19, 67), (16, 67)):
            W64, V64 = block(rng, n, 64, ld64), block(rng, n, 64, ld64)
            W16, V16 = np.full((n, ld16), SENT), np.full((n, ld16), SENT)
            W16[:, :16], V16[:, :16] = W64[:, :16], V64[:, :16]
            G16, T16 = dpgo_amd.modes_gram_debug(W16, V16, 16)
            G64, T64 = dpgo_amd.modes_gram_debug(W64, V64, 64)
            assert np.array_equal(bits(G16), bits(G64[:16, :16])) and np.array_equal(bits(T16), bits(T64[:16, :16]))
    W = np.zeros((4, 16))
    V = np.zeros((4, 16))
    W[0, 3], V[0, 1] = 2.0, 5.0     # W'V has its one entry at (3, 1): below the diagonal, handed out and mirrored
    G, T = dpgo_amd.modes_gram_debug(W, V, 16)
    want = np.zeros((16, 16))
    want[3, 1] = want[1, 3] = 10.0
    assert np.array_equal(T, want) and G[3, 3] == 4.0 and np.count_nonzero(G) == 1
    W[0, 3], W[0, 1], V[0, 1], V[0, 3] = 0.0, 2.0, 0.0, 5.0   # ... and at (1, 3): above it, not part of the lower triangle
    assert not dpgo_amd.modes_gram_debug(W, V, 16)[1].any()


def update_reference(W, V, Cm, theta, b, a0, adof):
    Wl, Vl, Cl = np.asarray(W[:, :b], LD), np.asarray(V[:, :b], LD), np.asarray(Cm, LD)
    Vn = Wl @ Cl
    R = Vl @ Cl - Vn * np.asarray(theta, LD)[None, :]
    aW, aV, aC = np.abs(W[:, :b]), np.abs(V[:, :b]), np.abs(Cm)
    eV = (b + 2) * U * (aW @ aC)
    eR = (b + 4) * U * (aV @ aC + (aW @ aC) * np.abs(theta)[None, :])
    if a0 >= 0:
        for M in (Vn, R, eV, eR):
            M[a0:a0 + adof] = 0
    n = W.shape[0]
    brr = np.sum(2 * np.abs(R) * eR + eR * eR, axis=0) + (n + 2) * U * np.sum(R * R, axis=0)
    bvv = np.sum(2 * np.abs(Vn) * eV + eV * eV, axis=0) + (n + 2) * U * np.sum(Vn * Vn, axis=0)
    return Vn, eV, np.sum(R * R, axis=0), brr, np.sum(Vn * Vn, axis=0), bvv


@pytest.mark.parametrize("b", BLOCKS)
def test_update_against_long_double(b):
    rng = np.random.default_rng(300 + b)
    worst = [0.0, 0.0, 0.0]
    for n in ROWS:
        for ld in lds(b):
            W, V = block(rng, n, b, ld), block(rng, n, b, ld)
            Cm = rng.standard_normal((b, b)) / np.sqrt(b)
            theta = rng.uniform(0.1, 3.0, b)
            for a0, adof in anchors(n, 6 if n % 6 == 0 or n > 64 else 3):
                Vn, rr, vv = dpgo_amd.modes_update_debug(W, V, Cm, theta, b, anchor_row0=a0, dof=adof)
                ref, eV, rr_ref, brr, vv_ref, bvv = update_reference(W, V, Cm, theta, b, a0, adof)
                err = np.abs(np.asarray(Vn[:, :b], LD) - ref)
                assert np.all(err <= eV), (n, b, ld, a0)
                assert np.all(np.abs(np.asarray(rr, LD) - rr_ref) <= brr) and np.all(np.abs(np.asarray(vv, LD) - vv_ref) <= bvv)
                free = np.ones(n, bool)
                if a0 >= 0:
                    free[a0:a0 + adof] = False
                    assert not Vn[a0:a0 + adof, :b].any()
                if free.any():
                    worst[0] = max(worst[0], float((err[free] / eV[free]).max()))
                    worst[1] = max(worst[1], float((np.abs(np.asarray(rr, LD) - rr_ref) / brr).max()))
                    worst[2] = max(worst[2], float((np.abs(np.asarray(vv, LD) - vv_ref) / bvv).max()))
                assert np.array_equal(bits(Vn[:, b:]), bits(V[:, b:]))          # the columns b ... ld: not touched
                again = dpgo_amd.modes_update_debug(W, V, Cm, theta, b, anchor_row0=a0, dof=adof)
                assert all(np.array_equal(bits(x), bits(y)) for x, y in zip((Vn, rr, vv), again))
    print("b = %d: worst error / bound: V' %.3g, residual sums %.3g, norm sums %.3g" % (b, *worst))


def test_update_column_does_not_depend_on_the_block():
    """C of order 16 inside a zero C of order 64: the longer sums add exact zeros, so the first 16 columns and their sums
    keep their bits."""
    rng = np.random.default_rng(11)
    for n in (17, 1030):
        W64, V64 = block(rng, n, 64, 67), block(rng, n, 64, 67)
        C16, th16 = rng.standard_normal((16, 16)), rng.uniform(0.1, 3.0, 16)
        C64, th64 = np.zeros((64, 64)), np.zeros(64)
        C64[:16, :16], th64[:16] = C16, th16
        o64 = dpgo_amd.modes_update_debug(W64, V64, C64, th64, 64, anchor_row0=6, dof=6)
        o16 = dpgo_amd.modes_update_debug(W64[:, :16].copy(), V64[:, :16].copy(), C16, th16, 16, anchor_row0=6, dof=6)
        assert np.array_equal(bits(o16[0]), bits(o64[0][:, :16]))
        assert np.array_equal(bits(o16[1]), bits(o64[1][:16])) and np.array_equal(bits(o16[2]), bits(o64[2][:16]))
        assert not o64[0][:, 16:64].any()


def test_ritz_on_device_blocks_is_the_host_hook_on_their_gram_matrices():
    rng = np.random.default_rng(5)
    W, V = block(rng, 257, 32, 35), block(rng, 257, 32, 35)
    G, T = dpgo_amd.modes_gram_debug(W, V, 32)
    th, Cm, used = dpgo_amd.modes_ritz_debug(G, T)
    th2, C2, used2 = dpgo_amd.modes_ritz_debug(W=W, V=V, b=32)
    assert used == used2 == 32 and np.array_equal(bits(th), bits(th2)) and np.array_equal(bits(Cm), bits(C2))
    # one step of the iteration through the hooks: the new block is G-orthonormal by construction, so its own Gram matrix is I
    Vn, rr, vv = dpgo_amd.modes_update_debug(W, V, Cm, th, 32)
    G2, _ = dpgo_amd.modes_gram_debug(Vn, Vn, 32)
    ds = 1.0 / np.sqrt(np.diag(G))
    kappa = float(np.linalg.cond(G * ds[:, None] * ds[None, :]))
    assert np.abs(G2 - np.eye(32)).max() <= 8 * (257 + 32 * 32) * U * kappa
    assert np.abs(vv - 1.0).max() <= 8 * (257 + 32 * 32) * U * kappa
