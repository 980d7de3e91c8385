"""Restatements for the marginal covariances: test infrastructure, like tests/factor_restatement.py and
tests/cert_restatement.py.  Plain numpy / scipy; nothing of the library is imported here.  Two of them: the selected
inversion (dpgo_amd/csrc/spd.h: spd_selinv_*), first, and the matrix it is applied to, the Riemannian Hessian in tangent
coordinates (dpgo_amd/csrc/cov.h), at the end of the file.

With W_s = [W_top ; W_bot] = [L11^-1 ; -L21 L11^-1] of front s (w pivots, u update rows) and S_uu the block of A^-1 on its
update rows, read from the parent's finished block,

    T = S_uu W_bot,    S_pp = W_top^T W_top + W_bot^T T,    S_front = [[S_pp, T^T], [T, S_uu]],

and S_front = W_top^T W_top for a root.  `recursion` runs this on W blocks it is given -- factor_restatement.Reference.W_fp64
(ordinary fp64: what the library's arithmetic can be expected to reach) or Reference.W (np.longdouble) -- so nothing in it
comes from the library but the front list.  The reference every entry is held against is the dense long-double inverse,
`inverse_ld`, which knows nothing of fronts.

The bound (entrywise, one number per matrix):   |S - S_ref| <= C * 2^-53 * kappa_2(A) * ||A^-1||_2
kappa_2 and the norm come from the dense matrix (eigvalsh).  C is chosen on the CPU before any device is asked: the fp64
restatement must stay within a quarter of the bound on every input (tests/test_covariance_host.py asserts it and DESIGN.md
section 14 holds the table).  C = 8 is the smallest power of two that does: with C = 1 the restatement reaches 1.75 on
arrow_wide and 1.35 on arrow_block4 -- the "mixed" family, kappa_2 = 4 - 5, where kappa_2 leaves no room for the length of the
sums (up to 451 terms per entry) -- and 5e-5 ... 3e-2 on the others; the long-double restatement stays below 2e-3 of the
C = 1 bound everywhere, so what is measured is rounding and not the recursion.
"""
import numpy as np

import factor_restatement as fr

LD = fr.LD
U = fr.U
C = 8.0


def inverse_ld(ref):
    """A^-1 in long double, in the ORIGINAL index order, from the reference's long-double Cholesky factor of the permuted
    matrix: A_p^-1 = L^-T L^-1."""
    assert ref.kstar < 0
    X = fr.lower_inverse_ld(ref.L)
    Sp = X.T @ X
    S = np.zeros_like(Sp)
    S[np.ix_(ref.perm, ref.perm)] = Sp
    return S


def front_indices(res, s):
    return np.concatenate([np.asarray(res["piv_idx"][s], np.int64), np.asarray(res["upd_idx"][s], np.int64)])


def recursion(res, W_of, dtype):
    """[S_front of every front] by the recursion above, in `dtype`; W_of(s): the (w + u) x w block of front s."""
    nt = res["nfronts"]
    out = [None] * nt
    for s in range(nt - 1, -1, -1):   # post-order backwards: parents first
        w, u = int(res["w"][s]), int(res["u"][s])
        W = np.asarray(W_of(s), dtype)
        top, bot = W[:w], W[w:]
        S = np.zeros((w + u, w + u), dtype)
        if u:
            p = int(res["parent"][s])
            where = {int(v): k for k, v in enumerate(front_indices(res, p))}
            pos = np.array([where[int(v)] for v in res["upd_idx"][s]], np.int64)
            Suu = out[p][np.ix_(pos, pos)]
            T = Suu @ bot
            S[w:, w:] = Suu
            S[w:, :w] = T
            S[:w, w:] = T.T
            S[:w, :w] = top.T @ top + bot.T @ T
        else:
            S[:w, :w] = top.T @ top
        out[s] = S
    return out


def bound(ref):
    """C u kappa_2(A) ||A^-1||_2; ||A^-1||_2 = 1 / lambda_min."""
    lam = np.linalg.eigvalsh(ref.Ap)
    assert lam[0] > 0
    return C * U * float(lam[-1] / lam[0]) / float(lam[0])


def worst_ratio(res, blocks, Sref, bnd):
    """max over the fronts and over every entry of their blocks of |S - S_ref| / bound."""
    worst = 0.0
    for s in range(res["nfronts"]):
        idx = front_indices(res, s)
        err = np.abs(np.asarray(blocks[s], LD) - Sref[np.ix_(idx, idx)]).max() if len(idx) else 0.0
        worst = max(worst, float(err) / bnd)
    return worst


def symmetric_bits(blocks):
    return all(np.array_equal(B.view(np.int64), np.ascontiguousarray(B.T).view(np.int64)) for B in blocks)


def same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(x.view(np.int64), y.view(np.int64)) for x, y in zip(a, b))


# the references are slow (long-double n^3 in numpy) and shared: built once per process
_refs = {}


def reference(name, res):
    """(factor_restatement.Reference, A^-1 in long double, the bound) of a named input of factor_restatement.INPUTS."""
    if name not in _refs:
        A, _ = fr.build_input(name)
        ref = fr.Reference(A, res)
        _refs[name] = (ref, inverse_ld(ref), bound(ref))
    return _refs[name]


# ---------------------------------------------------------------------------------------------------------------
# the matrix: the Riemannian Hessian in tangent coordinates (dpgo_amd/csrc/cov.h)
# ---------------------------------------------------------------------------------------------------------------
def dof_of(d):
    return d + d * (d - 1) // 2


def hat(w, d):
    """The standard hat map: so(3) from a 3-vector, [[0, -w], [w, 0]] for d = 2."""
    if d == 2:
        return np.array([[0.0, -w[0]], [w[0], 0.0]])
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def tangent_basis(X, d):
    """J[c]: ((d+1) N) x (dof N), column dof p + a = column c of the basis direction E_a(p) in the reference layout (row p
    the translation, rows N + d p + r the rows of Y_p): E_i = e_0 e_i^T, E_{d+k} = [0 ; -hat(e_k) Y_p]."""
    N = X.shape[0] // (d + 1)
    dof = dof_of(d)
    J = np.zeros((d, (d + 1) * N, dof * N))
    for p in range(N):
        Y = X[N + d * p:N + d * p + d]
        for i in range(d):
            J[i, p, dof * p + i] = 1.0
        for k in range(dof - d):
            e = np.zeros(dof - d)
            e[k] = 1.0
            Bk = -hat(e, d) @ Y
            for c in range(d):
                J[c, N + d * p:N + d * p + d, dof * p + d + k] = Bk[:, c]
    return J


def hessian(S, X, d):
    """H[dof p + a, dof q + b] = tr(E_a(p)^T S E_b(q)), dense; S: the certificate matrix in the reference layout."""
    Sd = S.toarray() if hasattr(S, "toarray") else np.asarray(S)
    J = tangent_basis(X, d)
    return sum(J[c].T @ Sd @ J[c] for c in range(d))


def anchored(H, anchor, dof):
    """The gauge: the anchor's rows and columns become those of the identity."""
    A = np.array(H)
    r = slice(dof * anchor, dof * anchor + dof)
    A[r, :] = 0.0
    A[:, r] = 0.0
    A[r, r] = np.eye(dof)
    return A


def retract(X, v, d):
    """The point the tangent coordinates v (dof N) lead to: t_p + dt, R_p Exp(hat(omega)), i.e. Y_p <- Exp(hat(omega))^T Y_p."""
    import scipy.linalg as sla
    N = X.shape[0] // (d + 1)
    dof = dof_of(d)
    Z = np.array(X)
    for p in range(N):
        Z[p] = X[p] + v[dof * p:dof * p + d]
        Z[N + d * p:N + d * p + d] = sla.expm(hat(v[dof * p + d:dof * p + dof], d)).T @ X[N + d * p:N + d * p + d]
    return Z


def random_rotations_point(X, d, seed):
    """X with every rotation replaced by a seeded random one (translations kept): far from any critical point."""
    rng = np.random.default_rng(seed)
    N = X.shape[0] // (d + 1)
    Z = np.array(X)
    for p in range(N):
        Q, R = np.linalg.qr(rng.standard_normal((d, d)))
        Q = Q * np.sign(np.diag(R))
        if np.linalg.det(Q) < 0:
            Q[:, 0] = -Q[:, 0]
        Z[N + d * p:N + d * p + d] = Q
    return Z
