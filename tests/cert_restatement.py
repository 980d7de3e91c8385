"""numpy / scipy restatement of the solution certificate (dpgo_amd/csrc/cert.h) on the oracle's explicit data matrix
(oracle.star.GlobalProblem.M): test infrastructure, like tests/pcm_restatement.py.

Semantics (reference layout: X is (d+1)N x d, rows 0..N-1 the translations, rows N + d p + r the rows of Y_p = R_p^T,
C++/DPGO/include/DPGO/DPGOProblem.h:167-171):
  Lambda_p = 1/2 (P + P^T), P = (M X)[rows of Y_p] (X[rows of Y_p])^T     compute_Lambda_blocks, SESyncProblem.cpp:375-395
  S = M - blkdiag(0_N, Lambda_0, ..., Lambda_{N-1})                        verify_solution, SESyncProblem.cpp:444-447
  LOBPCG on S, block size d, basis [V W P]                                 fast_verification STEP 2, SESync_utils.cpp:765-826;
                                                                           LOBPCG.h:131-337
"""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

UNDECIDED, NONNEGATIVE, NEGATIVE = 0, 1, 2


def lambda_blocks(M, X, d):
    """(N, d, d): the symmetric blocks Lambda_p."""
    N = X.shape[0] // (d + 1)
    MX = M @ X
    Y, MY = X[N:].reshape(N, d, d), MX[N:].reshape(N, d, d)
    P = MY @ Y.transpose(0, 2, 1)   # (batched matmul: the form of SOdProduct::SymBlockDiagProduct, SOdProduct.h:64-89)
    return 0.5 * (P + P.transpose(0, 2, 1))


def S_matrix(M, X, d):
    """The certificate matrix as a scipy CSR matrix."""
    N = X.shape[0] // (d + 1)
    Lam = lambda_blocks(M, X, d)
    rows = N + (np.arange(N)[:, None, None] * d + np.arange(d)[None, :, None] + 0 * np.arange(d)[None, None, :])
    cols = N + (np.arange(N)[:, None, None] * d + 0 * np.arange(d)[None, :, None] + np.arange(d)[None, None, :])
    L = sp.coo_matrix((Lam.ravel(), (rows.ravel(), cols.ravel())), shape=M.shape)
    return (sp.csr_matrix(M) - L.tocsr()).tocsr()


def apply(M, X, V, d, Lam=None):
    """S(X) V without forming S: (S V).x = (M V).x, (S V)_p.Y = (M V)_p.Y - Lambda_p V_p.Y."""
    N = X.shape[0] // (d + 1)
    if Lam is None:
        Lam = lambda_blocks(M, X, d)
    V = np.asarray(V, dtype=np.float64)
    SV = np.array(M @ V)
    nc = V.shape[1]
    SV[N:] = SV[N:] - (Lam @ V[N:].reshape(N, d, nc)).reshape(N * d, nc)
    return SV


def block_jacobi(M, d):
    """T_p = (M_pp)^-1 per pose ((d+1) x (d+1), rows {p, N + d p ..}), identity where M_pp is not positive definite (a
    pose without an edge); returns (N, d+1, d+1)."""
    M = sp.coo_matrix(M)
    N = M.shape[0] // (d + 1)

    def pose(i):
        return np.where(i < N, i, (i - N) // d)

    def slot(i):
        return np.where(i < N, 0, 1 + (i - N) % d)

    same = pose(M.row) == pose(M.col)
    blk = np.zeros((N, d + 1, d + 1))
    np.add.at(blk, (pose(M.row[same]), slot(M.row[same]), slot(M.col[same])), M.data[same])
    blk = 0.5 * (blk + blk.transpose(0, 2, 1))
    w = np.linalg.eigvalsh(blk)
    ok = w[:, 0] > 1e-12 * np.maximum(w[:, -1], 1e-300)
    T = np.tile(np.eye(d + 1), (N, 1, 1))
    T[ok] = np.linalg.inv(blk[ok])
    return T


def apply_block_jacobi(T, R, d):
    N = T.shape[0]
    out = np.empty_like(R)
    rec = np.concatenate([R[:N, None, :], R[N:].reshape(N, d, R.shape[1])], axis=1)   # (N, d+1, nc)
    rec = np.einsum("pij,pjc->pic", T, rec)
    out[:N] = rec[:, 0]
    out[N:] = rec[:, 1:].reshape(N * d, R.shape[1])
    return out


def rayleigh_ritz(A, B, ns, nblk):
    """The Rayleigh-Ritz step: scale by diag(B)^-1/2, Cholesky of the mass matrix (a pivot < 1e-12 drops the last block),
    symmetric eigenproblem.  Returns (theta[:ns], C (n x ns), used)."""
    nfull = ns * nblk
    for used in range(nblk, 0, -1):
        n = ns * used
        b = np.diag(B)[:n]
        if not np.all(b > 0):
            continue
        s = 1.0 / np.sqrt(b)
        Bs = 0.5 * (B[:n, :n] + B[:n, :n].T) * np.outer(s, s)
        As = 0.5 * (A[:n, :n] + A[:n, :n].T) * np.outer(s, s)
        L = np.zeros((n, n))
        ok = True
        for j in range(n):
            piv = Bs[j, j] - L[j, :j] @ L[j, :j]
            if not piv >= 1e-12:
                ok = False
                break
            L[j, j] = np.sqrt(piv)
            L[j + 1:, j] = (Bs[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
        if not ok:
            continue
        Y = sla.solve_triangular(L, As, lower=True)
        At = sla.solve_triangular(L, Y.T, lower=True).T
        w, Z = np.linalg.eigh(0.5 * (At + At.T))
        C = np.zeros((nfull, ns))
        C[:n] = s[:, None] * sla.solve_triangular(L.T, Z[:, :ns], lower=False)
        return w[:ns], C, used
    raise np.linalg.LinAlgError("rayleigh_ritz: the first block has no positive definite mass matrix")


def status_of(theta, residual, S_norm_est, eta, tau):
    if theta < -0.5 * eta:
        return NEGATIVE
    if residual <= tau * (S_norm_est + abs(theta)):
        return NONNEGATIVE
    return UNDECIDED


def tri_index(n, a, c):
    """Position of entry (a, c), a <= c, in the device's row-major upper triangle of an n x n matrix (cert_tri, cert.h)."""
    return a * n - a * (a - 1) // 2 + (c - a)


def upper_triangles(G, A):
    """Both Gram matrices as the device ships them: the upper triangles of B^T B and of B^T (S B), row-major, in that order."""
    iu = np.triu_indices(G.shape[0])
    return np.concatenate([G[iu], A[iu]])


def gram_step(M, Lam, V, W, P, SV, SP, d, MW=None, dtype=np.float64):
    """The products one pass of the loop reads, in `dtype`: S W = M W - [0 ; Lambda W_Y] (M W given as MW, or formed here),
    G = B^T B and A = B^T (S B) with B = [V W P], S B = [SV SW SP].  A is NOT symmetrised: entry (a, c) is B_a^T (S B)_c,
    which is what the device sums for a <= c.  Returns (G, A, SW)."""
    V, W, P, SV, SP = (np.asarray(Z, dtype=dtype) for Z in (V, W, P, SV, SP))
    N = V.shape[0] // (d + 1)
    nc = W.shape[1]
    if MW is None:
        MW = (M if dtype == np.float64 else sp.csr_matrix(M).astype(dtype)) @ W
    SW = np.array(MW, dtype=dtype)
    SW[N:] = SW[N:] - (np.asarray(Lam, dtype=dtype) @ W[N:].reshape(N, d, nc)).reshape(N * d, nc)
    Bb, SB = np.hstack([V, W, P]), np.hstack([SV, SW, SP])
    return Bb.T @ Bb, Bb.T @ SB, SW


def update_step(C, theta, V, W, P, SV, SW, SP, T, d, dtype=np.float64):
    """The recurrences of one pass, in `dtype`: C is 3d x d (rows of V, W, P), T the block-Jacobi blocks or None.
    P' = W C_w + P C_p, V' = V C_v + P', the same for S V', S P'; R' = S V' - V' diag(theta); W' = T R' (R' without T).
    Returns a dict with V, W, P, SV, SP, R and the stopping test's sums rr[j] = |R'_j|^2, vv[j] = |V'_j|^2."""
    C, theta, V, W, P, SV, SW, SP = (np.asarray(Z, dtype=dtype) for Z in (C, theta, V, W, P, SV, SW, SP))
    Pn = W @ C[d:2 * d] + P @ C[2 * d:]
    SPn = SW @ C[d:2 * d] + SP @ C[2 * d:]
    Vn, SVn = V @ C[:d] + Pn, SV @ C[:d] + SPn
    R = SVn - Vn * theta[None, :]
    Wn = apply_block_jacobi(np.asarray(T, dtype=dtype), R, d) if T is not None else R
    return dict(V=Vn, W=Wn, P=Pn, SV=SVn, SP=SPn, R=R, rr=np.sum(R * R, axis=0), vv=np.sum(Vn * Vn, axis=0))


def lobpcg(M, X, d, V0, eta=1e-3, tau=1e-6, max_iters=2000, precondition=True, stop_on_negative=True, refresh_every=50,
           seed=0):
    """The search as the device runs it: same recurrences, the stopping test one product late, theta / residual of the
    result from one fresh product S x.  Returns a dict with status, iterations, restarts, theta, residual, S_norm_est,
    stationarity, x."""
    Lam = lambda_blocks(M, X, d)
    S = lambda V: apply(M, X, V, d, Lam)
    T = block_jacobi(M, d) if precondition else None
    Om = np.random.default_rng(seed + 12345).standard_normal(X.shape)
    Sn = np.linalg.norm(S(Om)) / np.linalg.norm(Om)
    res = dict(S_norm_est=Sn, stationarity=float(np.linalg.norm(S(X))), restarts=0)
    V = np.array(V0, dtype=np.float64)
    SV = S(V)
    W, P, SW, SP = (np.zeros_like(V) for _ in range(4))
    it, theta0, have_norms, have_W, drop_P = 0, 0.0, False, False, True
    while True:
        while it < max_iters:
            G, A, SW = gram_step(M, Lam, V, W, P, SV, SP, d, MW=None if have_W else SW)   # (no W yet: W = M W = 0)
            if have_norms and r0 <= tau * (Sn + abs(theta0)) * x0:
                break
            nblk = 1 if not have_W else (2 if drop_P else 3)
            n = d * nblk
            th, C, used = rayleigh_ritz(A[:n, :n], G[:n, :n], d, nblk)
            res["restarts"] += used < nblk
            Cf = np.zeros((3 * d, d))
            Cf[:n] = C
            new = update_step(Cf, th, V, W, P, SV, SW, SP, T, d)
            V, W, P, SV, SP = (new[k] for k in ("V", "W", "P", "SV", "SP"))
            r0, x0 = np.linalg.norm(new["R"][:, 0]), np.linalg.norm(V[:, 0])
            it += 1
            theta0, have_norms = th[0], True
            drop_P, have_W = not have_W, True
            if stop_on_negative and theta0 < -0.5 * eta:
                break
            if refresh_every > 0 and it % refresh_every == 0:
                SV, SP = S(V), S(P)
        x = V[:, 0] / np.linalg.norm(V[:, 0])
        x = x / np.linalg.norm(x)
        sx = S(x[:, None])[:, 0]
        theta = float(x @ sx)
        resid = float(np.linalg.norm(sx - theta * x))
        st = status_of(theta, resid, Sn, eta, tau)
        if st != UNDECIDED or it >= max_iters:
            break
        SV, SP, have_norms = S(V), S(P), False
    res.update(status=st, iterations=it, theta=theta, residual=resid, x=x)
    return res
