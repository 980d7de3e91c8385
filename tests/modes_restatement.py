"""Restatement of the Hessian modes (dpgo_amd/csrc/modes.h): test infrastructure, like tests/newton_restatement.py and
tests/cov_restatement.py, which it builds on.  Plain numpy / scipy; nothing of the library is imported here.  Three parts:

  start_block   the hash start V0[i][j], bit for bit the library's modes_start_entry: splitmix64's finaliser of
                seed + 0x9e3779b97f4a7c15 (64 i + j + 1), its top 52 bits m mapped to (2 m + 1 - 2^52) 2^-52
  ritz          T c = theta G c on the lower triangles: G scaled to a unit diagonal, its Cholesky factor up to the first pivot
                below 1e-12 (the trailing columns are dropped and carried as e_j / sqrt(G_jj)), then a symmetric eigenproblem
  iterate       shift-invert block subspace iteration on the DENSE anchored Hessian of cov_restatement (`hessian`, `anchored`)
                with a dense Cholesky solve, in fp64 or -- the solves, the Gram matrices, the update and the residuals -- in
                long double; the values of the long-double run are the Rayleigh quotients of its vectors in long double

    mu = shift > 0 ? shift : 0;  a failed factorisation of A = H + mu I (non-anchor diagonal): mu = max(10 mu, 1e-3 hmax)
    V = V0;  per iteration  W = A^-1 V;  G = W'W, T = W'V;  (theta, C) = ritz(G, T);  R = V C - (W C) Theta;  V = W C
    column j < k is converged when |R_j| <= rel_tol hmax;  lambda_j = theta_j - mu
"""
import numpy as np
import scipy.linalg as sla

import factor_restatement as fr

LD = fr.LD
U = 2.0 ** -53
CONVERGED, MAX_ITERS, STALLED, SKIPPED = 0, 1, 2, 3
DEFAULTS = dict(guard=4, max_iters=100, max_tries=8, rel_tol=1e-8, shift=0.0, seed=1)


def block_of(k, guard=4):
    return 16 * ((k + guard + 15) // 16)


def start_block(n, b, seed=1, anchor_row0=-1, dof=0):
    """V0 (n, b) in float64; zeros on the rows anchor_row0 ... anchor_row0 + dof."""
    with np.errstate(over="ignore"):
        i = np.arange(n, dtype=np.uint64)[:, None]
        j = np.arange(b, dtype=np.uint64)[None, :]
        z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * (np.uint64(64) * i + j + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        m = (np.uint64(2) * (z >> np.uint64(12)) + np.uint64(1)).astype(np.int64) - np.int64(1 << 52)
    V = m.astype(np.float64) * (1.0 / 4503599627370496.0)
    if anchor_row0 >= 0:
        V[anchor_row0:anchor_row0 + dof] = 0.0
    return V


def ritz(G, T):
    """(theta (used,) ascending, C (b, b), used) from the lower triangles of G and T (float64)."""
    G = np.tril(np.asarray(G, np.float64))
    G = G + np.tril(G, -1).T
    T = np.tril(np.asarray(T, np.float64))
    T = T + np.tril(T, -1).T
    b = G.shape[0]
    g = np.diag(G)
    ds = np.where((g > 0) & np.isfinite(g), 1.0 / np.sqrt(np.where(g > 0, g, 1.0)), 0.0)
    Gs = G * ds[:, None] * ds[None, :]
    L = np.zeros((b, b))
    used = 0
    for j in range(b):
        if not ds[j] > 0:
            break
        row = sla.solve_triangular(L[:j, :j], Gs[j, :j], lower=True) if j else np.zeros(0)
        s = Gs[j, j] - float(row @ row)
        if not s >= 1e-12:
            break
        L[j, :j] = row
        L[j, j] = np.sqrt(s)
        used += 1
    C = np.zeros((b, b))
    for j in range(used, b):
        C[j, j] = ds[j]
    if used == 0:
        return np.zeros(0), C, 0
    Lu = L[:used, :used]
    Ts = T[:used, :used] * ds[:used, None] * ds[None, :used]
    As = sla.solve_triangular(Lu, sla.solve_triangular(Lu, Ts, lower=True).T, lower=True)
    As = 0.5 * (As + As.T)
    w, Z = np.linalg.eigh(As)
    C[:used, :used] = ds[:used, None] * sla.solve_triangular(Lu.T, Z, lower=False)
    return w, C, used


def hmax_of(A, anchor, dof):
    diag = np.array(np.diag(A), np.float64)
    diag[dof * anchor:dof * anchor + dof] = -np.inf
    return float(diag.max())


def _solver(A, ld):
    """X -> A^-1 X for the symmetric positive definite A, or None where the Cholesky factorisation meets a non-positive pivot."""
    if not ld:
        try:
            L = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            return None
        return lambda X: sla.cho_solve((L, True), X)
    L, kstar, _ = fr.cholesky_ld(A)
    if kstar >= 0:
        return None
    Li = fr.lower_inverse_ld(L)
    return lambda X: Li.T @ (Li @ np.asarray(X, LD))


def iterate(A, anchor, dof, k, ld=False, **opts):
    """A: the dense ANCHORED Hessian (the anchor's block the identity).  Returns a dict: outcome, iterations, factorisations,
    shift_tries, block, negative, mu, hmax, values (k), residuals (k), vectors (k, n) unit rows, history (iterations, k): the
    residual norms |R_j| of every iteration."""
    o = dict(DEFAULTS, **opts)
    A = np.asarray(A, np.float64)
    n = A.shape[0]
    b = block_of(k, o["guard"])
    dt = LD if ld else np.float64
    free = np.ones(n)
    free[dof * anchor:dof * anchor + dof] = 0.0
    hmax = hmax_of(A, anchor, dof)
    mu = o["shift"] if o["shift"] > 0 else 0.0
    out = dict(outcome=STALLED, iterations=0, factorisations=0, shift_tries=0, block=b, negative=0, mu=mu, hmax=hmax,
               values=np.zeros(k), residuals=np.zeros(k), vectors=np.zeros((k, n)), history=np.zeros((0, k)))
    solve = None
    for _ in range(o["max_tries"]):
        out["factorisations"] += 1
        solve = _solver(A + mu * np.diag(free), ld)
        if solve is not None:
            break
        out["shift_tries"] += 1
        mu = max(10.0 * mu, 1e-3 * hmax)
    out["mu"] = mu
    if solve is None:
        return out
    Amu = np.asarray(A + mu * np.diag(free), dt)
    V = np.asarray(start_block(n, b, o["seed"], dof * anchor, dof), dt)
    hist = []
    theta = rn = None
    converged = stalled = False
    for it in range(1, o["max_iters"] + 1):
        W = solve(V)
        G, T = W.T @ W, W.T @ V
        out["iterations"] = it
        th, C, used = ritz(np.asarray(G, np.float64), np.asarray(T, np.float64))
        if used < k:
            stalled = True
            break
        theta = np.concatenate([th, np.zeros(b - used)])
        Cd = np.asarray(C, dt)
        Vn = W @ Cd
        R = V @ Cd - Vn * np.asarray(theta, dt)[None, :]
        Vn[dof * anchor:dof * anchor + dof] = 0
        R[dof * anchor:dof * anchor + dof] = 0
        rn = np.asarray(np.sqrt(np.sum(R * R, axis=0)), np.float64)
        V = Vn
        hist.append(rn[:k].copy())
        if np.all(rn[:k] <= o["rel_tol"] * hmax):
            converged = True
            break
    if theta is None:
        return out
    out["outcome"] = CONVERGED if converged else (STALLED if stalled else MAX_ITERS)
    Vk = V[:, :k] / np.sqrt(np.sum(V[:, :k] * V[:, :k], axis=0))[None, :]
    out["vectors"] = np.asarray(Vk.T, np.float64)
    out["values"] = theta[:k] - mu
    if ld:   # the Rayleigh quotients in long double: exact to the square of the residual
        out["values"] = np.asarray(np.sum(Vk * (np.asarray(A, LD) @ Vk), axis=0), np.float64)
    out["residuals"] = rn[:k]
    out["negative"] = int(np.sum(out["values"] < 0)) if converged else 0
    out["history"] = np.array(hist).reshape(-1, k)
    return out


def spectrum(A, anchor, dof):
    """The ascending eigenvalues of the anchored Hessian with the anchor's rows and columns struck out (numpy.linalg.eigvalsh)."""
    keep = np.ones(A.shape[0], bool)
    keep[dof * anchor:dof * anchor + dof] = False
    return np.linalg.eigvalsh(np.asarray(A, np.float64)[np.ix_(keep, keep)])


def true_residuals(A, values, vectors):
    """|A v_j - lambda_j v_j|_2 in long double, v_j the rows of `vectors` (zero on the anchor's rows, where A is the identity)."""
    Al, Vl = np.asarray(A, LD), np.asarray(vectors, LD).T
    R = Al @ Vl - Vl * np.asarray(values, LD)[None, :]
    return np.asarray(np.sqrt(np.sum(R * R, axis=0)), np.float64)


def decisive(history, k, tol, factor=4.0):
    """The condition under which an iteration count may be compared: at the stopping iteration every residual sits at least
    `factor` below tol, and at the one before the largest sits at least `factor` above."""
    if len(history) < 2:
        return False
    return bool(np.all(history[-1][:k] * factor <= tol) and history[-2][:k].max() >= factor * tol)
