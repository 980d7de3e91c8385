"""Restatement of the Riemannian staircase (dpgo_amd/csrc/stair.h): test infrastructure, like tests/newton_restatement.py and
tests/cert_restatement.py, which it imports.  Plain numpy / scipy on the oracle's explicit data matrix
(oracle.star.GlobalProblem.M), the trust-region method itself being oracle.tnt.tnt driven with callables for the lifted
problem; nothing of the library is imported here.

A point at rank r is X, (d+1)N x r (or wider, with zero columns) in the reference's row order: rows 0..N-1 the translations,
rows N + d p + k the rows of Y_p (d x r), Y_p Y_p^T = I.

    F = 1/2 tr(X^T M X);  Lambda_p = sym((M X)_p.Y Y_p^T);  grad F = S X, S = M - Lambda;  Hess[V] = Proj_X(S V)
    Proj_X(W)_p.Y = W_p.Y - sym(W_p.Y Y_p^T) Y_p;  retract: t + v, the polar factor of Y_p + V_p.Y

    r = d;  Y = X
    repeat:  Y = TNT(Y);  lambda_min, x = the smallest eigenpair of S(Y) (dense eigh here; verify on the device)
             lambda_min >= -eta / 2 -> SOLVED;   r == r_max -> MAX_RANK
             Ydot = x in a new zero column;  alpha = 1, at most 30 times: Z = retract(Y, alpha Ydot), accepted when
             F(Z) <= F(Y) + 1/4 alpha^2 lambda_min, else alpha /= 2;   none accepted -> SADDLE;   Y = Z, r += 1
    round:   B = the d leading eigenvectors of sum_p Y_p^T Y_p, each signed so that its entry of largest magnitude is
             positive; X B, the last column of B negated where most det(Y_p B) are negative, every Y_p B onto SO(d)
"""
import numpy as np
import scipy.sparse as sp

import cert_restatement as cert
from oracle import tnt as otnt

SOLVED, MAX_RANK, SADDLE, SKIPPED = 0, 1, 2, 3
# the tight options of the tests: the absolute gradient test alone
TIGHT = dict(grad_norm_tol=1e-8, preconditioned_grad_norm_tol=0.0, rel_func_decrease_tol=0.0, stepsize_tol=0.0)
DEFAULTS = dict(grad_norm_tol=1e-2, preconditioned_grad_norm_tol=1e-4, rel_func_decrease_tol=1e-6, stepsize_tol=1e-3,
                max_iterations=1000, max_tCG_iterations=10000, STPCG_kappa=0.1, STPCG_theta=0.5)


def sym(A):
    return 0.5 * (A + np.swapaxes(A, -1, -2))


def rot(X, d):
    """(N, d, r): the blocks Y_p."""
    N = X.shape[0] // (d + 1)
    return X[N:].reshape(N, d, X.shape[1])


def objective(M, X):
    return 0.5 * float(np.sum(X * (M @ X)))


def lambda_blocks(M, X, d):
    return sym(rot(M @ X, d) @ rot(X, d).transpose(0, 2, 1))


def apply_S(M, X, V, d, Lam=None):
    """S(X) V: (M V).t, (M V)_p.Y - Lambda_p V_p.Y."""
    N = X.shape[0] // (d + 1)
    if Lam is None:
        Lam = lambda_blocks(M, X, d)
    SV = np.array(M @ V)
    SV[N:] -= (Lam @ rot(V, d)).reshape(N * d, V.shape[1])
    return SV


def proj(X, W, d):
    N = X.shape[0] // (d + 1)
    Y = rot(X, d)
    out = np.array(W)
    out[N:] -= (sym(rot(W, d) @ Y.transpose(0, 2, 1)) @ Y).reshape(N * d, X.shape[1])
    return out


def grad(M, X, d):
    """S X: tangent as it stands (sym((S X)_p.Y Y_p^T) = 0 by the choice of Lambda)."""
    return apply_S(M, X, X, d)


def hess(M, X, V, d, Lam=None):
    return proj(X, apply_S(M, X, V, d, Lam), d)


def retract(X, V, d):
    N = X.shape[0] // (d + 1)
    Z = X + V
    U, _, Vt = np.linalg.svd(rot(Z, d), full_matrices=False)
    Z[N:] = (U @ Vt).reshape(N * d, X.shape[1])
    return Z


def precondition(T, X, V, d):
    """Proj o T_p o Proj with the certificate's block-Jacobi T_p."""
    return proj(X, cert.apply_block_jacobi(T, proj(X, V, d), d), d)


def S_matrix(M, X, d):
    N = X.shape[0] // (d + 1)
    Lam = lambda_blocks(M, X, d)
    rows = N + (np.arange(N)[:, None, None] * d + np.arange(d)[None, :, None] + 0 * np.arange(d)[None, None, :])
    cols = N + (np.arange(N)[:, None, None] * d + 0 * np.arange(d)[None, :, None] + np.arange(d)[None, None, :])
    L = sp.coo_matrix((Lam.ravel(), (rows.ravel(), cols.ravel())), shape=M.shape)
    return (sp.csr_matrix(M) - L.tocsr()).tocsr()


def min_eigenpair(M, X, d):
    w, Z = np.linalg.eigh(S_matrix(M, X, d).toarray())
    return float(w[0]), Z[:, 0]


def tnt_level(M, X, d, T=None, **opts):
    """oracle.tnt.tnt on the lifted problem.  Returns (X, F, |grad|, outer iterations, Hessian products)."""
    o = dict(DEFAULTS, **opts)
    p = otnt.TNTParams()
    p.max_iterations = p.max_iterations_accepted = o["max_iterations"]
    p.gradient_tolerance = o["grad_norm_tol"]
    p.preconditioned_gradient_tolerance = o["preconditioned_grad_norm_tol"]
    p.relative_decrease_tolerance = o["rel_func_decrease_tol"]
    p.stepsize_tolerance = o["stepsize_tol"]
    p.max_TPCG_iterations = o["max_tCG_iterations"]
    p.kappa_fgr, p.theta = o["STPCG_kappa"], o["STPCG_theta"]
    count = [0]

    def QM(x):
        Lam = lambda_blocks(M, x, d)

        def H(xx, v):
            count[0] += 1
            return hess(M, xx, v, d, Lam)
        return apply_S(M, x, x, d, Lam), H

    log = []
    out = otnt.tnt(lambda x: objective(M, x), QM, lambda x, a, b: float(np.sum(a * b)), lambda x, v: retract(x, v, d), X,
                   precon=(lambda x, v: precondition(T, x, v, d)) if T is not None else None, params=p, log=log)
    # (tnt() takes one more product per iteration for the model's decrease; the device accumulates H s inside the CG)
    return out["x"], out["f"], out["gradfx_norm"], len(log), count[0] - len(log)


def round_solution(X, d):
    """(Xhat, B, the singular values of the rotation rows, descending)."""
    N = X.shape[0] // (d + 1)
    R = X[N:]
    w, Z = np.linalg.eigh(R.T @ R)
    order = np.argsort(-w, kind="stable")
    sigma = np.sqrt(np.maximum(w[order], 0.0))
    B = Z[:, order[:d]].copy()
    for j in range(d):
        if B[np.argmax(np.abs(B[:, j])), j] < 0:
            B[:, j] = -B[:, j]
    W = X @ B
    if 2 * int(np.sum(np.linalg.det(rot(W, d)) > 0)) < N:
        B[:, -1] = -B[:, -1]
        W = X @ B
    U, _, Vt = np.linalg.svd(rot(W, d))
    flip = np.linalg.det(U @ Vt) < 0
    U[flip, :, -1] = -U[flip, :, -1]
    W[N:] = (U @ Vt).reshape(N * d, d)
    return W, B, sigma


def staircase(M, X, d, r_max=None, eta=1e-3, precondition_on=True, **opts):
    """The loop above, without the polish.  Returns a dict: outcome, final_rank, levels (one dict per level: rank, F_in, F,
    grad, iterations, products, lambda_min, alpha, halvings), Y, F_sdp, lambda_min, Xhat, B, sigma, F_rounded."""
    r_max = 2 * d if r_max is None else r_max
    T = cert.block_jacobi(M, d) if precondition_on else None
    Y = np.array(X, dtype=np.float64)
    F = objective(M, Y)
    levels = []
    outcome = SADDLE
    while True:
        r = Y.shape[1]
        F_in = F
        Y, F, gn, its, prods = tnt_level(M, Y, d, T, **opts)
        lam, x = min_eigenpair(M, Y, d)
        levels.append(dict(rank=r, F_in=F_in, F=F, grad=gn, iterations=its, products=prods, lambda_min=lam, alpha=0.0, halvings=0))
        if lam >= -0.5 * eta:
            outcome = SOLVED
            break
        if r == r_max:
            outcome = MAX_RANK
            break
        Y1 = np.hstack([Y, np.zeros((Y.shape[0], 1))])
        Yd = np.zeros_like(Y1)
        Yd[:, -1] = x
        alpha, accepted = 1.0, False
        for _ in range(30):
            Z = retract(Y1, alpha * Yd, d)
            FZ = objective(M, Z)
            if FZ <= F + 0.25 * alpha * alpha * lam:
                accepted = True
                break
            alpha *= 0.5
            levels[-1]["halvings"] += 1
        if not accepted:
            break
        levels[-1]["alpha"] = alpha
        Y, F = Z, FZ
    Xhat, B, sigma = round_solution(Y, d) if Y.shape[1] > d else (Y.copy(), np.eye(d), round_solution(Y, d)[2])
    return dict(outcome=outcome, final_rank=Y.shape[1], levels=levels, Y=Y, F_sdp=F, lambda_min=levels[-1]["lambda_min"],
                Xhat=Xhat, B=B, sigma=sigma, F_rounded=objective(M, Xhat))


def lift(X, d):
    """(d+1)N x 2d with zero columns behind X's."""
    out = np.zeros((X.shape[0], 2 * d), order="F")
    out[:, :X.shape[1]] = X
    return out


def random_lifted_point(rng, N, d, r):
    """A feasible point at rank r in the 2d-column layout."""
    X = np.zeros(((d + 1) * N, 2 * d), order="F")
    X[:N, :r] = rng.standard_normal((N, r))
    Q = np.linalg.qr(rng.standard_normal((N, r, d)))[0]        # (N, r, d), orthonormal columns
    X[N:, :r] = Q.transpose(0, 2, 1).reshape(N * d, r)
    return X


def weak_duality_interval(M, Y, d, Xnorm2):
    """(lower, upper, lambda_min, err) for the optimum F* of the rank-d problem from the restated S = S(Y): every feasible X
    has F(X) >= 1/2 sum tr Lambda_p + 1/2 min(lambda_min, 0) |X|_F^2, and F(Y) = 1/2 sum tr Lambda_p + 1/2 <Y, S Y>.  Xnorm2: a
    bound on |X|_F^2 of the feasible points compared.  err: what the two ends carry of their own evaluation in fp64 -- both
    are sums of products of Y with M Y, whose entries are sums of the terms of |M| |Y| -- 4 u |Y|_F | |M| |Y| |_F."""
    Lam = lambda_blocks(M, Y, d)
    S = S_matrix(M, Y, d)
    lam = float(np.linalg.eigvalsh(S.toarray())[0])
    base = 0.5 * float(np.trace(Lam, axis1=1, axis2=2).sum())
    err = 4 * 2.0 ** -53 * float(np.linalg.norm(Y)) * float(np.linalg.norm(abs(sp.csr_matrix(M)) @ np.abs(Y)))
    return base + 0.5 * min(lam, 0.0) * Xnorm2, base + 0.5 * float(np.sum(Y * (S @ Y))), lam, err
