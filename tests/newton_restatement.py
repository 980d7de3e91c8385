"""Restatement of the Newton polish (dpgo_amd/csrc/polish.h): test infrastructure, like tests/cov_restatement.py and
tests/cert_restatement.py, which it imports.  Plain numpy / scipy; nothing of the library is imported here.

Damped Riemannian Newton steps (Levenberg-Marquardt on the anchored tangent-space Hessian H of cov_restatement.hessian) with
a dense Cholesky factorisation:

    mu = 0
    for k = 0 ... max_steps:
        g, |g|, F0, H, hmax at X                     (hmax: the largest diagonal entry of H over the non-anchor unknowns)
        |g| <= (grad_tol > 0 ? grad_tol : rel_tol hmax)   -> CONVERGED
        k == max_steps                                     -> MAX_STEPS
        at most max_tries times:
            factor H + mu I (non-anchor diagonal);  not positive definite: indefinite += 1 if mu == 0,
                                                    mu = max(10 mu, 1e-3 hmax), next try
            delta = -(H + mu I)^-1 g,  Z = retract(X, delta),  F1 = F(Z)
            pred = -1/2 g'delta + 1/2 mu |delta|^2,  rho = pred > 0 ? (F0 - F1) / pred : -1
            accept if rho >= 0.1 or |F0 - F1| <= 1e-13 |F0|:   X = Z;  rho > 0.75: mu /= 10, and mu = 0 once mu < 1e-8 hmax
            else mu = max(10 mu, 1e-3 hmax)
        no try accepted -> STALLED
"""
import numpy as np
import scipy.linalg as sla

import cert_restatement as cert
import cov_restatement as cr

CONVERGED, MAX_STEPS, STALLED, SKIPPED = 0, 1, 2, 3
DEFAULTS = dict(max_steps=20, max_tries=8, rel_tol=1e-9, grad_tol=0.0)


def objective(M, X):
    """F = 1/2 <X, M X>."""
    return 0.5 * float(np.sum(X * (M @ X)))


def grad(M, X, d, anchor=None):
    """g[dof p + a] = tr(E_a(p)^T (M X)_p) in cov_restatement's basis; the anchor's dof entries are zero."""
    MX = M @ X
    J = cr.tangent_basis(X, d)
    g = sum(J[c].T @ MX[:, c] for c in range(d))
    if anchor is not None:
        dof = cr.dof_of(d)
        g[dof * anchor:dof * anchor + dof] = 0.0
    return g


def anchored_hessian(M, X, d, anchor):
    return cr.anchored(cr.hessian(cert.S_matrix(M, X, d), X, d), anchor, cr.dof_of(d))


def hmax_of(H, anchor, dof):
    diag = np.array(np.diag(H))
    diag[dof * anchor:dof * anchor + dof] = -np.inf
    return float(diag.max())


def retract(X, delta, d, anchor):
    """cov_restatement.retract, the anchor's record copied bit for bit."""
    N = X.shape[0] // (d + 1)
    Z = cr.retract(X, delta, d)
    Z[anchor] = X[anchor]
    Z[N + d * anchor:N + d * anchor + d] = X[N + d * anchor:N + d * anchor + d]
    return Z


def polish(M, X, d, anchor=0, max_steps=20, max_tries=8, rel_tol=1e-9, grad_tol=0.0):
    """Returns (X, outcome, steps, factorisations, indefinite, log); log: one row per iteration k of
    (F0, |g|, mu at entry, rho of the accepted try, tries), the last row that of the iteration that ended the run."""
    out = polish_full(M, X, d, anchor, max_steps, max_tries, rel_tol, grad_tol)
    return out["X"], out["outcome"], out["steps"], out["factorisations"], out["indefinite"], out["log"]


def polish_full(M, X, d, anchor=0, max_steps=20, max_tries=8, rel_tol=1e-9, grad_tol=0.0):
    """polish() with everything the result struct of the library carries: hmax, mu_final, F / grad initial and final, and
    `rounding`: per iteration whether the accepted try was taken under the rounding clause."""
    dof = cr.dof_of(d)
    X = np.array(X, dtype=np.float64)
    n = dof * (X.shape[0] // (d + 1))
    free = np.ones(n, bool)
    free[dof * anchor:dof * anchor + dof] = False
    mu = 0.0
    steps = factorisations = indefinite = 0
    log, rounding = [], []
    outcome = STALLED
    F_initial = grad_initial = None
    for k in range(max_steps + 1):
        g = grad(M, X, d, anchor)
        gn = float(np.linalg.norm(g))
        F0 = objective(M, X)
        H = anchored_hessian(M, X, d, anchor)
        hmax = hmax_of(H, anchor, dof)
        if k == 0:
            F_initial, grad_initial = F0, gn
        mu_in = mu
        if gn <= (grad_tol if grad_tol > 0 else rel_tol * hmax):
            outcome = CONVERGED
            log.append((F0, gn, mu_in, 0.0, 0))
            rounding.append(False)
            break
        if k == max_steps:
            outcome = MAX_STEPS
            log.append((F0, gn, mu_in, 0.0, 0))
            rounding.append(False)
            break
        accepted = False
        tries = 0
        rho = 0.0
        for _ in range(max_tries):
            tries += 1
            A = H + mu * np.diag(free.astype(np.float64))
            factorisations += 1
            try:
                L = np.linalg.cholesky(A)
            except np.linalg.LinAlgError:
                if mu == 0.0:
                    indefinite += 1
                mu = max(10.0 * mu, 1e-3 * hmax)
                continue
            delta = -sla.cho_solve((L, True), g)
            Z = retract(X, delta, d, anchor)
            F1 = objective(M, Z)
            pred = -0.5 * float(g @ delta) + 0.5 * mu * float(delta @ delta)
            rho = (F0 - F1) / pred if pred > 0 else -1.0
            by_rounding = abs(F0 - F1) <= 1e-13 * abs(F0)
            if rho >= 0.1 or by_rounding:
                X = Z
                accepted = True
                steps += 1
                rounding.append(bool(by_rounding and not rho >= 0.1))
                if rho > 0.75:
                    mu = mu / 10.0
                    if mu < 1e-8 * hmax:
                        mu = 0.0
                break
            mu = max(10.0 * mu, 1e-3 * hmax)
        log.append((F0, gn, mu_in, rho if accepted else 0.0, tries))
        if not accepted:
            rounding.append(False)
            break
    log = np.array(log, dtype=np.float64).reshape(-1, 5)
    return dict(X=X, outcome=outcome, steps=steps, factorisations=factorisations, indefinite=indefinite, log=log,
                rounding=rounding, hmax=hmax, mu_final=mu, F_initial=F_initial, F_final=float(log[-1, 0]),
                grad_initial=grad_initial, grad_final=float(log[-1, 1]))
