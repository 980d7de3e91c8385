"""Restatement of the measurement sensitivities (dpgo_amd/csrc/sens.h, sens_math.h): test infrastructure in the style of
tests/pairs_restatement.py, whose layout and hat map it uses.  Plain numpy; nothing of the library is imported here.  Every
function takes a dtype: np.float64 is "what ordinary fp64 reaches", np.longdouble the reference.

A problem is robust_restatement's dict(d, N, I, J, R, t, kappa, tau, ...); X is in the reference layout (row p the translation,
rows N + d p ... the rows of Y_p = R_p^T); an adjoint lam is (dof N,) or (dof N, k) by global pose in cov.h's coordinates
(dt in the world frame, R <- R Exp(hat(omega))).

Edge e = (i, j) with theta_e = (kappa, tau, t~, R~):   a = t_j - t_i - R_i t~,   B = R_j - R_i R~,
    1/2 s_e = 1/2 tau |a|^2 + 1/2 kappa |B|_F^2
    da = dt_j - dt_i - R_i hat(omega_i) t~,     dB = R_j hat(omega_j) - R_i hat(omega_i) R~
    phi_e(lam; theta_e) = D_lam (1/2 s_e) = tau a^T da + kappa <B, dB>
and dL/dtheta_e = -d phi_e / d theta_e with kappa + dkappa, tau + dtau, t~ + dt~ and R~ <- R~ Exp(hat(eta)):
    d phi/d tau = a^T da        d phi/d t~    = -tau (R_i^T da - hat(omega_i) R_i^T a)
    d phi/d kappa = <B, dB>     d phi/d eta_k = -kappa <hat(e_k), R~^T (R_i^T dB - hat(omega_i) R_i^T B)>
tests/test_sens_host.py holds these closed forms against central differences of lam^T g (newton_restatement.grad) in theta:
that, not this paragraph, is the judge of signs and frames.

The margin (u = 2^-53), fixed here before any device is asked, to first order in u.  Every output is a polynomial in the
records, the measurement and lam, evaluated by nested sums of products.  The longest path from an input to an output (the eta
entries) has 4 d + 5 roundings: B^T or hat(omega) Y (d + 1 resp. 2 and, behind R~^T, d + 1 more), the product with Y_i (d), the hat
(2) resp. nothing, one subtraction, the two sums of d products over R~ (2 d), the weight (1).  So with T the same expression on
the magnitudes of every operand and with every subtraction an addition (the sum of the magnitudes of the terms),
    |fl(out) - out| <= (4 d + 6) u T(|lam|)          (one rounding more for what first order leaves out)
and, every output being linear in lam, an entrywise error of at most b in lam moves it by at most T(1) b.
margin_sens = (4 d + 6) u T(|lam|) + T(1) b.
"""
import numpy as np

import cov_restatement as cr
import pairs_restatement as pr

LD = pr.LD
U = pr.U


def dof_of(d):
    return cr.dof_of(d)


def _hat(w, d, dtype, absolute):
    """(..., d, d) from (..., dof - d); absolute: every entry's magnitude."""
    w = np.asarray(w, dtype)
    out = np.zeros(w.shape[:-1] + (d, d), dtype)
    s = 1 if absolute else -1
    if d == 2:
        out[..., 0, 1] = s * w[..., 0]
        out[..., 1, 0] = w[..., 0]
    else:
        out[..., 0, 1], out[..., 0, 2] = s * w[..., 2], w[..., 1]
        out[..., 1, 0], out[..., 1, 2] = w[..., 2], s * w[..., 0]
        out[..., 2, 0], out[..., 2, 1] = s * w[..., 1], w[..., 0]
    return out


def _mm(A, B):
    """A @ B on the last two axes by explicit sums (long double has no BLAS and no einsum)."""
    out = 0
    for k in range(A.shape[-1]):
        out = out + A[..., :, k, None] * B[..., None, k, :]
    return out


def _mv(A, v):
    return _mm(A, v[..., None])[..., 0]


def _T(A):
    return np.swapaxes(A, -1, -2)


def _evaluate(P, X, lam, dtype, absolute):
    """(sens (m, k, 2 + dof), phi (m, k)).  absolute: the sums of the magnitudes of the terms."""
    d, N = P["d"], P["N"]
    dof = dof_of(d)
    X = np.asarray(X, dtype)
    lam = np.asarray(lam, dtype).reshape(dof * N, -1)
    I, J = np.asarray(P["I"]), np.asarray(P["J"])
    Rt, tt = np.asarray(P["R"], dtype), np.asarray(P["t"], dtype)
    kappa, tau = np.asarray(P["kappa"], dtype)[:, None], np.asarray(P["tau"], dtype)[:, None]
    if absolute:
        X, lam, Rt, tt = np.abs(X), np.abs(lam), np.abs(Rt), np.abs(tt)
    sub = (lambda a, b: a + b) if absolute else (lambda a, b: a - b)
    Y = X[N:].reshape(N, d, d)
    Ri, Rj, ti, tj = _T(Y[I]), _T(Y[J]), X[I], X[J]                      # (m, d, d), (m, d)
    L = lam.reshape(N, dof, -1)
    li, lj = np.moveaxis(L[I], 2, 1), np.moveaxis(L[J], 2, 1)            # (m, k, dof)
    Wi, Wj = _hat(li[..., d:], d, dtype, absolute), _hat(lj[..., d:], d, dtype, absolute)   # (m, k, d, d)
    Ri_, Rj_, Rt_ = Ri[:, None], Rj[:, None], Rt[:, None]
    a = sub(sub(tj, ti), _mv(Ri, tt))[:, None]                           # (m, 1, d)
    da = sub(sub(lj[..., :d], li[..., :d]), _mv(Ri_, _mv(Wi, tt[:, None])))
    B = sub(Rj, _mm(Ri, Rt))[:, None]
    dB = sub(_mm(Rj_, Wj), _mm(Ri_, _mm(Wi, Rt_)))
    p_tau = np.sum(a * da, axis=-1)
    p_kappa = np.sum(np.sum(B * dB, axis=-1), axis=-1)
    p_t = tau[..., None] * sub(_mv(_T(Ri_), da), _mv(Wi, _mv(_T(Ri_), a)))
    Z = _mm(_T(Rt_), sub(_mm(_T(Ri_), dB), _mm(Wi, _mm(_T(Ri_), B))))
    if d == 2:
        p_eta = np.stack([sub(Z[..., 1, 0], Z[..., 0, 1])], axis=-1)
    else:
        p_eta = np.stack([sub(Z[..., 2, 1], Z[..., 1, 2]), sub(Z[..., 0, 2], Z[..., 2, 0]), sub(Z[..., 1, 0], Z[..., 0, 1])], axis=-1)
    p_eta = kappa[..., None] * p_eta
    s = 1 if absolute else -1
    # d phi/d t~ and d phi/d eta carry a minus sign of their own: the sensitivities are minus the derivatives of phi
    sens = np.concatenate([(s * p_kappa)[..., None], (s * p_tau)[..., None], p_t, p_eta], axis=-1)
    phi = tau * p_tau + kappa * p_kappa
    return sens, phi


def _shape(out, lam):
    return out[:, 0] if np.ndim(lam) == 1 else out


def sens_edge(P, X, lam, dtype=np.float64):
    """dL/d(kappa, tau, t~, eta) of every edge for the adjoint(s) lam: (m, 2 + dof), or (m, k, 2 + dof) for lam (dof N, k)."""
    return _shape(_evaluate(P, X, lam, dtype, False)[0], lam)


def phi(P, X, lam, dtype=np.float64):
    """phi_e = lam_i' ghat_e(i) + lam_j' ghat_e(j) of every edge: (m,) or (m, k)."""
    return _shape(_evaluate(P, X, lam, dtype, False)[1], lam)


def rounding_count(d):
    return 4 * d + 6


def margin_sens(P, X, lam, b_lam=0.0):
    """The entrywise bound of the module docstring on the fp64 evaluation of sens_edge, lam known to within b_lam entrywise
    (a number, or one per column of lam)."""
    T = _evaluate(P, X, lam, np.float64, True)[0]
    T1 = _evaluate(P, X, np.ones(np.shape(lam)), np.float64, True)[0]
    b = np.broadcast_to(np.asarray(b_lam, np.float64), (T.shape[1],))
    return _shape(rounding_count(P["d"]) * U * T + b[None, :, None] * T1, lam)


def perturbed(P, e, param, h, dtype=LD):
    """The problem with parameter `param` of edge e moved by h: 0 kappa, 1 tau, 2 ... 2 + d - 1 the entries of t~, then eta_k
    (R~ <- R~ Exp(hat(h e_k)))."""
    d = P["d"]
    Q = dict(P, R=np.array(P["R"], dtype), t=np.array(P["t"], dtype), kappa=np.array(P["kappa"], dtype), tau=np.array(P["tau"], dtype))
    h = dtype(h)
    if param == 0:
        Q["kappa"][e] += h
    elif param == 1:
        Q["tau"][e] += h
    elif param < 2 + d:
        Q["t"][e, param - 2] += h
    else:
        w = np.zeros(dof_of(d) - d, dtype)
        w[param - 2 - d] = h
        Q["R"][e] = np.asarray(Q["R"][e], dtype) @ np.asarray(pr.exp_so(w, d, LD), dtype)
    return Q
