"""Restatement of the joint marginals of a pose set (dpgo_amd/csrc/marg.h, marg_math.h): test infrastructure in the style of
tests/pairs_restatement.py, whose Jacobian, margins and dtype convention it uses.  Plain numpy; nothing of the library is
imported here.  np.float64 is "what ordinary fp64 reaches", np.longdouble the reference.

keep: K distinct global poses, in LIST order; every output follows that order.
  absolute form   cov = (A^-1)_KK of the anchored restated Hessian A (tests/cov_restatement.py), n = dof K.  Its inverse is the
                  Schur complement A_KK - A_KM A_MM^-1 A_MK (M: every other unknown), computed here directly.
  relative form   base in keep: cov = J Sigma_KK J^T, n = dof (K - 1); row block k of J (the kept poses other than the base, in
                  list order) holds pairs_restatement.jacobian(base, k)'s J_p on the base's columns and J_q on k's; the anchor's
                  blocks of Sigma_KK are zeros.
  info = cov^-1, logdet = log det cov, both through the long-double Cholesky of tests/factor_restatement.py.

The bounds (u = 2^-53, C = cov_restatement.C), fixed here before any device is asked; nothing in them comes from the device.
With B the entrywise bound of cov's error (bSigma 11^T in the absolute form, m_rel in the relative form), eps = |B|_2 >= |E|_2
for every E with |E| <= B entrywise -- n bSigma in the absolute form -- Lambda = cov^-1 and rho = eps |Lambda|_2 (a test asserts
rho <= 0.1 on its inputs: that is a condition that keeps the first-order bound honest, not a tolerance):
  cov, absolute   bSigma entrywise (tests/test_gpu_covariance.py's formula; an input here).
  cov, relative   m_rel = |J| B |J|^T + EJ |Sigma| |J|^T + |J| |Sigma| EJ^T + (4 dof + 2) u |J| |Sigma| |J|^T, B = bSigma off the
                  anchor's rows and columns: pairs_restatement.margin_rel on the set's J.  A row of J has at most 2 dof non-zeros
                  and an entry of a four-term block is two chained sums of at most 2 dof products each, as for a pair -- the
                  four terms are the four block products of |J| |Sigma| |J|^T -- so the count (4 dof + 2) u carries over.
  info            C u kappa_2(cov) |Lambda|_2 + |Lambda|_2^2 eps / (1 - rho): the inversion's own error, and
                  (cov + E)^-1 - cov^-1 with |E|_2 <= eps.
  logdet          n rho / (1 - rho) for E (every eigenvalue of cov^-1 (cov + E) lies in [1 - rho, 1 + rho], and
                  |log(1 - rho)| <= rho / (1 - rho)), plus the factorisation's own term: n rho_f / (1 - rho_f) with
                  rho_f = C u kappa_2(cov) for its backward error, and (n + 8) u sum |log W_ii| for the logarithms (one ulp),
                  the reciprocal pivots (relative error 2 u under a logarithm) and the sum of n terms.
"""
import numpy as np

import cov_restatement as cr
import factor_restatement as fr
import pairs_restatement as pr
import solve_restatement as sr

LD, U, C = cr.LD, cr.U, cr.C


def unknowns(dof, poses):
    return np.concatenate([np.arange(dof * int(g), dof * int(g) + dof) for g in poses]) if len(poses) else np.zeros(0, int)


def columns_ld(A, dof, poses, L=None):
    """The columns of A^-1 that belong to `poses` (ascending unknowns of each), long double: (n x dof len(poses))."""
    if L is None:
        L, kstar, _ = fr.cholesky_ld(A)
        assert kstar < 0
    cols = unknowns(dof, poses)
    E = np.zeros((A.shape[0], len(cols)))
    E[cols, np.arange(len(cols))] = 1.0
    return sr.solve_cholesky_ld(A, E, L)


def sigma_kk(A, dof, keep, anchor, L=None):
    """Sigma_KK in list order, long double, the anchor's blocks exact zeros."""
    S = np.array(columns_ld(A, dof, keep, L)[unknowns(dof, keep)], LD)
    return zero_anchor(S, dof, keep, anchor)


def zero_anchor(S, dof, keep, anchor):
    S = np.array(S)
    for i, g in enumerate(keep):
        if int(g) == anchor:
            S[dof * i:dof * i + dof, :] = 0
            S[:, dof * i:dof * i + dof] = 0
    return S


def sigma_from_dense(Sigma, dof, keep, anchor):
    """The same out of a dense inverse on the unknowns dof g + a (any dtype)."""
    idx = unknowns(dof, keep)
    return zero_anchor(Sigma[np.ix_(idx, idx)], dof, keep, anchor)


def schur(A, dof, keep):
    """A_KK - A_KM A_MM^-1 A_MK in long double, K in list order, M every other unknown (the anchor's identity block among them)."""
    k = unknowns(dof, keep)
    m = np.setdiff1d(np.arange(A.shape[0]), k)
    Amm = np.asarray(A[np.ix_(m, m)], np.float64)
    L, kstar, _ = fr.cholesky_ld(Amm)
    assert kstar < 0
    Z = sr.solve_cholesky_ld(Amm, np.asarray(A[np.ix_(m, k)], np.float64), L)
    return np.asarray(A[np.ix_(k, k)], LD) - np.asarray(A[np.ix_(k, m)], LD) @ Z


def others(keep, base):
    return [int(g) for g in keep if int(g) != base]


def jacobian_set(X, d, keep, base, dtype=np.float64, error=False):
    """J (dof (K - 1) x dof K); error=True: EJ of pairs_restatement.jacobian_error in the same places."""
    dof = cr.dof_of(d)
    keep = [int(g) for g in keep]
    b = keep.index(base)
    J = np.zeros((dof * (len(keep) - 1), dof * len(keep)), np.float64 if error else dtype)
    for ko, g in enumerate(others(keep, base)):
        k = keep.index(g)
        Jp = pr.jacobian_error(X, d, base, g)[0] if error else pr.jacobian(X, d, base, g, dtype)
        J[dof * ko:dof * ko + dof, dof * b:dof * b + dof] = Jp[:, :dof]
        J[dof * ko:dof * ko + dof, dof * k:dof * k + dof] = Jp[:, dof:]
    return J


def rel_cov(J, S):
    return J @ S @ J.T


def inverse_ld(Cm):
    """(Cm^-1, log det Cm, sum |log L_ii|) through the long-double Cholesky of the symmetrised matrix."""
    Cm = np.asarray(Cm, LD)
    L, kstar, _ = fr.cholesky_ld(np.asarray((Cm + Cm.T) / 2, LD))
    assert kstar < 0
    Li = fr.lower_inverse_ld(L)
    lg = np.log(np.diag(np.asarray(L, LD)))
    return Li.T @ Li, 2 * lg.sum(), float(np.abs(lg).sum())


def anchor_mask(dof, keep, anchor, bS):
    B = np.full((dof * len(keep), dof * len(keep)), float(bS))
    return zero_anchor(B, dof, keep, anchor)


def margin_rel(X, d, keep, base, anchor, S64, bS):
    dof = cr.dof_of(d)
    J = np.abs(jacobian_set(X, d, keep, base))
    EJ = jacobian_set(X, d, keep, base, error=True)
    Sa = np.abs(np.asarray(S64, np.float64))
    return J @ anchor_mask(dof, keep, anchor, bS) @ J.T + EJ @ Sa @ J.T + J @ Sa @ EJ.T + (4 * dof + 2) * U * (J @ Sa @ J.T)


def spectrum(cov_ld):
    lam = np.linalg.eigvalsh(np.asarray((cov_ld + cov_ld.T) / 2, np.float64))
    assert lam[0] > 0
    return float(lam[-1] / lam[0]), float(1 / lam[0])   # kappa_2(cov), |Lambda|_2


def eps_of(cov_ld, B):
    """|B|_2 of the entrywise bound B (a matrix, or a scalar standing for B 11^T: n B)."""
    return cov_ld.shape[0] * float(B) if np.ndim(B) == 0 else float(np.linalg.norm(np.asarray(B, np.float64), 2))


def rho_of(cov_ld, B):
    return eps_of(cov_ld, B) * spectrum(cov_ld)[1]


def info_bound(cov_ld, B):
    kappa, nl = spectrum(cov_ld)
    eps = eps_of(cov_ld, B)
    return C * U * kappa * nl + nl * nl * eps / (1 - eps * nl)


def logdet_bound(cov_ld, B, sum_abs_log):
    n = cov_ld.shape[0]
    kappa, nl = spectrum(cov_ld)
    rho, rho_f = eps_of(cov_ld, B) * nl, C * U * kappa
    return n * rho / (1 - rho) + n * rho_f / (1 - rho_f) + (n + 8) * U * sum_abs_log


# ---------------------------------------------------------------------------------------------------------------
# the device's arithmetic in numpy fp64, block by block, with the mistakes a kernel could make
# ---------------------------------------------------------------------------------------------------------------
MUTANTS = ("transposed_block", "dropped_term", "wrong_base_column", "ascending_order", "upper_source_block", "hat_sign")


def absolute_fp64(Sigma64, dof, keep, anchor, mutant=None):
    """Sigma_KK of the absolute form out of a dense fp64 inverse; ascending_order: the blocks by ascending pose, not by the list."""
    order = sorted(int(g) for g in keep) if mutant == "ascending_order" else keep
    return sigma_from_dense(Sigma64, dof, order, anchor)


def relative_fp64(X, d, keep, base, S64, mutant=None):
    """The relative covariance from Sigma_KK (fp64, list order) as marg_math.h computes it: block (k, l), k >= l, from the
    four terms, block (l, k) its transpose.  Mutants: transposed_block -- block (l, k) written untransposed; dropped_term --
    A_k S_bl B_l^T left out; wrong_base_column -- S_bb's columns taken at the pose after the base in the list;
    upper_source_block -- S_kb read as the stored block S_bk, untransposed; hat_sign -- hat(t_bk) with the other sign."""
    dof = cr.dof_of(d)
    keep = [int(g) for g in keep]
    b = keep.index(base)
    oth = others(keep, base)
    n = dof * len(oth)
    out = np.zeros((n, n))

    def blk(i, j):
        return S64[dof * i:dof * i + dof, dof * j:dof * j + dof]

    def AB(g):
        J = pr.jacobian(X, d, base, g)
        if mutant == "hat_sign":
            J[:d, d:dof] = -J[:d, d:dof]
        return J[:, :dof], J[:, dof:]

    bc = (b + 1) % len(keep) if mutant == "wrong_base_column" else b
    for ko, gk in enumerate(oth):
        k = keep.index(gk)
        Ak, Bk = AB(gk)
        for lo in range(ko + 1):
            l = keep.index(oth[lo])
            Al, Bl = AB(oth[lo])
            Skb = blk(b, k) if mutant == "upper_source_block" else blk(k, b)
            T = Ak @ blk(b, bc) @ Al.T + Bk @ Skb @ Al.T + Bk @ blk(k, l) @ Bl.T
            if mutant != "dropped_term":
                T = T + Ak @ blk(b, l) @ Bl.T
            if ko == lo:
                T = np.tril(T) + np.tril(T, -1).T
            out[dof * ko:dof * ko + dof, dof * lo:dof * lo + dof] = T
            out[dof * lo:dof * lo + dof, dof * ko:dof * ko + dof] = T if (mutant == "transposed_block" and ko != lo) else T.T
    return out
