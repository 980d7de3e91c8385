"""Restatement of the candidate sets (dpgo_amd/csrc/cand.h, cand_math.h): test infrastructure in the style of
tests/marg_restatement.py, whose Sigma_KK, margins and dtype convention it uses.  Plain numpy; nothing of the library is imported
here.  np.float64 is "what ordinary fp64 reaches", np.longdouble the reference.

pairs (m, 2): the candidates' end poses, p != q.  K: the distinct ends in order of first appearance; kpos (m, 2) their positions
in K.  n = dof m.
  J          (n x dof |K|): row block i holds pairs_restatement.jacobian(p_i, q_i)'s J_p on p_i's columns and J_q on q_i's
  cov        J Sigma_KK J^T, the anchor's blocks of Sigma_KK zeros
  S          cov + blkdiag(Omega_i^-1), Omega_i = blkdiag(tau_i I_d, 2 kappa_i I_{dof - d}); r stacks pairs_restatement.residual
  joint      S^-1, log det S, d2_joint = r^T S^-1 r, gain_all = 1/2 (log det S - sum_i log det Omega_i^-1)
  greedy     at every step, for every candidate not yet chosen, the conditional covariance C_i and residual rho_i given the
             chosen set -- by the RIGHT-looking Schur complement W <- W - W[:, s] W_ss^-1 W[s, :] on the whole matrix, which is
             not how the device gets them (left-looking panels) -- gain_i = 1/2 (log det C_i - log det Omega_i^-1),
             d2_i = rho_i^T C_i^-1 rho_i; eligible iff C_i is positive definite and (d2_max <= 0 or d2_i <= d2_max); the
             eligible candidate of the largest gain is chosen, ties to the lowest index; the loop stops where none is eligible.

The bounds (u = 2^-53, C = cov_restatement.C), fixed here before any device is asked; nothing in them comes from the device.
  cov        marg_restatement.margin_rel's formula on the candidates' J: |J| B |J|^T + EJ |Sigma| |J|^T + |J| |Sigma| EJ^T +
             (4 dof + 2) u |J| |Sigma| |J|^T, B = bSigma off the anchor's rows and columns.  A row of J has at most 2 dof
             non-zeros and an entry of a four-term block is two chained sums of at most 2 dof products, as for a pair.
  S          cov's bound + u |S| (the one add) + u Omega^-1 (the reciprocal) on the diagonal: bound_S.
  S^-1, logdet   marg_restatement.info_bound / logdet_bound with B = bound_S, under the same condition rho <= 0.1, which the
             tests assert on their inputs.  gain_all: half the logdet bound plus omega_log_bound.
  d2_joint   2 |S^-1 r|^T m_r + bI (sum |r|)^2 + 2 (n + 2) u |r|^T |S^-1| |r|: the residual's error, the inverse's entrywise
             bound bI, and the two chained sums of k_cand_quad.
  selection  The device's block Cholesky after t steps (k = dof (t + 1) + 2 terms in every chain, each an fma, with a division and
             a square root at the end: gamma_t = 2 k u) computes the EXACT conditional quantities of a perturbed input S + dS,
             |dS_ab| <= gamma_t sqrt(S_aa S_bb) (Higham, Accuracy and Stability, thm 10.3 with |L| |L^T|_ab <= sqrt(S_aa S_bb)),
             and r + dr, |dr_a| <= gamma_t sqrt(S_aa) sqrt(d2_total) (the same theorem on the matrix bordered by r, whose last
             pivot is d2).  With E = |dS|_2 + the input's own bound, e_r likewise, G_i = S_sel^-1 S_sel,i, y = S_sel^-1 r_sel and
             rho_S = E |S_sel^-1|_2 (asserted <= 0.1), first-order perturbation of a Schur complement gives
                 |dC_i|_2   <= (1 + |G_i|_2)^2 E / (1 - rho_S)                                  =: eC_i
                 |drho_i|_2 <= (1 + |G_i|_2) (e_r + E |y|_2) / (1 - rho_S)                      =: eR_i
             and then, with z = C_i^-1 rho_i, rho_i' = eC_i |C_i^-1|_2 (asserted <= 0.1):
                 gain_i     1/2 [dof rho_i' / (1 - rho_i') + dof rho_f / (1 - rho_f) + (dof + 8) u sum |log L_jj|] +
                            omega_log_bound, rho_f = C u kappa_2(C_i): marg_restatement.logdet_bound's three terms on C_i
                 d2_i       [2 |z|_2 eR_i + |z|_2^2 eC_i] / (1 - rho_i') + 4 (dof + 1) u kappa_2(C_i) d2_i:
                            pairs_restatement.margin_d2's terms in the 2-norm.
  condition, not tolerance: on every selection input the restated gap between the best and the second-best eligible gain at
             every step exceeds GAP_FACTOR times the sum of their two bounds, and every candidate's d2_i is further than
             GAP_FACTOR times its bound from d2_max (check_decisions).  A deliberately exact tie (a duplicated candidate, whose
             rows of S are bit-equal) is the one exception and must resolve to the lower index.
"""
import numpy as np

import cov_restatement as cr
import factor_restatement as fr
import marg_restatement as mr
import pairs_restatement as pr

LD, U, C = cr.LD, cr.U, cr.C
GAP_FACTOR = 4.0


def pose_list(pairs):
    K, kpos = [], []
    for g in np.asarray(pairs).reshape(-1):
        g = int(g)
        if g not in K:
            K.append(g)
        kpos.append(K.index(g))
    return K, np.asarray(kpos, int).reshape(-1, 2)


def jacobian_cand(X, d, pairs, K, dtype=np.float64, error=False):
    """J (dof m x dof |K|); error=True: EJ of pairs_restatement.jacobian_error in the same places."""
    dof = cr.dof_of(d)
    pairs = np.asarray(pairs).reshape(-1, 2)
    J = np.zeros((dof * len(pairs), dof * len(K)), np.float64 if error else dtype)
    for i, (p, q) in enumerate(pairs):
        p, q = int(p), int(q)
        Jp = pr.jacobian_error(X, d, p, q)[0] if error else pr.jacobian(X, d, p, q, dtype)
        kp, kq = K.index(p), K.index(q)
        J[dof * i:dof * i + dof, dof * kp:dof * kp + dof] = Jp[:, :dof]
        J[dof * i:dof * i + dof, dof * kq:dof * kq + dof] = Jp[:, dof:]
    return J


def omega_inv(d, kappa, tau, dtype=np.float64):
    """The diagonal of blkdiag(Omega_i^-1), (dof m,)."""
    dof = cr.dof_of(d)
    kappa, tau = np.asarray(kappa, dtype).reshape(-1), np.asarray(tau, dtype).reshape(-1)
    one = np.asarray(1, dtype)
    return np.concatenate([np.concatenate([np.repeat(one / tau[i], d), np.repeat(one / (2 * kappa[i]), dof - d)])
                           for i in range(len(kappa))])


def logdet_omega_inv(d, kappa, tau, dtype=LD):
    """(m,): log det Omega_i^-1."""
    dof = cr.dof_of(d)
    w = np.log(omega_inv(d, kappa, tau, dtype)).reshape(-1, dof)
    return w.sum(axis=1)


def omega_log_bound(d, kappa, tau):
    """Per candidate: the reciprocals (u relative, so u under a logarithm), the logarithms (one ulp) and the dof - 1 adds."""
    dof = cr.dof_of(d)
    w = np.abs(np.log(omega_inv(d, kappa, tau, np.float64))).reshape(-1, dof)
    return (dof + 4) * U * w.sum(axis=1) + 2 * dof * U


def cov_of(J, S):
    return J @ S @ J.T


def innovation(cov, d, kappa, tau, dtype=np.float64):
    return np.asarray(cov, dtype) + np.diag(omega_inv(d, kappa, tau, dtype))


def residuals(X, d, pairs, cands, dtype=np.float64):
    """cands: a list of (R~, t~, kappa, tau)."""
    return np.concatenate([pr.residual(X, d, int(p), int(q), cands[i], dtype) for i, (p, q) in enumerate(np.asarray(pairs).reshape(-1, 2))])


def margin_cov(X, d, pairs, K, anchor, S64, bS):
    dof = cr.dof_of(d)
    J = np.abs(jacobian_cand(X, d, pairs, K))
    EJ = jacobian_cand(X, d, pairs, K, error=True)
    Sa = np.abs(np.asarray(S64, np.float64))
    return J @ mr.anchor_mask(dof, K, anchor, bS) @ J.T + EJ @ Sa @ J.T + J @ Sa @ EJ.T + (4 * dof + 2) * U * (J @ Sa @ J.T)


def bound_S(m_cov, S64, d, kappa, tau):
    return m_cov + U * np.abs(np.asarray(S64, np.float64)) + U * np.diag(omega_inv(d, kappa, tau))


def margin_residuals(X, d, pairs, cands):
    return np.concatenate([pr.margin_residual(X, d, int(p), int(q), cands[i]) for i, (p, q) in enumerate(np.asarray(pairs).reshape(-1, 2))])


def joint(S, r, d, kappa, tau):
    """(S^-1, log det S, d2_joint, gain_all, sum |log L_ii|) in long double."""
    Sinv, logdet, sal = mr.inverse_ld(S)
    r = np.asarray(r, LD)
    return Sinv, logdet, r @ Sinv @ r, (logdet - logdet_omega_inv(d, kappa, tau).sum()) / 2, sal


def d2_joint_bound(Sinv_ld, r, m_r, bI):
    Sa, ra = np.abs(np.asarray(Sinv_ld, np.float64)), np.abs(np.asarray(r, np.float64))
    z = np.abs(np.asarray(Sinv_ld @ np.asarray(r, LD), np.float64))
    return float(2 * z @ m_r + bI * ra.sum() ** 2 + 2 * (len(ra) + 2) * U * (ra @ Sa @ ra))


def block_stats(Cb, rho):
    """(pd, log det, d2, z, L) of a dof-block in long double."""
    Cs = np.asarray((Cb + Cb.T) / 2, LD)
    L, kstar, _ = fr.cholesky_ld(Cs)
    if kstar >= 0:
        return False, LD(0), LD(0), None, None
    Li = fr.lower_inverse_ld(L)
    z = Li @ np.asarray(rho, LD)
    return True, 2 * np.log(np.diag(L)).sum(), z @ z, Li.T @ z, L


def greedy(S, r, d, kappa, tau, budget, d2_max=0.0, mutant=None):
    """The greedy rule in long double.  Returns (selected, steps, trace): steps rows (index, gain, d2, eligible); trace[t] a dict of
    the (m,) arrays gain, d2, pd, eligible, taken and the conditional blocks C, rho of that step.  Mutants: rho_not_updated -- the
    residual is never conditioned; tie_high -- ties go to the higher index; gate_unconditioned -- the gate compares the candidate's
    own d2 = r_i^T S_ii^-1 r_i."""
    dof = cr.dof_of(d)
    m = len(np.asarray(kappa).reshape(-1))
    W, rho = np.array(S, LD), np.array(r, LD)
    W0, r0 = W.copy(), rho.copy()
    lw = logdet_omega_inv(d, kappa, tau)
    taken = np.zeros(m, bool)
    selected, steps, trace = [], [], []
    for t in range(min(int(budget), m)):
        gain, d2, pd, el = np.zeros(m, LD), np.zeros(m, LD), np.zeros(m, bool), np.zeros(m, bool)
        for i in range(m):
            if taken[i]:
                continue
            sl = slice(dof * i, dof * i + dof)
            pd[i], lg, d2[i], _, _ = block_stats(W[sl, sl], rho[sl])
            if not pd[i]:
                continue
            gain[i] = (lg - lw[i]) / 2
            dgate = block_stats(W0[sl, sl], r0[sl])[2] if mutant == "gate_unconditioned" else d2[i]
            el[i] = not (d2_max > 0 and not dgate <= d2_max)
        trace.append({"gain": gain, "d2": d2, "pd": pd, "eligible": el, "taken": taken.copy(), "W": W.copy(), "rho": rho.copy()})
        if not el.any():
            break
        idx = np.flatnonzero(el)
        best = gain[idx].max()
        ties = idx[gain[idx] == best]
        s = int(ties[-1] if mutant == "tie_high" else ties[0])
        selected.append(s)
        steps.append((s, gain[s], d2[s], int(el.sum())))
        taken[s] = True
        ss = slice(dof * s, dof * s + dof)
        _, _, _, _, L = block_stats(W[ss, ss], rho[ss])
        Li = fr.lower_inverse_ld(L)
        Pn = W[:, ss] @ Li.T               # the panel: W[:, s] L_ss^-T
        if mutant != "rho_not_updated":
            rho = rho - Pn @ (Li @ rho[ss])
        W = W - Pn @ Pn.T
    return selected, steps, trace


def step_bounds(S, r, d, kappa, tau, selected, trace, E_in=0.0, er_in=0.0):
    """Per step t and candidate i: (bound of gain_i, bound of d2_i), (T, m) each, NaN where the candidate is taken or not
    positive definite.  E_in: the 2-norm bound of the input S's own error, er_in: that of r.  Asserts the two conditions
    rho_S <= 0.1 and rho_i' <= 0.1 the first-order bounds stand on."""
    dof = cr.dof_of(d)
    S64, r64 = np.asarray(S, np.float64), np.asarray(r, np.float64)
    m = S64.shape[0] // dof
    sd = np.sqrt(np.abs(np.diag(S64)))
    olb = omega_log_bound(d, kappa, tau)
    d2_total = float(sum(trace[t]["d2"][s] for t, s in enumerate(selected)))   # r_sel^T S_sel^-1 r_sel of the final chosen set
    bg, bd = np.full((len(trace), m), np.nan), np.full((len(trace), m), np.nan)
    for t, tr in enumerate(trace):
        gam = 2 * (dof * (t + 1) + 2) * U
        E = gam * float(np.linalg.norm(np.outer(sd, sd), 2)) + E_in
        er = gam * float(np.linalg.norm(sd)) * np.sqrt(max(d2_total, 0.0)) + er_in
        sel = np.concatenate([np.arange(dof * s, dof * s + dof) for s in selected[:t]]).astype(int) if t else np.zeros(0, int)
        if t:
            Ssel = S64[np.ix_(sel, sel)]
            nsi = 1 / np.linalg.eigvalsh(Ssel)[0]
            assert nsi > 0
            y = np.linalg.norm(np.linalg.solve(Ssel, r64[sel]))
        else:
            nsi, y = 0.0, 0.0
        Gall = np.linalg.solve(Ssel, S64[sel, :]) if t else None   # S_sel^-1 S_sel,i of every candidate at once
        rho_S = E * nsi
        assert rho_S <= 0.1, "rho_S = %g" % rho_S
        for i in range(m):
            if tr["taken"][i] or not tr["pd"][i]:
                continue
            sl = slice(dof * i, dof * i + dof)
            G = np.linalg.norm(Gall[:, sl], 2) if t else 0.0
            eC = (1 + G) ** 2 * E / (1 - rho_S)
            eR = (1 + G) * (er + E * y) / (1 - rho_S)
            Ci = np.asarray(tr["W"][sl, sl], np.float64)
            lam = np.linalg.eigvalsh((Ci + Ci.T) / 2)
            kap, nci = lam[-1] / lam[0], 1 / lam[0]
            rp, rf = eC * nci, C * U * kap
            assert rp <= 0.1 and rf <= 0.1, "rho_i' = %g, rho_f = %g" % (rp, rf)
            sal = float(np.abs(np.log(np.diag(np.linalg.cholesky((Ci + Ci.T) / 2)))).sum())
            bg[t, i] = 0.5 * (dof * rp / (1 - rp) + dof * rf / (1 - rf) + (dof + 8) * U * sal) + olb[i]
            z = np.linalg.norm(np.linalg.solve(Ci, np.asarray(tr["rho"][sl], np.float64)))
            bd[t, i] = (2 * z * eR + z * z * eC) / (1 - rp) + 4 * (dof + 1) * U * kap * float(tr["d2"][i])
    return bg, bd


def check_decisions(trace, bg, bd, d2_max=0.0, tie=None):
    """The condition every selection input must meet: at every step the two best eligible gains are GAP_FACTOR times the sum of
    their bounds apart (tie = (i, j): that one pair of candidates, an exact duplicate, is exempt), and every candidate that is
    neither taken nor indefinite is GAP_FACTOR times its bound away from d2_max.  Returns the smallest ratio met (>= 1)."""
    worst = np.inf
    for t, tr in enumerate(trace):
        live = np.flatnonzero(~tr["taken"] & tr["pd"])
        if d2_max > 0:
            for i in live:
                worst = min(worst, abs(float(tr["d2"][i]) - d2_max) / (GAP_FACTOR * bd[t, i]))
        el = np.flatnonzero(tr["eligible"])
        if len(el) < 2:
            continue
        order = el[np.argsort(-np.asarray(tr["gain"][el], np.float64), kind="stable")]
        a = order[0]
        for b in order[1:]:
            if tie is not None and {int(a), int(b)} == set(tie):
                continue
            gap = float(tr["gain"][a] - tr["gain"][b])
            worst = min(worst, gap / (GAP_FACTOR * (bg[t, a] + bg[t, b])))
    assert worst >= 1.0, "a decision sits within %.3g of its bounds" % worst
    return worst


# ---------------------------------------------------------------------------------------------------------------
# the device's block arithmetic in numpy fp64, with the mistakes a kernel could make
# ---------------------------------------------------------------------------------------------------------------
INNOV_MUTANTS = ("transposed_block", "dropped_term", "q_block_at_p", "omega_off_diagonal")


def innovation_fp64(X, d, pairs, K, S64, kappa, tau, mutant=None):
    """(cov, S) from Sigma_KK (fp64, list order) block by block as cand_math.h computes them.  Mutants: transposed_block -- block
    (j, i) written untransposed; dropped_term -- A_i S[p_i, q_j] B_j^T left out; q_block_at_p -- S[q_i, q_j] read at
    S[q_i, p_j]; omega_off_diagonal -- Omega_i^-1 added to the blocks (i, j) and (j, i) of the next candidate too."""
    dof = cr.dof_of(d)
    pairs = np.asarray(pairs).reshape(-1, 2)
    m = len(pairs)
    cov = np.zeros((dof * m, dof * m))

    def blk(a, b):
        return S64[dof * a:dof * a + dof, dof * b:dof * b + dof]

    AB = [pr.jacobian(X, d, int(p), int(q)) for p, q in pairs]
    kp = [(K.index(int(p)), K.index(int(q))) for p, q in pairs]
    for i in range(m):
        Ai, Bi = AB[i][:, :dof], AB[i][:, dof:]
        for j in range(i + 1):
            Aj, Bj = AB[j][:, :dof], AB[j][:, dof:]
            Sqq = blk(kp[i][1], kp[j][0]) if mutant == "q_block_at_p" else blk(kp[i][1], kp[j][1])
            T = Ai @ blk(kp[i][0], kp[j][0]) @ Aj.T + Bi @ blk(kp[i][1], kp[j][0]) @ Aj.T + Bi @ Sqq @ Bj.T
            if mutant != "dropped_term":
                T = T + Ai @ blk(kp[i][0], kp[j][1]) @ Bj.T
            if i == j:
                T = np.tril(T) + np.tril(T, -1).T
            cov[dof * i:dof * i + dof, dof * j:dof * j + dof] = T
            cov[dof * j:dof * j + dof, dof * i:dof * i + dof] = T if (mutant == "transposed_block" and i != j) else T.T
    w = omega_inv(d, kappa, tau)
    S = cov + np.diag(w)
    if mutant == "omega_off_diagonal":
        for i in range(m - 1):
            o = np.diag(w[dof * i:dof * i + dof])
            S[dof * (i + 1):dof * (i + 2), dof * i:dof * i + dof] += o
            S[dof * i:dof * i + dof, dof * (i + 1):dof * (i + 2)] += o
    return cov, S


# ---------------------------------------------------------------------------------------------------------------
# seeded inputs of the selection, without a graph
# ---------------------------------------------------------------------------------------------------------------
def synthetic_selection(d, m, seed, dup=None, bad=None):
    """(S, r, kappa, tau) of m synthetic candidates: cov = F F^T / k of a seeded F (dof m0 x k) scaled block by block so that the
    gains spread, weights in [5, 50], residuals of size one.  dup = (i, j), i < j: candidate j is an exact copy of i (its rows
    and columns of cov, its weights and its residual are i's bit for bit).  bad = i: S_ii is replaced by -I / 2 and its
    coupling by zeros, so that C_i is never positive definite."""
    dof = cr.dof_of(d)
    rng = np.random.default_rng(seed)
    m0 = m - (1 if dup else 0)
    k = dof * m0 + 4
    F = rng.standard_normal((dof * m0, k)) * np.repeat(rng.uniform(0.2, 1.0, m0), dof)[:, None]
    cov = F @ F.T / k
    cov = np.tril(cov) + np.tril(cov, -1).T
    kappa, tau, r = rng.uniform(5, 50, m0), rng.uniform(5, 50, m0), rng.standard_normal(dof * m0) * 0.3
    who = list(range(m0))
    if dup:
        who.insert(dup[1], dup[0])
    rows = np.concatenate([np.arange(dof * c, dof * c + dof) for c in who])
    cov, r, kappa, tau = cov[np.ix_(rows, rows)], r[rows], kappa[who], tau[who]
    S = innovation(cov, d, kappa, tau)
    if bad is not None:
        sl = slice(dof * bad, dof * bad + dof)
        S[sl, :] = 0
        S[:, sl] = 0
        S[sl, sl] = -0.5 * np.eye(dof)
    return np.ascontiguousarray(S), np.ascontiguousarray(r), kappa, tau


def find_gate(S, r, d, kappa, tau, budget, want):
    """A d2_max, found on the CPU among the midpoints of the sorted conditional and unconditioned d2's of the ungated run, for
    which want(d2_max, selected) holds and every decision meets check_decisions.  None if there is none."""
    _, _, trace = greedy(S, r, d, kappa, tau, budget)
    vals = sorted({float(v) for tr in trace for v, tk, pd in zip(tr["d2"], tr["taken"], tr["pd"]) if pd and not tk})
    for lo, hi in zip(vals[:-1], vals[1:]):
        g = 0.5 * (lo + hi)
        sel, steps, tr = greedy(S, r, d, kappa, tau, budget, g)
        if not want(g, sel):
            continue
        try:
            bg, bd = step_bounds(S, r, d, kappa, tau, sel, tr)
            check_decisions(tr, bg, bd, g)
        except AssertionError:
            continue
        return g
    return None


def seeded_records(d, K, rng):
    """K pose records (t, then Y = R^T row-major) with seeded rotations and translations of size three."""
    rec = np.zeros((K, (d + 1) * d))
    for i in range(K):
        Q, R = np.linalg.qr(rng.standard_normal((d, d)))
        Q = Q * np.sign(np.diag(R))
        if np.linalg.det(Q) < 0:
            Q[:, 0] = -Q[:, 0]
        rec[i, :d] = 3 * rng.standard_normal(d)
        rec[i, d:] = Q.reshape(-1)
    return rec


def layout_of(rec, d):
    """The reference layout of the restatements (row p the translation, then the rows of Y_p) from K records."""
    K = len(rec)
    return np.concatenate([rec[:, :d], rec[:, d:].reshape(K * d, d)])
