"""The comparisons tests/test_gpu_cert_search.py holds the kernels of the certificate's search to, and
tests/test_cert_search_host.py shows able to fail: test infrastructure, like the restatements.

Every comparison is against cert_restatement.gram_step / update_step evaluated in np.longdouble on the SAME input bits
(u_ld = 2^-64: its own error is 2^-11 of the bounds below and is not carried).  u = 2^-53; n = (d+1) N is the number of
products in one of the search's sums (the dead lanes of a segment add exact zeros).

Gram (k_cert_gram + k_cert_reduce):
  a sum of n products in ANY order -- fma chains of d + 1 inside a pose, a tree over the lanes, the segments in turn --
  is within gamma_n <= (n + 2) u of the sum of the magnitudes (Higham, Accuracy and Stability, (3.5)):
      |dev - ref|_ac <= (n + 2) u (|B|^T |B|)_ac                                   for B^T B,
      |dev - ref|_ac <= (n + 2) u (|B|^T (|S B| + bSB))_ac + (|B|^T bSB)_ac        for B^T (S B),
  bSB the bound on the S B the device summed: zero in the columns of S V and S P (input bits), bSW in those of S W;
  S W = M W - [0 ; Lambda W_Y] per rotation entry is a sum of d products (d u |Lambda_p| |W_p|) subtracted from M W once:
      bSW = 2 d u (|Lambda_p| |W_p|) + u |ref|                                      for a given M W,
  and (1 + u) bMW on top where the device formed M W itself (bMW = test_gpu_certify.prod_bound), translation rows
  bMW alone -- with a given M W they are copies and must be equal.
Update (k_cert_update + k_cert_reduce), T = Sum |terms| the sum of the magnitudes of the products of an entry:
  P', S P' are chains of 2d fmas, V', S V' a chain of d, one of 2d and a sum: bX = (3 d + 2) u T;
  R' = fl(S V' - theta V'), one fma on the device's own V', S V':  e = bSV + |theta| bV,  bR = (1 + u) e + u |ref|;
  W' = T_p R', a chain of d + 1 fmas per entry:  bW = |T_p| bR + (d + 2) u |T_p| (|ref R'| + bR)   (bR without T_p: a copy);
  the two norm sums, n squares in any order of values within bR (bV) of the reference's:
      b = Sum bR (2 |ref| + bR) + (n + 2) u Sum (|ref| + bR)^2.
Preconditioner (cert_build_precon) against cert_restatement.block_jacobi, both float64, different assemblies of M_pp and
different inversions:  |T_p| dM |T_p| + c u kappa_2(M_pp) |T_p|_2  entrywise, dM the assembly's bound (2 k u (|G_pp| + |S_pp|),
averaged with its transpose as the device averages the block), c = 10 x inverse_constant(): the worst
|inv - inverse by a longdouble Cholesky| / (u kappa_2 |T_p|_2) numpy's own inverse shows on the same blocks."""
import numpy as np

import cert_restatement as cr

U = 2.0 ** -53
LD = np.longdouble
BLOCKS = ("V", "W", "P", "SV", "SP", "MW")


def ntri(d):
    return 3 * d * (3 * d + 1) // 2


def gaussian_blocks(rng, shape, variant="full"):
    """Independent Gaussian V, W, P, SV, SP, MW (S V and S P are NOT products with S: nothing hides behind symmetry).
    variant: "full"; "P=0"; "W=P=0" (the loop's second and first pass); "P=W" (a singular mass matrix)."""
    b = dict((k, rng.standard_normal(shape)) for k in BLOCKS)
    if variant in ("P=0", "W=P=0"):
        b["P"] = np.zeros(shape)
    if variant == "W=P=0":
        b["W"] = np.zeros(shape)
    if variant == "P=W":
        b["P"] = b["W"].copy()
    return b


def _ratio(err, bound):
    """max err / bound, a zero bound demanding equality."""
    err, bound = np.asarray(err, LD), np.asarray(bound, LD)
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0))
    return float(np.max(r)) if r.size else 0.0


def gram_ratios(d, Lam, b, sums, SW, M=None, bMW=None):
    """Worst error / bound of one k_cert_gram + k_cert_reduce: {"BtB", "BtSB", "SW"}.  b: the blocks that went in; sums, SW:
    what came out; b["MW"] None: M W was formed on the other side from M, within bMW."""
    N = b["V"].shape[0] // (d + 1)
    n, NT = (d + 1) * N, ntri(d)
    given = b["MW"] is not None
    G, A, SWr = cr.gram_step(M, Lam, b["V"], b["W"], b["P"], b["SV"], b["SP"], d, MW=b["MW"] if given else None, dtype=LD)
    Wa = np.abs(np.asarray(b["W"], LD))
    bSW = np.zeros(SWr.shape, LD)
    bSW[N:] = 2 * d * U * (np.abs(np.asarray(Lam, LD)) @ Wa[N:].reshape(N, d, d)).reshape(N * d, d) + U * np.abs(SWr[N:])
    if not given:
        bSW = bSW + (1 + U) * np.asarray(bMW, LD)
    Ba = np.abs(np.hstack([b["V"], b["W"], b["P"]]).astype(LD))
    SBa = np.abs(np.hstack([np.asarray(b["SV"], LD), SWr, np.asarray(b["SP"], LD)]))
    bSB = np.hstack([np.zeros_like(bSW), bSW, np.zeros_like(bSW)])
    bG = (n + 2) * U * (Ba.T @ Ba)
    bA = (n + 2) * U * (Ba.T @ (SBa + bSB)) + Ba.T @ bSB
    iu = np.triu_indices(3 * d)
    sums = np.asarray(sums, LD)
    return dict(BtB=_ratio(np.abs(sums[:NT] - G[iu]), bG[iu]), BtSB=_ratio(np.abs(sums[NT:2 * NT] - A[iu]), bA[iu]),
                SW=_ratio(np.abs(np.asarray(SW, LD) - SWr), bSW))


def update_ratios(d, Cf, theta, b, out, T):
    """Worst error / bound of one k_cert_update + k_cert_reduce: {"V", "P", "SV", "SP", "W", "rr", "vv"}.  b: V, W, P, SV, SW,
    SP that went in; out: V, W, P, SV, SP, rr, vv that came out; T: the blocks the launch applied, or None."""
    N = b["V"].shape[0] // (d + 1)
    n = (d + 1) * N
    ref = cr.update_step(Cf, theta, b["V"], b["W"], b["P"], b["SV"], b["SW"], b["SP"], T, d, dtype=LD)
    Ca, th = np.abs(np.asarray(Cf, LD)), np.abs(np.asarray(theta, LD))
    a = dict((k, np.abs(np.asarray(b[k], LD))) for k in ("V", "W", "P", "SV", "SW", "SP"))
    tP = a["W"] @ Ca[d:2 * d] + a["P"] @ Ca[2 * d:]
    tSP = a["SW"] @ Ca[d:2 * d] + a["SP"] @ Ca[2 * d:]
    bound = dict(P=(3 * d + 2) * U * tP, SP=(3 * d + 2) * U * tSP, V=(3 * d + 2) * U * (a["V"] @ Ca[:d] + tP),
                 SV=(3 * d + 2) * U * (a["SV"] @ Ca[:d] + tSP))
    e = bound["SV"] + th[None, :] * bound["V"]
    bR = (1 + U) * e + U * np.abs(ref["R"])
    if T is None:
        bound["W"] = bR
    else:
        Ta = np.abs(np.asarray(T, LD))
        bound["W"] = cr.apply_block_jacobi(Ta, bR + (d + 2) * U * (np.abs(ref["R"]) + bR), d)
    r = dict((k, _ratio(np.abs(np.asarray(out[k], LD) - ref[k]), bound[k])) for k in ("V", "P", "SV", "SP", "W"))
    for key, x, bx in (("rr", ref["R"], bR), ("vv", ref["V"], bound["V"])):
        xa = np.abs(x)
        bs = np.sum(bx * (2 * xa + bx), axis=0) + (n + 2) * U * np.sum((xa + bx) ** 2, axis=0)
        r[key] = _ratio(np.abs(np.asarray(out[key], LD) - ref[key]), bs)
    return r


def pose_blocks(A, N, d):
    """((N, d+1, d+1), (N, d+1)): the diagonal pose blocks (slot 0 the translation) of a sparse matrix in the reference layout,
    and the reference rows of every pose's slots."""
    import scipy.sparse as sp
    A = sp.coo_matrix(A)
    pose = lambda i: np.where(i < N, i, (i - N) // d)          # noqa: E731
    slot = lambda i: np.where(i < N, 0, 1 + (i - N) % d)       # noqa: E731
    same = pose(A.row) == pose(A.col)
    blk = np.zeros((N, d + 1, d + 1))
    np.add.at(blk, (pose(A.row[same]), slot(A.row[same]), slot(A.col[same])), A.data[same])
    idx = np.concatenate([np.arange(N)[:, None], N + d * np.arange(N)[:, None] + np.arange(d)[None, :]], axis=1)
    return blk, idx


def cholesky_inverse_ld(Mb):
    """The inverses of symmetric positive definite blocks (N, B, B) by a Cholesky factorisation in longdouble."""
    A = np.asarray(Mb, LD)
    A = 0.5 * (A + A.transpose(0, 2, 1))
    n, B = A.shape[0], A.shape[1]
    L, Li = np.zeros((n, B, B), LD), np.zeros((n, B, B), LD)
    for j in range(B):
        L[:, j, j] = np.sqrt(A[:, j, j] - np.sum(L[:, j, :j] ** 2, axis=1))
        for i in range(j + 1, B):
            L[:, i, j] = (A[:, i, j] - np.sum(L[:, i, :j] * L[:, j, :j], axis=1)) / L[:, j, j]
    for c in range(B):
        for i in range(B):
            Li[:, i, c] = ((1.0 if i == c else 0.0) - np.sum(L[:, i, :i] * Li[:, :i, c], axis=1)) / L[:, i, i]
    return Li.transpose(0, 2, 1) @ Li


def inverse_ratios(M, N, d):
    """Per pose |inv - longdouble Cholesky inverse|_max / (u kappa_2 |T_p|_2) of numpy's inverse on the restatement's blocks."""
    Mb, _ = pose_blocks(M, N, d)
    Mb = 0.5 * (Mb + Mb.transpose(0, 2, 1))
    T = np.linalg.inv(Mb)
    err = np.max(np.abs(T - cholesky_inverse_ld(Mb)), axis=(1, 2)).astype(np.float64)
    return err / (U * np.linalg.cond(Mb, 2) * np.linalg.norm(T, 2, axis=(1, 2)))


def precon_ratio(M, Aabs, k, N, d, Tdev, c_inv):
    """Worst error / bound of cert_build_precon's blocks against block_jacobi(M, d); Aabs, k: test_gpu_certify.abs_operator."""
    Tref = cr.block_jacobi(M, d)
    Mb, idx = pose_blocks(M, N, d)
    Ab, _ = pose_blocks(Aabs, N, d)
    dM = 2 * k[idx][:, :, None] * U * Ab
    dM = 0.5 * (dM + dM.transpose(0, 2, 1))
    Ta = np.abs(Tref)
    first = Ta @ dM @ Ta
    scal = c_inv * U * np.linalg.cond(0.5 * (Mb + Mb.transpose(0, 2, 1)), 2) * np.linalg.norm(Tref, 2, axis=(1, 2))
    return _ratio(np.abs(Tdev - Tref), first + scal[:, None, None])


def worst(ratios, into):
    """Fold one comparison's ratios into a running worst-per-quantity dict; returns the quantities out of bound."""
    for q, v in ratios.items():
        into[q] = max(into.get(q, 0.0), v)
    return sorted(q for q, v in ratios.items() if not v <= 1.0)


def ritz_matrices(sums, d, nblk):
    """(A, B): the leading d nblk square of B^T (S B) and B^T B, filled from the upper triangles as cert_search fills them."""
    n, NT = d * nblk, ntri(d)
    A, B = np.zeros((n, n)), np.zeros((n, n))
    for a in range(n):
        for c in range(a, n):
            B[a, c] = B[c, a] = sums[cr.tri_index(3 * d, a, c)]
            A[a, c] = A[c, a] = sums[NT + cr.tri_index(3 * d, a, c)]
    return A, B
