"""numpy restatement of the edge evaluation (dpgo_amd/csrc/edges.h) and of the re-weighted problem: test infrastructure, like
tests/pcm_restatement.py and tests/cert_restatement.py.

X is in the reference layout ((d+1)N x d, t_p = row p, Y_p = R_p^T = rows N + d p ..).  For edge e = (i, j, R, t, kappa, tau):
  s_rot   = kappa |Y_j - R^T Y_i|_F^2
  s_trans = tau |t_j - t_i - t^T Y_i|^2
  s       = s_rot + s_trans
Every function takes dtype: np.float64 (plain numpy) or np.longdouble (the reference the device is held to).

The error bound of s_rot, s_trans and s is (d + 3) 2^-53 times the SAME formula with every operand replaced by its absolute
value and every difference by a sum (s_bar): an entry of the residual is a dot product of length d and one or two differences,
d + 1 or d + 2 roundings against the magnitudes it is made of, and the square and the scale add one each against s_bar."""
import numpy as np

from dpgo_amd import synthetic
from oracle import g2o as og
from oracle.problem import LOSS_GM, LOSS_HUBER, LOSS_NONE, LOSS_WELSCH

U = 2.0 ** -53


def poses(X, d, dtype=np.float64):
    N = X.shape[0] // (d + 1)
    X = np.asarray(X, dtype=dtype)
    return X[:N], X[N:].reshape(N, d, d)


def edge_s(I, J, R, t, kappa, tau, X, dtype=np.float64, absolute=False):
    """(s_rot, s_trans) per edge; absolute=True: s_bar's two halves."""
    d = t.shape[1]
    T, Y = poses(X, d, dtype)
    R, t = np.asarray(R, dtype=dtype), np.asarray(t, dtype=dtype)
    kappa, tau = np.asarray(kappa, dtype=dtype), np.asarray(tau, dtype=dtype)
    Yi, Yj, ti, tj = Y[I], Y[J], T[I], T[J]
    if absolute:
        R, t, Yi, Yj, ti, tj = (np.abs(a) for a in (R, t, Yi, Yj, ti, tj))
    m = len(I)
    RtY = np.zeros((m, d, d), dtype=dtype)
    tY = np.zeros((m, d), dtype=dtype)
    for k in range(d):   # explicit sums: einsum has no long-double kernels worth trusting
        tY += t[:, k, None] * Yi[:, k, :]
        for r in range(d):
            RtY[:, r, :] += R[:, k, r, None] * Yi[:, k, :]
    if absolute:
        er, et = Yj + RtY, tj + ti + tY
    else:
        er, et = Yj - RtY, (tj - ti) - tY
    return kappa * np.sum(np.sum(er * er, axis=2), axis=1), tau * np.sum(et * et, axis=1)


def s_bound(I, J, R, t, kappa, tau, X):
    """(bound of s_rot, of s_trans, of s) per edge."""
    d = t.shape[1]
    a, b = edge_s(I, J, R, t, kappa, tau, X, np.longdouble, absolute=True)
    c = (d + 3) * U
    return np.asarray(c * a, np.float64), np.asarray(c * b, np.float64), np.asarray(c * (a + b), np.float64)


def rho_w(s, loss, delta, dtype=np.float64):
    """(rho, w) of DPGOProblem.cpp:651-670 as functions of s."""
    s = np.asarray(s, dtype=dtype)
    dl = dtype(delta)
    if loss == LOSS_NONE:
        return s.copy(), np.ones_like(s)
    if loss == LOSS_HUBER:
        rs = np.sqrt(np.maximum(s, dl))
        return np.minimum(2 * np.sqrt(dl) * rs - dl, s), np.sqrt(dl) / rs
    if loss == LOSS_GM:
        return dl * s / (s + dl), dl * dl / ((s + dl) * (s + dl))
    if loss == LOSS_WELSCH:
        # rho = delta - delta w, evaluated as -delta expm1(-s / delta): the same number, without the cancellation at s << delta
        return -dl * np.expm1(-s / dl), np.exp(-s / dl)
    raise ValueError("loss")


def inter_mask(num_poses, num_nodes, I, J):
    node_of, _ = og.partition_index(num_poses, num_nodes)
    return node_of[np.asarray(I)] != node_of[np.asarray(J)]


def evaluate(num_poses, num_nodes, I, J, R, t, kappa, tau, X, loss, delta, dtype=np.float64):
    """dict(s_rot, s_trans, s, rho, w, inter, F, F_intra, F_inter)."""
    sr, st = edge_s(I, J, R, t, kappa, tau, X, dtype)
    s = sr + st
    inter = inter_mask(num_poses, num_nodes, I, J)
    rho, w = s.copy(), np.ones_like(s)
    if loss != LOSS_NONE and inter.any():
        rho[inter], w[inter] = rho_w(s[inter], loss, delta, dtype)
    Fi, Fe = 0.5 * np.sum(s[~inter]), 0.5 * np.sum(rho[inter])
    return dict(s_rot=sr, s_trans=st, s=s, rho=rho, w=w, inter=inter, F=Fi + Fe, F_intra=Fi, F_inter=Fe)


def scaled(mm, w):
    """The oracle's measurements with kappa, tau multiplied by w."""
    w = np.asarray(w, np.float64)
    return og.Measurements(mm.inode, mm.ipose, mm.jnode, mm.jpose, mm.R, mm.t, mm.kappa * w, mm.tau * w)


# ---- shared by tests/test_edges_host.py (the library's host restatement of the kernel) and tests/test_gpu_edges.py ----
def random_graph(d, m, N=40, seed=0):
    """m edges between random pairs of N poses: noisy relative poses of a ground truth, one in seven an outlier; X is the
    ground truth, perturbed.  Residuals straddle delta = 0.25."""
    rng = np.random.default_rng(1000 * d + m + seed)
    Rg = synthetic._random_rotations_d(rng, N, d)
    tg = rng.uniform(0, 10, (N, d))
    I = rng.integers(0, N, m)
    J = (I + rng.integers(1, N, m)) % N
    noise = synthetic._random_rotations_d(rng, m, d)
    small = np.eye(d) + 0.02 * rng.standard_normal((m, d, d))
    out = rng.uniform(size=m) < 1 / 7
    Rn = np.where(out[:, None, None], noise, small)
    Rn = np.stack([np.linalg.qr(a)[0] * np.sign(np.diag(np.linalg.qr(a)[1])) for a in Rn])
    R = np.einsum("eji,ejk,ekl->eil", Rg[I], Rg[J], Rn)                     # R_i^T R_j (noise)
    t = np.einsum("eji,ej->ei", Rg[I], tg[J] - tg[I]) + np.where(out[:, None], 3.0, 0.03) * rng.standard_normal((m, d))
    kappa, tau = rng.uniform(50, 200, m), rng.uniform(50, 100, m)
    X = synthetic.global_X(Rg, tg + 0.01 * rng.standard_normal((N, d)))
    return dict(d=d, N=N, I=I, J=J, R=R, t=t, kappa=kappa, tau=tau, X=np.asfortranarray(X))


def check_run(g, nn, loss, out, ref_s, bnd, delta=0.25):
    """One result (s_rot, s_trans, rho, w, summary) of the device, or of the host's lane-by-lane restatement of it,
    against the long-double restatement: the bounds of tests/test_gpu_edges.py's docstring."""
    s_rot, s_trans, rho, w, sm = out
    m, N = len(g["I"]), g["N"]
    inter = inter_mask(N, nn, g["I"], g["J"])
    assert np.all(np.abs(np.asarray(s_rot - ref_s[0], np.float64)) <= bnd[0])
    assert np.all(np.abs(np.asarray(s_trans - ref_s[1], np.float64)) <= bnd[1])
    s = s_rot + s_trans
    # intra edges and the trivial loss: rho = s, w = 1, exactly
    plain = ~inter if loss != LOSS_NONE else np.ones(m, bool)
    assert np.array_equal(rho[plain], s[plain]) and np.all(w[plain] == 1.0)
    if loss != LOSS_NONE and inter.any():
        rho_ref, w_ref = rho_w(s[inter], loss, delta, np.longdouble)
        rel = 4 * 2.0 ** -52 + (s[inter] / delta * 2.0 ** -52 if loss == LOSS_WELSCH else 0.0)
        assert np.all(np.abs(np.asarray(rho[inter] - rho_ref, np.float64)) <= rel * np.abs(np.asarray(rho_ref, np.float64)))
        assert np.all(np.abs(np.asarray(w[inter] - w_ref, np.float64)) <= rel * np.abs(np.asarray(w_ref, np.float64)))
    # the summary
    assert sm.num_inter == int(inter.sum())
    assert sm.num_downweighted == int(np.sum(w < 1.0)) and sm.weight_min == w.min()
    s_ref = np.asarray(ref_s[0] + ref_s[1], np.float64)
    if loss == LOSS_NONE:
        assert sm.num_downweighted == 0
    elif loss == LOSS_HUBER:
        clear = inter & (np.abs(s_ref - delta) > bnd[2])     # (w < 1 exactly when s > delta)
        assert np.array_equal((w < 1.0)[clear], (s_ref > delta)[clear])
        assert np.all(w[inter & ~clear] <= 1.0)
    else:
        assert np.all((w < 1.0)[inter & (s_ref > 1e-10)]) and np.all(w[inter & (s_ref == 0)] == 1.0)
    ref = evaluate(N, nn, *(g["I"], g["J"], g["R"], g["t"], g["kappa"], g["tau"]), g["X"], loss, delta, np.longdouble)
    tol = m * float(np.max(bnd[2]))
    assert abs(sm.F_intra - float(ref["F_intra"])) <= tol and abs(sm.F_inter - float(ref["F_inter"])) <= tol
    assert abs(sm.F - float(ref["F"])) <= tol and sm.F == sm.F_intra + sm.F_inter
