"""Single device operators (Group::debug_apply) against the oracle's (oracle/problem.py, assembled with scipy from the
measurements), at the benchmark's node size and at the row / segment edges of the kernels.

Every operator runs under the node's own mask (the compacted live-segment launch), under the whole group's mask (the
whole-grid launch the iteration mostly uses: suffix ":all") and, for the headline node, in a one-node group.  The
tolerances are derived from the operation (u = 2^-53):
  products:  |dev - ref| <= 2 k_i u (|A| |X|)_i per entry, k_i the scalar terms of row i (both sides round)
  solves:    backward error against the oracle's matrix <= 1e-13 (|A| |x| + |b|) (inf-norms, per column) and forward
             error against the oracle's solve <= 10 kappa_1 u |x| (kappa_1 from onenormest on the oracle's factor)
  composite: the solve's forward bound carried through the operator that follows, plus the product bounds
  sums:      the fused dot products against numpy dots of the returned vectors at 1e-13 of sum |a_i b_i|
  proximal:  the rotations at 1e-12 per entry (the projected matrix's singular values asserted within 1e3 of each other
             from the oracle's), the translations at the product bound of the rows of N and T that form them
"""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import dpgo_amd
from dpgo_amd import synthetic
from oracle import g2o as og
from oracle.problem import DPGOProblem, LOSS_HUBER, LOSS_NONE, SpdSolver, project_to_SOdn, tangent_proj

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def _measurements(g):
    z = np.zeros(len(g["I"]), np.int64)
    return og.Measurements(z, g["I"], z, g["J"], g["R"], g["t"], g["kappa"], g["tau"])


def _device_graph(g, nn):
    return dpgo_amd.graph_from_edges(g["d"], g["num_poses"], g["I"], g["J"], g["R"], g["t"], g["kappa"], g["tau"], nn)


def _inv_norm1(solver, n):
    """||A^-1||_1 of an SPD matrix from its factor (onenormest: a few solves)."""
    op = spla.LinearOperator((n, n), matvec=solver.solve, rmatvec=solver.solve, matmat=solver.solve, dtype=np.float64)
    return spla.onenormest(op)


def _norm1(A):
    return float(abs(sp.csr_matrix(A)).sum(axis=0).max())


def _prod_bound(A, X, add=None, terms=None):
    """Per-entry bound on |fl(A X (+ add)) - A X (+ add)| for two independent evaluations: 2 k_i u (|A||X| + |add|)_i, k_i the
    scalar terms of row i -- its stored entries, plus `terms` (the edge contributions the two sides assembled them from, in
    their own orders: Ref.terms)."""
    A = sp.csr_matrix(A)
    k = np.diff(A.indptr).astype(np.float64) + (1 if add is not None else 0) + (0 if terms is None else terms)
    B = abs(A) @ np.abs(X) + (np.abs(add) if add is not None else 0)
    return 2 * k[:, None] * U * B


def _block_norms(V, d):
    return np.linalg.norm(V.reshape(-1, d * d), axis=1)


def _proj_bound(V, d):
    """Rounding of Proj_R(V) = V - sym(V R^T) R per d x d block: 3d + 2 roundings per entry, |R| <= 1 entrywise (row sums
    <= d), both sides: 2 (3d + 2) d u |V_i|_F per block."""
    return 2 * (3 * d + 2) * d * U * _block_norms(V, d)


def _assert_sums(got, pairs, what):
    for q, (a, b) in enumerate(pairs):
        ref = float(np.sum(a * b))
        # the device's tree reduction and numpy's pairwise sum each err by <= log2(n) u sum |a b|; 1e-13 covers n < 2^400
        assert abs(got[q] - ref) <= 1e-13 * float(np.sum(np.abs(a * b))), (what, q, got[q], ref)


class Ref:
    """The oracle's operators of one node, the RegularizedCholesky shift formed with the device's lambda_max."""

    def __init__(self, meas_a, a, loss, opt, lam_dev, precon_rr=True, scale=None):
        """scale (one per inter-node edge of the node): the Rescale::Dynamic surrogate at these scales (update_quadratic_mat)."""
        self.p = p = DPGOProblem(a, meas_a, opt.regularizer, loss, opt.reg_Cholesky_precon_max_condition_number, opt.loss_reg,
                                 preconditioner=0, dynamic=scale is not None)
        if scale is not None:
            p.update_quadratic_mat(scale)
        self.d, self.n0, self.n1 = p.d, p.n[0], p.n[1]
        m = p.mat
        self.Gtt, self.GtR, self.GRt, self.GRR, self.G = m.Gtt, m.GtR, m.GRt, m.GRR, m.G
        # the proximal step's T, N and V = H_RR - H_Rt T H_tR (the oracle keeps V for the robust losses only; the device's
        # step is the general one, DPGOProblem.cpp:618-629, for every loss)
        self.T, self.N = m.T, sp.csr_matrix(m.N)
        self.V = m.V if loss != LOSS_NONE else (m.H[self.n0:, self.n0:] - m.H[self.n0:, :self.n0] @ (sp.diags(m.T) @ m.H[:self.n0, self.n0:])).tocsr()
        # edge contributions per row of G: every incident measurement adds one term to each entry of the pose's diagonal
        # block row (d + 1 of them), and one more for the regulariser
        ti, _, tj, _, bi, bj = og.local_rows(p.info, meas_a, self.d)
        deg = np.bincount(np.concatenate([ti[bi == 0], tj[bj == 0]]), minlength=self.n0)[:self.n0] + 1
        self.terms = np.concatenate([deg, np.repeat(deg, self.d)]) * (self.d + 1)
        self.kmax = int((np.diff(sp.csr_matrix(m.G).indptr) + self.terms).max())
        self.inv_tt = _inv_norm1(p.L, self.n0)
        self.kappa_tt = _norm1(m.Gtt) * self.inv_tt
        # |G_Rt|_2 <= sqrt(|G_Rt|_1 |G_Rt|_inf)
        self.GRt_norm = np.sqrt(_norm1(m.GRt) * _norm1(m.GRt.T))
        self.lam_dev = lam_dev
        if precon_rr:
            self.Arr = (m.GRR + (lam_dev / opt.reg_Cholesky_precon_max_condition_number) * sp.eye(m.GRR.shape[0])).tocsr()
            self.Lrr = SpdSolver(self.Arr)
            self.inv_rr = _inv_norm1(self.Lrr, self.Arr.shape[0])
            self.kappa_rr = _norm1(self.Arr) * self.inv_rr

    # ---- checks of one device output against the oracle; each returns nothing and asserts
    def check_solve(self, A, solver, kappa, b, x, what):
        """x = A^-1 b from the device: backward error against A, forward error against the oracle's solve."""
        A = sp.csr_matrix(A)
        Ainf = abs(A).sum(axis=1).max()
        res = np.abs(A @ x - b).max(axis=0)
        # backward error (issue's bound), per column
        assert np.all(res <= 1e-13 * (Ainf * np.abs(x).max(axis=0) + np.abs(b).max(axis=0))), (what, res)
        xr = solver.solve(b)
        # forward error: 10 kappa_1 u |x|_1 per column
        err = np.abs(x - xr).sum(axis=0)
        assert np.all(err <= 10 * kappa * U * np.abs(xr).sum(axis=0)), (what, err, kappa)

    def tdot_bound(self, rhs_bound, t):
        """Forward bound on t = -G_tt^-1 rhs when rhs is itself known to rhs_bound (entrywise): Frobenius."""
        return 10 * self.kappa_tt * U * np.linalg.norm(t) + self.inv_tt * np.linalg.norm(rhs_bound)


def _inputs(rng, ref):
    d, n0 = ref.d, ref.n0
    R = project_to_SOdn(rng.standard_normal((d * n0, d)), d)
    Y = np.vstack([3.0 * rng.standard_normal((n0, d)), R])
    const = np.vstack([np.ones((n0, d)), np.tile(np.eye(d), (n0, 1))])   # the Laplacian's constant vector
    mag = 10.0 ** rng.uniform(-6, 6, (d + 1) * n0)[:, None]
    mixed = mag * rng.standard_normal(((d + 1) * n0, d))
    g = rng.standard_normal(((d + 1) * n0, d))
    Ydot = np.zeros_like(Y)
    Ydot[n0:] = 0.1 * tangent_proj(R, rng.standard_normal(R.shape), d)
    r = np.zeros_like(Y)
    r[n0:] = tangent_proj(R, rng.standard_normal(R.shape), d)
    Z = rng.standard_normal(((d + 1) * (n0 + ref.n1), d))
    # the proximal step's Df: random translation rows; rotation rows chosen so that the matrix it projects,
    # M = -Df_R + N^T Df_t + V R0, is s_p (Q_p + 0.3 E_p) per pose -- Q_p a rotation, |E_p| <= 1 entrywise / d: singular values within
    # [0.7, 1.3] s_p, s_p the size of the terms that cancel to it (so the cancellation costs no more than the terms' rounding)
    Dfp = rng.standard_normal(((d + 1) * n0, d))
    R0 = Z[n0:n0 + d * n0]
    rest = ref.N.T @ Dfp[:n0] + ref.V @ R0
    sc = np.repeat(np.maximum(1.0, _block_norms(rest, d)), d)[:, None]
    Mstar = sc * (project_to_SOdn(rng.standard_normal((d * n0, d)), d) + 0.3 * rng.uniform(-1, 1, (d * n0, d)) / d)
    Dfp[n0:] = rest - Mstar
    return dict(Y=Y, const=const, mixed=mixed, g=g, Ydot=Ydot, r=r, Z=Z, Dfp=Dfp)


def run_ops(grp, a, suffix, ref, x, jacobi=False):
    """Every debug operator of node a on the inputs x: {name: output}."""
    d, n0 = ref.d, ref.n0
    R0 = (d + 1) * n0
    op = lambda name, X, rows: grp.debug_apply(a, name + suffix, X, rows)
    out = {}
    for k in ("Y", "const", "mixed"):
        out["G/" + k] = op("G", x[k], R0)
    for k in ("Y", "mixed"):
        out["solve_tt/" + k] = op("solve_tt", x[k], R0)
        if not jacobi:
            out["solve_rr/" + k] = op("solve_rr", x[k], R0)
    for k in ("Y", "const"):
        Yk = x[k]
        nabla = ref.G @ Yk + x["g"]
        out["hess/" + k] = op("hess", np.vstack([Yk, nabla, x["Ydot"], x["r"]]), R0 + 4)
        out["rgrad/" + k] = op("rgrad", np.vstack([Yk, x["g"]]), 5 * R0 + 4)
    out["precon"] = op("precon", np.vstack([x["Y"], x["r"]]), R0 + 1)
    out["retract"] = op("retract", np.vstack([x["Y"], x["Ydot"], x["g"]]), R0)
    out["project"] = op("project", x["mixed"][n0:], d * n0)
    out["proximal"] = op("proximal", np.vstack([x["Z"], x["Dfp"]]), R0)
    return out


def check_ops(ref, x, out, jacobi=False, jacobi_diag=None):
    """Every output of run_ops against the oracle."""
    d, n0 = ref.d, ref.n0
    R0 = (d + 1) * n0
    G = ref.G
    for k in ("Y", "const", "mixed"):
        X = x[k]
        err = np.abs(out["G/" + k] - G @ X)
        bound = _prod_bound(G, X, terms=ref.terms)
        assert np.all(err <= bound), ("G", k, err.max(), (err / np.maximum(bound, 1e-300)).max())
    for k in ("Y", "mixed"):
        b = x[k]
        ref.check_solve(ref.Gtt, ref.p.L, ref.kappa_tt, b[:n0], out["solve_tt/" + k][:n0], "solve_tt/" + k)
        if not jacobi:
            ref.check_solve(ref.Arr, ref.Lrr, ref.kappa_rr, b[n0:], out["solve_rr/" + k][n0:], "solve_rr/" + k)
    for k in ("Y", "const"):
        Yk, g = x[k], x["g"]
        R = Yk[n0:]
        # ---- hess: Proj_R(G_Rt tdot + G_RR Rdot - SBD(Rdot, R, nabla)), tdot = -G_tt^-1 G_tR Rdot
        nabla = G @ Yk + g
        Rdot = x["Ydot"][n0:]
        H = out["hess/" + k]
        assert np.all(H[:n0] == 0)
        Href = ref.p.hessian_vector_product(Yk, nabla[n0:], Rdot)
        tdot = -ref.p.L.solve(ref.GtR @ Rdot)
        e_t = ref.tdot_bound(_prod_bound(ref.GtR, Rdot, terms=ref.terms[:n0]), tdot)
        sbd = float(np.sum(_block_norms(Rdot, d) * _block_norms(nabla[n0:], d)))
        mag = np.linalg.norm(abs(ref.GRt) @ np.abs(tdot)) + np.linalg.norm(abs(ref.GRR) @ np.abs(Rdot)) + sbd
        # the solve's forward bound carried through G_Rt, plus the
        # products (k_max terms per entry) and the block products / projection (3d + 2 per entry, |R| row sums <= d)
        tol = ref.GRt_norm * e_t + 2 * (ref.kmax + 3 * d + 2) * d * U * mag
        assert np.linalg.norm(H[n0:R0] - Href) <= tol, ("hess", k, np.linalg.norm(H[n0:R0] - Href), tol)
        _assert_sums(H[R0:R0 + 4, 0], [(Rdot, H[n0:R0]), (H[n0:R0], H[n0:R0]), (Rdot, Rdot), (Rdot, x["r"][n0:])], "hess")
        # ---- rgrad, at Y as given (launch_bsr + launch_tangent_rot)
        o = out["rgrad/" + k]
        Yp, nab1, grad1, nab2, grad2 = (o[q * R0:(q + 1) * R0] for q in range(5))
        assert np.all(np.abs(nab2 - nabla) <= _prod_bound(G, Yk, g, ref.terms)), ("rgrad nabla", k)
        assert np.all(grad2[:n0] == 0)
        dg = _block_norms(grad2[n0:] - tangent_proj(R, nab2[n0:], d), d)
        assert np.all(dg <= _proj_bound(nab2[n0:], d)), ("rgrad grad", k, dg.max())
        # ... and at Y' = [t recovered ; R] (recover_translations + apply_tcol mode 1)
        assert np.array_equal(Yp[n0:], R)
        trec = ref.p.recover_translations(R, g)
        e_t = ref.tdot_bound(_prod_bound(ref.GtR, R, g[:n0], ref.terms[:n0]), trec)
        assert np.linalg.norm(Yp[:n0] - trec) <= e_t, ("rgrad t", k, np.linalg.norm(Yp[:n0] - trec), e_t)
        assert np.all(np.abs(nab1 - (G @ Yp + g)) <= _prod_bound(G, Yp, g, ref.terms)), ("rgrad nabla'", k)
        assert np.all(grad1[:n0] == 0)
        dg = _block_norms(grad1[n0:] - tangent_proj(R, nab1[n0:], d), d)
        assert np.all(dg <= _proj_bound(nab1[n0:], d)), ("rgrad grad'", k, dg.max())
        _assert_sums(o[5 * R0:5 * R0 + 4, 0], [(grad1, grad1), (Yp, nab1), (Yp, g), (Yp, g)], "rgrad")
    # ---- precon: Proj_Y(M^-1 v)
    R = x["Y"][n0:]
    v = x["r"][n0:]
    P = out["precon"]
    assert np.all(P[:n0] == 0)
    if jacobi:
        w = v / jacobi_diag[:, None]
        # the device scales by fl(1 / diag) (2 roundings against numpy's 1) of a diagonal it assembled in its own order
        # (<= k_max positive terms: relative k_max u)
        e = (ref.kmax + 3) * U * np.linalg.norm(w)
    else:
        w = ref.Lrr.solve(v)
        e = 10 * ref.kappa_rr * U * np.linalg.norm(w)    # the solve's forward bound (the projection is a contraction)
    Pref = tangent_proj(R, w, d)
    assert np.linalg.norm(P[n0:R0] - Pref) <= e + np.linalg.norm(_proj_bound(w, d)), ("precon", np.linalg.norm(P[n0:R0] - Pref))
    _assert_sums(P[R0:R0 + 1, 0], [(v, P[n0:R0])], "precon")
    # ---- retract: [-G_tt^-1 (g_t + G_tR R+) ; R+ = proj(R + Ydot)]
    T = out["retract"]
    Rp = project_to_SOdn(R + x["Ydot"][n0:], d)
    # Ydot = R W, W skew: R + Ydot = R (I + W) has singular values >= 1, so its polar factor is conditioned <= 1; the
    # device's projection is orthonormal to 1e-13 (test_projection_kernel); 1e-12 per entry holds both sides
    assert np.abs(T[n0:] - Rp).max() <= 1e-12
    tref = ref.p.recover_translations(T[n0:], x["g"])
    e_t = ref.tdot_bound(_prod_bound(ref.GtR, T[n0:], x["g"][:n0], ref.terms[:n0]), tref)
    assert np.linalg.norm(T[:n0] - tref) <= e_t, ("retract t", np.linalg.norm(T[:n0] - tref), e_t)
    # ---- proximal: R = proj(M), M = -Df_R + N^T Df_t + V R0; t = t0 - N (R - R0) - T Df_t
    Z, Df = x["Z"], x["Dfp"]
    t0, R0z = Z[:n0], Z[n0:n0 + d * n0]
    M = -Df[n0:] + ref.N.T @ Df[:n0] + ref.V @ R0z
    Rp = project_to_SOdn(M, d)
    tp = t0 - ref.N @ (Rp - R0z) - ref.T[:, None] * Df[:n0]
    if not ref.p.trivial:   # (the oracle's own statement of the step, where it takes this branch)
        assert np.array_equal(ref.p.proximal(Z, Df), np.vstack([tp, Rp]))
    # the conditioning of what is projected, from the oracle's singular values: the smallest at least 1e-3 of the largest
    sv = np.linalg.svd(M.reshape(n0, d, d), compute_uv=False)
    assert np.all(sv[:, -1] >= 1e-3 * sv[:, 0]), ("proximal conditioning", (sv[:, -1] / sv[:, 0]).min())
    X = out["proximal"]
    # the rotations: 1e-12 per entry, as for retract
    assert np.abs(X[n0:] - Rp).max() <= 1e-12, ("proximal R", np.abs(X[n0:] - Rp).max())
    # the translations: the product bound of the rows of N and T that form them (d + 2 terms per entry, both sides), plus the
    # rotations' 1e-12 carried through |N|
    aN = abs(ref.N)
    tb = 2 * (d + 2) * U * (np.abs(t0) + aN @ np.abs(X[n0:] - R0z) + np.abs(ref.T[:, None] * Df[:n0])) \
        + np.asarray(aN.sum(axis=1)) * 1e-12
    assert np.all(np.abs(X[:n0] - tp) <= tb), ("proximal t", (np.abs(X[:n0] - tp) / tb).max())
    # ---- project (the existing op; here for the whole-mask launch): nearest rotations, orthonormal
    Q = out["project"].reshape(n0, d, d)
    np.testing.assert_allclose(np.einsum("nij,nkj->nik", Q, Q), np.broadcast_to(np.eye(d), Q.shape), atol=1e-13)


# the outputs that take no solve: the same per-row arithmetic and k_reduce's order under every launch layout
BIT_SAME = ("G/Y", "G/const", "G/mixed", "project", "proximal")


def _rgrad_no_solve(o, R0):
    return o[3 * R0:5 * R0]


def compare_layouts(outs, R0):
    """Outputs of the same node under different launch layouts.  Bit-identical where the arithmetic is the same; the
    solves are not held to bits: spd_run picks the root's tile class by how many roots are live (fine_root_for), and a
    one-node group factors its node alone -- there each layout was checked against the oracle on its own."""
    names = list(outs)
    base = outs[names[0]]
    for other in names[1:]:
        o = outs[other]
        for k in BIT_SAME:
            assert np.array_equal(base[k], o[k]), (names[0], other, k)
        for k in ("rgrad/Y", "rgrad/const"):
            assert np.array_equal(_rgrad_no_solve(base[k], R0), _rgrad_no_solve(o[k], R0)), (names[0], other, k)


def _lambda(grp, a):
    return float(grp.debug_apply(a, "lambda_max", np.zeros((1, grp.d)), 1)[0, 0])


def _check_lambda(ref, lam):
    """The device's Lanczos lambda_max within the reference's own Spectra tolerance (1e-4, DPGOProblem.cpp:101-124)."""
    top = spla.eigsh(ref.GRR, k=1, which="LA", tol=1e-12, ncv=min(ref.GRR.shape[0] - 1, 20), return_eigenvectors=False)[0] \
        if ref.GRR.shape[0] > 3 else np.linalg.eigvalsh(ref.GRR.toarray())[-1]
    assert abs(lam - top) <= 1e-4 * top, (lam, top)


def _node_case(meas, a, loss, opt, layouts, seed, jacobi=False):
    """layouts: {name: (group, local index, suffix)}; runs and checks every op under each, then compares them."""
    grp0, a0, _ = next(iter(layouts.values()))
    lam = _lambda(grp0, a0) if not jacobi else 0.0
    ref = Ref(meas[a], a, loss, opt, lam, precon_rr=not jacobi)
    if not jacobi:
        _check_lambda(ref, lam)
        for grp, k, _ in layouts.values():
            assert _lambda(grp, k) == lam
    x = _inputs(np.random.default_rng(seed), ref)
    diag = ref.GRR.diagonal() if jacobi else None
    outs = {}
    for name, (grp, k, suffix) in layouts.items():
        outs[name] = run_ops(grp, k, suffix, ref, x, jacobi)
        check_ops(ref, x, outs[name], jacobi, diag)
    compare_layouts(outs, (ref.d + 1) * ref.n0)


# ---------------------------------------------------------------------------------------------------------------------
# headline node: synthetic.grid(**HEADLINE), 8 nodes; nodes 0, 3, 7 in the 8-node group (own and whole mask) and node 3
# as a one-node group (--emulate-world 8)

@pytest.fixture(scope="module")
def headline():
    g = synthetic.grid(**synthetic.HEADLINE)
    _, meas, _ = og.partition_measurements(g["num_poses"], _measurements(g), 8)
    return g, _device_graph(g, 8), meas


_HEADLINE_GROUPS = {}


def _headline_groups(headline, loss):
    if loss not in _HEADLINE_GROUPS:
        _HEADLINE_GROUPS.clear()   # (one loss's groups at a time on the device)
        _, G, _ = headline
        opt = dpgo_amd.Options.driver(loss, True)
        _HEADLINE_GROUPS[loss] = (opt, dpgo_amd.NodeGroup(G, range(8), opt), dpgo_amd.NodeGroup(G, [3], opt))
    return _HEADLINE_GROUPS[loss]


@pytest.mark.parametrize("loss", [LOSS_NONE, LOSS_HUBER])
@pytest.mark.parametrize("node", [0, 3, 7])
def test_headline_node_operators(headline, loss, node):
    _, _, meas = headline
    opt, grp8, grp1 = _headline_groups(headline, loss)
    layouts = {"own mask": (grp8, node, ""), "whole mask": (grp8, node, ":all")}
    if node == 3:
        layouts["one-node group"] = (grp1, 0, "")
    _node_case(meas, node, loss, opt, layouts, seed=100 + node)


def test_headline_groups_released():
    _HEADLINE_GROUPS.clear()


# ---------------------------------------------------------------------------------------------------------------------
# 32 x 32 x 24 lattice, 6 nodes (test_option_matrix_at_scale's graph): every node

def test_lattice_every_node_operators():
    g = synthetic.grid(32, 32, 24, 98304)
    _, meas, _ = og.partition_measurements(g["num_poses"], _measurements(g), 6)
    opt = dpgo_amd.Options.driver(LOSS_HUBER, True)
    grp = dpgo_amd.NodeGroup(_device_graph(g, 6), range(6), opt)
    for a in range(6):
        _node_case(meas, a, LOSS_HUBER, opt, {"own mask": (grp, a, ""), "whole mask": (grp, a, ":all")}, seed=200 + a)


# ---------------------------------------------------------------------------------------------------------------------
# the row-degree ladder (synthetic.ladder): every row length mod 8 / mod 16, nodes of 1, 63, 64, 65, 129 poses

@pytest.mark.parametrize("loss", [LOSS_NONE, LOSS_HUBER])
@pytest.mark.parametrize("d", [3, 2])
def test_ladder_operators(d, loss):
    g = synthetic.ladder(d)
    nn = g["num_nodes"]
    _, meas, _ = og.partition_measurements(g["num_poses"], _measurements(g), nn)
    G = _device_graph(g, nn)
    assert [G.node_sizes(a)[0] for a in range(nn)] == list(synthetic.LADDER_SIZES)
    opt = dpgo_amd.Options.driver(loss, True)
    grp = dpgo_amd.NodeGroup(G, range(nn), opt)
    for a in range(nn):
        _node_case(meas, a, loss, opt, {"own mask": (grp, a, ""), "whole mask": (grp, a, ":all")}, seed=300 + a)
    # Preconditioner::Jacobi (launch_rot_rowscale)
    optj = dpgo_amd.Options.driver(loss, True, preconditioner=dpgo_amd.PRECON_JACOBI)
    grpj = dpgo_amd.NodeGroup(G, range(nn), optj)
    for a in (0, 1, 5):
        _node_case(meas, a, loss, optj, {"own mask": (grpj, a, ""), "whole mask": (grpj, a, ":all")}, seed=400 + a, jacobi=True)


# ---------------------------------------------------------------------------------------------------------------------
# SE(2) at size: M3500, 4 nodes

def test_m3500_operators(fixtures_dir):
    path = os.path.join(fixtures_dir, "M3500.g2o")
    _, meas, _ = og.read_g2o(path, 4)
    opt = dpgo_amd.Options.driver(LOSS_HUBER, True)
    grp = dpgo_amd.NodeGroup(dpgo_amd.read_g2o(path, 4), range(4), opt)
    for a in range(4):
        _node_case(meas, a, LOSS_HUBER, opt, {"own mask": (grp, a, ""), "whole mask": (grp, a, ":all")}, seed=500 + a)
