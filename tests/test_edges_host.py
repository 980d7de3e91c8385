"""Host checks of the edge evaluation's yardstick and of the re-weighted problem (no GPU):
  * tests/edge_restatement.py against the oracle's residual rows (assemble_global's B0 / B1) and GlobalProblem.evaluate_f,
    and plain fp64 numpy against its long-double variant within the stated bound;
  * dpgo_graph_scale_edges: fields, order, identity, zero weights, refusals, and the oracle's data matrix of the scaled
    measurements against M_intra + sum_e w_e M_e;
  * the gradient identity the re-weighted certificate rests on: grad F_robust(X) = M_w X with w frozen at X;
  * the new C-ABI symbols and their argument validation."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import dpgo_amd
from oracle import g2o as og
from oracle.assemble import assemble_global
from oracle.hash import Options as OOptions
from oracle.problem import LOSS_GM, LOSS_HUBER, LOSS_NONE, LOSS_WELSCH, project_to_SOdn
from oracle.star import GlobalProblem, chordal_initialization

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_restatement as er  # noqa: E402

U = 2.0 ** -53
DELTA = 0.25   # loss_reg of the driver's options
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dpgo_debug_edge_eval_host", "dpgo_edge_eval_create", "dpgo_edge_eval_free", "dpgo_edge_eval_run", "dpgo_edge_eval_kernel_ms",
               "dpgo_graph_scale_edges", "dpgo_graph_verify_reweighted")

_cache = {}


def fixture(fixtures_dir, name):
    """(num_poses, mm, chordal point, random point) of a fixture, read once."""
    if name not in _cache:
        N, mm = og.read_g2o_file(os.path.join(fixtures_dir, name + ".g2o"))
        X0 = chordal_initialization(N, mm)
        Xr = np.random.default_rng(5).standard_normal(X0.shape)
        Xr[N:] = project_to_SOdn(Xr[N:], mm.d)
        _cache[name] = (N, mm, X0, Xr)
    return _cache[name]


def edges_of(mm):
    return mm.ipose, mm.jpose, mm.R, mm.t, mm.kappa, mm.tau


# ---------------------------------------------------------------------------------------------------------------
# 1. the restatement
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tinyGrid3D", "smallGrid3D", "M3500"])
def test_fp64_restatement_within_a_fraction_of_the_bound(fixtures_dir, name):
    """Plain fp64 numpy against long double: inside the bound (it uses a small fraction of it; the worst ratio is printed
    and recorded in DESIGN 13)."""
    N, mm, X0, Xr = fixture(fixtures_dir, name)
    worst = 0.0
    for X in (X0, Xr):
        a = er.edge_s(*edges_of(mm), X, np.float64)
        b = er.edge_s(*edges_of(mm), X, np.longdouble)
        bnd = er.s_bound(*edges_of(mm), X)
        for k in range(2):
            err = np.abs(np.asarray(a[k] - b[k], np.float64))
            assert np.all(err <= bnd[k]), name
            worst = max(worst, float(np.max(err / np.maximum(bnd[k], 1e-300))))
        err = np.abs(np.asarray((a[0] + a[1]) - (b[0] + b[1]), np.float64))
        assert np.all(err <= bnd[2]), name
        worst = max(worst, float(np.max(err / np.maximum(bnd[2], 1e-300))))
    print(name, "fp64 numpy vs long double: worst error / bound = %.4f" % worst)


@pytest.mark.parametrize("name", ["tinyGrid3D", "smallGrid3D", "M3500"])
@pytest.mark.parametrize("nn", [1, 2, 5])
def test_restatement_against_the_oracles_rows(fixtures_dir, name, nn):
    """s_e = |(B X)_e|^2 of assemble_global's residual rows, intra (B0) and inter (B1).  The oracle is fp64 and scales by
    sqrt(kappa), sqrt(tau) before the products (two more roundings against the same magnitudes): twice the bound."""
    N, mm, X0, Xr = fixture(fixtures_dir, name)
    d = mm.d
    gp = GlobalProblem(N, mm, nn, OOptions.driver(LOSS_HUBER, True))
    inter = er.inter_mask(N, nn, mm.ipose, mm.jpose)
    assert inter.sum() == len(gp.inter) and (~inter).sum() == len(gp.intra)
    assert (inter.sum() == 0) == (nn == 1)
    for X in (X0, Xr):
        sr, st = er.edge_s(*edges_of(mm), X, np.longdouble)
        s = np.asarray(sr + st, np.float64)
        bnd = er.s_bound(*edges_of(mm), X)[2]
        for B, mask in ((gp.B0, ~inter), (gp.B1, inter)):
            if not mask.any():
                continue
            so = np.sum((B @ X).reshape(int(mask.sum()), (d + 1) * d) ** 2, axis=1)
            assert np.all(np.abs(so - s[mask]) <= 2 * bnd[mask]), (name, nn)


@pytest.mark.parametrize("name", ["tinyGrid3D", "smallGrid3D", "M3500"])
@pytest.mark.parametrize("nn", [1, 2, 5])
@pytest.mark.parametrize("loss", [LOSS_HUBER, LOSS_GM, LOSS_WELSCH])
def test_restatement_against_evaluate_f(fixtures_dir, name, nn, loss):
    """F = 1/2 sum_intra s + 1/2 sum_inter rho against GlobalProblem.evaluate_f (DPGOStar.cpp:713-761).  |rho'| <= 1 for the
    three losses, so an error in s is not amplified: the sum of the per-edge bounds (both sides carry one), plus the
    roundings of two sums of m terms."""
    N, mm, X0, Xr = fixture(fixtures_dir, name)
    gp = GlobalProblem(N, mm, nn, OOptions.driver(loss, True))
    m = len(mm)
    for X in (X0, Xr):
        ref = er.evaluate(N, nn, *edges_of(mm), X, loss, DELTA, np.longdouble)
        tol = 0.5 * 3 * float(np.sum(er.s_bound(*edges_of(mm), X)[2])) + 2 * m * U * float(ref["F"])
        assert abs(gp.evaluate_f(X) - float(ref["F"])) <= tol, (name, nn, loss)
        got = er.evaluate(N, nn, *edges_of(mm), X, loss, DELTA, np.float64)
        assert abs(got["F"] - float(ref["F"])) <= tol


def test_loss_formulas_at_their_corners():
    s = np.array([0.0, 0.1, 0.25, 0.3, 7.0, 200.0])
    for loss in (LOSS_HUBER, LOSS_GM, LOSS_WELSCH):
        rho, w = er.rho_w(s, loss, DELTA)
        assert rho[0] == 0 and w[0] == 1
        assert np.all(np.diff(rho) >= 0) and np.all(np.diff(w) <= 0) and np.all(rho <= s) and np.all(w <= 1)
    rho, w = er.rho_w(s, LOSS_HUBER, DELTA)
    assert np.array_equal(rho[:3], s[:3]) and np.all(w[:3] == 1) and np.all(w[3:] < 1)
    rho, w = er.rho_w(np.array([800 * DELTA]), LOSS_WELSCH, DELTA)
    assert w[0] == 0 and rho[0] == DELTA
    rho, w = er.rho_w(s, LOSS_NONE, DELTA)
    assert np.array_equal(rho, s) and np.all(w == 1)


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 257])
def test_library_host_restatement_of_the_kernel(d, m):
    """dpgo_debug_edge_eval_host -- the kernel's per-lane code (edge_math.h) on the library's own records, summed in the
    device's order, compiled for the host -- against the long-double restatement, with the bounds and cases of the GPU test."""
    g = er.random_graph(d, m)
    E = (g["I"], g["J"], g["R"], g["t"], g["kappa"], g["tau"])
    ref_s = er.edge_s(*E, g["X"], np.longdouble)
    bnd = er.s_bound(*E, g["X"])
    for nn in (1, 2, 5):
        G = dpgo_amd.graph_from_edges(d, g["N"], *E, nn)
        for loss in (LOSS_NONE, LOSS_HUBER, LOSS_GM, LOSS_WELSCH):
            a = dpgo_amd.edge_eval_host(G, g["X"], loss, DELTA)
            er.check_run(g, nn, loss, a, ref_s, bnd)
            b = dpgo_amd.edge_eval_host(G, g["X"], loss, DELTA)
            assert all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4].F == b[4].F
    with pytest.raises(ValueError):
        dpgo_amd.edge_eval_host(G, g["X"][:-1], LOSS_HUBER, DELTA)
    with pytest.raises(ValueError):
        dpgo_amd.edge_eval_host(G, g["X"], LOSS_HUBER, 0.0)
    with pytest.raises(ValueError):
        dpgo_amd.edge_eval_host(G, g["X"], 7, DELTA)


@pytest.mark.parametrize("name,nn,loss", [("smallGrid3D", 2, LOSS_HUBER), ("tinyGrid3D", 2, LOSS_WELSCH), ("M3500", 5, LOSS_GM)])
def test_library_host_restatement_on_the_fixtures(fixtures_dir, name, nn, loss):
    """... and on graphs read from files: F against GlobalProblem.evaluate_f (1e-11 relative, the tolerance of
    test_evaluate_f_and_grad_at_arbitrary_X), the per-edge values within the bound."""
    N, mm, X0, Xr = fixture(fixtures_dir, name)
    G = dpgo_amd.read_g2o(os.path.join(fixtures_dir, name + ".g2o"), nn)
    gp = GlobalProblem(N, mm, nn, OOptions.driver(loss, True))
    for X in (X0, Xr):
        s_rot, s_trans, rho, w, sm = dpgo_amd.edge_eval_host(G, X, loss, DELTA)
        ref = er.edge_s(*edges_of(mm), X, np.longdouble)
        bnd = er.s_bound(*edges_of(mm), X)
        assert np.all(np.abs(np.asarray(s_rot - ref[0], np.float64)) <= bnd[0])
        assert np.all(np.abs(np.asarray(s_trans - ref[1], np.float64)) <= bnd[1])
        Fo = gp.evaluate_f(X)
        assert abs(sm.F - Fo) <= 1e-11 * abs(Fo)
        assert sm.num_inter == int(er.inter_mask(N, nn, mm.ipose, mm.jpose).sum()) and sm.weight_min == w.min()


# ---------------------------------------------------------------------------------------------------------------
# 2. dpgo_graph_scale_edges
# ---------------------------------------------------------------------------------------------------------------
def test_scale_edges_fields_order_identity_and_zeros(fixtures_dir):
    for name, nn in (("tinyGrid3D", 2), ("smallGrid3D", 5), ("M3500", 3)):
        G = dpgo_amd.read_g2o(os.path.join(fixtures_dir, name + ".g2o"), nn)
        I, J, R, t, kap, tau = G.edges()
        m = G.num_edges
        one = G.scale_edges(np.ones(m))
        assert (one.d, one.num_poses, one.num_nodes, one.num_edges) == (G.d, G.num_poses, G.num_nodes, m)
        for a, b in zip(one.edges(), G.edges()):
            assert np.array_equal(a, b)
        for a in range(nn):
            assert one.node_sizes(a) == G.node_sizes(a) and one.node_offset(a) == G.node_offset(a)
            for which in ("index", "sent", "recv"):
                assert one.node_maps(a, which) == G.node_maps(a, which)
        w = np.random.default_rng(3).uniform(0, 1, m)
        w[::7] = 0.0
        w[1::7] = 1.0
        H = G.scale_edges(w)
        I2, J2, R2, t2, kap2, tau2 = H.edges()
        assert np.array_equal(I2, I) and np.array_equal(J2, J) and np.array_equal(R2, R) and np.array_equal(t2, t)
        assert np.array_equal(kap2, kap * w) and np.array_equal(tau2, tau * w)
        assert np.all(kap2[::7] == 0) and np.all(tau2[::7] == 0) and H.num_edges == m   # zero-weight edges stay
        for a in range(nn):
            assert H.node_sizes(a) == G.node_sizes(a)
        # G itself is untouched
        assert np.array_equal(G.edges()[4], kap)


def test_scale_edges_refusals(fixtures_dir):
    G = dpgo_amd.read_g2o(os.path.join(fixtures_dir, "tinyGrid3D.g2o"), 2)
    m = G.num_edges
    for bad in (-1e-300, -1.0, float("nan"), float("inf"), -float("inf")):
        w = np.ones(m)
        w[m // 2] = bad
        with pytest.raises(ValueError):
            G.scale_edges(w)
    with pytest.raises(ValueError):
        G.scale_edges(np.ones(m + 1))
    L = dpgo_amd.lib()
    h = C.c_void_p(1)
    w = np.ones(m)
    assert L.dpgo_graph_scale_edges(None, dpgo_amd._dp(w), C.byref(h)) == -1 and not h.value
    h = C.c_void_p(1)
    assert L.dpgo_graph_scale_edges(G._h, None, C.byref(h)) == -1 and not h.value
    assert L.dpgo_graph_scale_edges(G._h, dpgo_amd._dp(w), None) == -1


@pytest.mark.parametrize("name,nn", [("tinyGrid3D", 2), ("smallGrid3D", 2)])
def test_data_matrix_of_the_scaled_graph(fixtures_dir, name, nn):
    """The oracle's M of the library's scaled measurements = M_intra + sum_e w_e M_e (M_e: the data matrix of inter edge e
    alone).  Entry by entry both are sums of the same products w_e kappa_e (...); the bound is a few roundings per term
    against the sum of the terms' magnitudes, |M_intra| + sum_e w_e |M_e|."""
    N, mm, _, _ = fixture(fixtures_dir, name)
    d = mm.d
    G = dpgo_amd.read_g2o(os.path.join(fixtures_dir, name + ".g2o"), nn)
    inter = er.inter_mask(N, nn, mm.ipose, mm.jpose)
    w = np.ones(len(mm))
    w[inter] = np.random.default_rng(11).uniform(0, 1, int(inter.sum()))
    w[np.nonzero(inter)[0][::5]] = 0.0
    I, J, R, t, kap, tau = G.scale_edges(w).edges()
    z = np.zeros(len(I), np.int64)
    got = GlobalProblem(N, og.Measurements(z, I, z, J, R, t, kap, tau), nn, OOptions.driver(LOSS_NONE, True)).M
    none = mm.take([])

    def data_matrix(sel):
        sub = mm.take(sel)
        return assemble_global(N, d, sub, none, sub.ipose, sub.jpose, [], [])[0]

    want = sp.csr_matrix(data_matrix(np.nonzero(~inter)[0]))
    mag = abs(want)
    for e in np.nonzero(inter)[0]:
        Me = data_matrix([e])
        want = want + w[e] * Me
        mag = mag + w[e] * abs(Me)
    k = int(np.max(np.diff(sp.csr_matrix(mag).indptr)))
    err = abs(sp.csr_matrix(got) - want).toarray()
    assert np.all(err <= 8 * k * U * mag.toarray()), float(err.max())
    assert err.max() < 1e-10


# ---------------------------------------------------------------------------------------------------------------
# 3. the gradient identity
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nn", [("tinyGrid3D", 2), ("smallGrid3D", 2), ("smallGrid3D", 5)])
@pytest.mark.parametrize("loss", [LOSS_HUBER, LOSS_GM, LOSS_WELSCH])
def test_gradient_identity(fixtures_dir, name, nn, loss):
    """evaluate_grad of the robust problem at X (B0' B0 X + B1' W B1 X, DPGOStar.cpp:763-829) is the gradient of the
    trivial-loss problem on the measurements scaled by the weights frozen at X (M_w X): the same terms, summed in another
    order.  Bound per entry: 2 (k + d + 3) u (|B0|' |B0| + |B1|' W |B1|) |X|, k the longest row -- nothing cancels inside
    the right-hand side."""
    N, mm, X0, Xr = fixture(fixtures_dir, name)
    d = mm.d
    rob = GlobalProblem(N, mm, nn, OOptions.driver(loss, True))
    for X in (X0, Xr):
        w = np.asarray(er.evaluate(N, nn, *edges_of(mm), X, loss, DELTA)["w"], np.float64)
        assert np.all(w[~er.inter_mask(N, nn, mm.ipose, mm.jpose)] == 1)
        tri = GlobalProblem(N, er.scaled(mm, w), nn, OOptions.driver(LOSS_NONE, True))
        g_rob, g_w = rob.evaluate_grad(X), tri.evaluate_grad(X)
        wi = np.repeat(w[er.inter_mask(N, nn, mm.ipose, mm.jpose)], d + 1)
        A = abs(rob.B0).T @ abs(rob.B0) + abs(rob.B1).T @ sp.diags(wi) @ abs(rob.B1)
        k = int(np.max(np.diff(sp.csr_matrix(A).indptr)))
        bD = 2 * (k + d + 3) * U * (A @ np.abs(X))
        # the tangent projection is the same linear map of the d x d block Df_p on both sides, with |Y_p| <= 1 entrywise: an
        # entry of its image moves by at most the entry's own error plus d times the block's summed error; its own roundings
        # (a dozen per entry against the block's magnitude) are counted with the block of A |X|
        blk = (bD[N:] + 16 * d * U * (A @ np.abs(X))[N:]).reshape(N, d * d).sum(axis=1)
        bound = bD.copy()
        bound[N:] += d * np.repeat(blk, d)[:, None]
        diff = np.abs(g_rob - g_w)
        print(name, nn, loss, "|grad F_robust - grad F_w| = %.3e, |grad| = %.3e" % (np.linalg.norm(diff), np.linalg.norm(g_rob)))
        assert np.all(diff <= bound)
        assert np.linalg.norm(diff) <= 1e-10 * max(np.linalg.norm(g_rob), 1.0)


# ---------------------------------------------------------------------------------------------------------------
# 4. the C ABI
# ---------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "dpgo_amd.h")).read()
    L = dpgo_amd.lib()
    for name in NEW_SYMBOLS:
        assert name + "(" in header and name in dpgo_amd.SYMBOLS and hasattr(L, name)
    assert "dpgo_edge_summary_t" in header
    assert [f for f, _ in dpgo_amd.EdgeSummary._fields_] == ["F", "F_intra", "F_inter", "weight_min", "num_inter",
                                                              "num_downweighted"]
    assert C.sizeof(dpgo_amd.EdgeSummary) == 4 * 8 + 2 * 4


def test_argument_validation(fixtures_dir):
    """Every new entry returns -1 on a NULL handle or argument, and leaves its output handle NULL.  (What needs a device --
    the successful paths -- is in tests/test_gpu_edges.py; on a machine without one, create itself returns -1.)"""
    L = dpgo_amd.lib()
    G = dpgo_amd.read_g2o(os.path.join(fixtures_dir, "tinyGrid3D.g2o"), 2)
    X = np.asfortranarray(G.chordal_initialization())
    h = C.c_void_p(1)
    assert L.dpgo_edge_eval_create(None, 0, C.byref(h)) == -1 and not h.value
    assert L.dpgo_edge_eval_create(G._h, 0, None) == -1
    h = C.c_void_p(1)
    assert L.dpgo_edge_eval_create(G._h, 1 << 20, C.byref(h)) == -1 and not h.value      # no such device anywhere
    s = dpgo_amd.EdgeSummary()
    assert L.dpgo_edge_eval_run(None, dpgo_amd._dp(X), X.shape[0], 0, 0.25, None, None, None, None, C.byref(s)) == -1
    ms = C.c_double()
    assert L.dpgo_edge_eval_kernel_ms(None, C.byref(ms)) == -1
    L.dpgo_edge_eval_free(None)
    res, fac, o = dpgo_amd.CertResult(), dpgo_amd.CertFactor(), dpgo_amd.CertOptions()
    args = lambda g, x, r, f: L.dpgo_graph_verify_reweighted(g, 0, x, X.shape[0], 1, 0.25, C.byref(o), 0, r, f, C.byref(s), None, 0)
    assert args(None, dpgo_amd._dp(X), C.byref(res), C.byref(fac)) == -1
    assert args(G._h, None, C.byref(res), C.byref(fac)) == -1
    assert args(G._h, dpgo_amd._dp(X), None, C.byref(fac)) == -1
    assert args(G._h, dpgo_amd._dp(X), C.byref(res), None) == -1
