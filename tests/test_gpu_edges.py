"""The edge evaluation on the device (dpgo_amd/csrc/edges.hip: k_edge_eval, k_edge_final) and the certificate of the
re-weighted problem (dpgo_graph_scale_edges, dpgo_graph_verify_reweighted), against tests/edge_restatement.py in long
double and tests/cert_restatement.py on the oracle's data matrix of the scaled measurements.

Bounds (u = 2^-53):
  s_rot, s_trans   (d + 3) u s_bar, s_bar the same formula on absolute values with sums for differences (edge_restatement);
  rho, w           as functions of the DEVICE's own s = fl(s_rot + s_trans), relative 4 * 2^-52 (a square root or a division
                   or two, each correctly rounded, and a product); Welsch (4 + s / delta) 2^-52 -- the rounding of the
                   exponential's argument moves its value by |x| u;
  F                m times the largest per-edge bound: |rho'| <= 1, so an edge's error in s passes to rho undiminished at
                   most, and the halving leaves the other half to the roundings of rho and of the two sums;
  S_w + eta I      the entrywise bound of tests/test_gpu_cert_proof.py (restated in matrix_bound below) on the scaled
                   measurements;
  gradients        the tolerance of tests/test_gpu_parity.py::test_evaluate_f_and_grad_at_arbitrary_X (1e-10 of the largest
                   entry), F 1e-11 relative."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import dpgo_amd
from dpgo_amd import synthetic
from oracle import g2o as og
from oracle.hash import Options as OOptions
from oracle.problem import LOSS_GM, LOSS_HUBER, LOSS_NONE, LOSS_WELSCH
from oracle.star import GlobalProblem

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cert_restatement as cr  # noqa: E402
import edge_restatement as er  # noqa: E402
import test_gpu_certify as tc  # noqa: E402  (its inputs and derived bounds; none of its tests is imported)

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
DELTA = 0.25
ETA = 1e-3
ROOT = tc.ROOT
LOSSES = (LOSS_NONE, LOSS_HUBER, LOSS_GM, LOSS_WELSCH)


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
random_graph = er.random_graph


def device_graph(g, nn):
    return dpgo_amd.graph_from_edges(g["d"], g["N"], g["I"], g["J"], g["R"], g["t"], g["kappa"], g["tau"], nn)


def edges_of(g):
    return g["I"], g["J"], g["R"], g["t"], g["kappa"], g["tau"]


check_run = er.check_run


# ---------------------------------------------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 257])
def test_kernel_against_the_restatement(d, m):
    """m = 1, 63, 64, 65, 257: one lane, a wave short of one, a whole wave (one workgroup), one past it, and five
    workgroups with a one-lane tail, over partitions of 1, 2 and 5 nodes and the four losses."""
    g = random_graph(d, m)
    ref_s = er.edge_s(*edges_of(g), g["X"], np.longdouble)
    bnd = er.s_bound(*edges_of(g), g["X"])
    worst = 0.0
    for nn in (1, 2, 5):
        ev = dpgo_amd.EdgeEval(device_graph(g, nn))
        for loss in LOSSES:
            out = ev.run(g["X"], loss, DELTA)
            check_run(g, nn, loss, out, ref_s, bnd)
            worst = max(worst, float(np.max(np.abs(np.asarray(out[0] - ref_s[0], np.float64)) / np.maximum(bnd[0], 1e-300))),
                        float(np.max(np.abs(np.asarray(out[1] - ref_s[1], np.float64)) / np.maximum(bnd[1], 1e-300))))
    print("d %d m %d: worst error / bound of s_rot, s_trans = %.4f" % (d, m, worst))


@pytest.mark.parametrize("d", [2, 3])
def test_null_outputs_and_the_same_bits_twice(d):
    g = random_graph(d, 257, seed=3)
    G = device_graph(g, 2)
    ev = dpgo_amd.EdgeEval(G)
    a = ev.run(g["X"], LOSS_HUBER, DELTA)
    b = ev.run(g["X"], LOSS_HUBER, DELTA)
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x, y)
    fields = [f for f, _ in dpgo_amd.EdgeSummary._fields_]
    assert [getattr(a[4], f) for f in fields] == [getattr(b[4], f) for f in fields]
    s = ev.summary(g["X"], LOSS_HUBER, DELTA)                                   # every array NULL
    assert [getattr(s, f) for f in fields] == [getattr(a[4], f) for f in fields]
    L, X = dpgo_amd.lib(), g["X"]
    w = np.full(257, -7.0)
    assert L.dpgo_edge_eval_run(ev._h, dpgo_amd._dp(X), X.shape[0], LOSS_HUBER, DELTA, None, None, None, dpgo_amd._dp(w), None) == 0
    assert np.array_equal(w, a[3])                                              # one array, no summary
    # another loss in between does not leave anything behind
    ev.run(g["X"], LOSS_WELSCH, DELTA)
    c = ev.run(g["X"], LOSS_HUBER, DELTA)
    assert all(np.array_equal(x, y) for x, y in zip(a[:4], c[:4])) and c[4].F == a[4].F
    # a second object of the same graph gives the same bits
    e = dpgo_amd.EdgeEval(G).run(g["X"], LOSS_HUBER, DELTA)
    assert all(np.array_equal(x, y) for x, y in zip(a[:4], e[:4])) and e[4].F == a[4].F
    # refusals of run
    for bad in (lambda: ev.run(X[:-1], LOSS_HUBER, DELTA), lambda: ev.run(X, 4, DELTA), lambda: ev.run(X, -1, DELTA),
                lambda: ev.run(X, LOSS_HUBER, 0.0), lambda: ev.run(X, LOSS_GM, float("nan")), lambda: ev.run(X, LOSS_WELSCH, -1.0)):
        with pytest.raises(ValueError):
            bad()
    assert ev.run(X, LOSS_NONE, 0.0)[4].num_downweighted == 0                    # the trivial loss needs no delta
    assert ev.kernel_ms() > 0


@pytest.mark.parametrize("d", [2, 3])
def test_exact_edges(d):
    """An edge whose measurement is exactly consistent with X, built from integers: s = 0, w = 1, rho = 0 exactly under every
    loss.  And a Welsch edge with s / delta > 745 (exp underflows past the last denormal): w = 0, rho = delta exactly."""
    N = 6
    P = np.eye(d)
    P[:2, :2] = [[0.0, -1.0], [1.0, 0.0]]          # a quarter turn: integer powers
    Rg = np.stack([np.linalg.matrix_power(P, k % 4) for k in range(N)])
    tg = np.array([[3.0 * k, -2.0 * k, 5.0 + k][:d] for k in range(N)])
    I, J = np.array([0, 5, 1, 2]), np.array([5, 1, 4, 3])
    R = np.einsum("eji,ejk->eik", Rg[I], Rg[J])
    t = np.einsum("eji,ej->ei", Rg[I], tg[J] - tg[I])
    t[2, 0] += 4.0                       # edge 2: s = tau 16 = 1600 = 6400 delta
    kappa, tau = np.full(4, 100.0), np.full(4, 100.0)
    X = np.asfortranarray(synthetic.global_X(Rg, tg))
    for nn in (1, 2, 3):
        G = dpgo_amd.graph_from_edges(d, N, I, J, R, t, kappa, tau, nn)
        inter = er.inter_mask(N, nn, I, J)
        ev = dpgo_amd.EdgeEval(G)
        for loss in LOSSES:
            s_rot, s_trans, rho, w, sm = ev.run(X, loss, DELTA)
            for e in (0, 1, 3):
                assert s_rot[e] == 0 and s_trans[e] == 0 and rho[e] == 0 and w[e] == 1
            assert s_rot[2] == 0 and s_trans[2] == 1600.0
            if loss == LOSS_WELSCH and inter[2]:
                assert w[2] == 0.0 and rho[2] == DELTA and sm.weight_min == 0.0 and sm.num_downweighted == 1
                assert sm.F == 0.5 * DELTA
            elif loss == LOSS_NONE or not inter[2]:
                assert w[2] == 1.0 and rho[2] == 1600.0 and sm.num_downweighted == 0 and sm.F == 800.0
            assert sm.num_inter == int(inter.sum())


def test_F_equals_the_robust_groups_evaluate(fixtures_dir):
    """smallGrid3D on 2 nodes, Huber: F of the edge evaluation = dpgo_group_evaluate of a robust group, at the chordal point
    and at a random one (the tolerance of test_evaluate_f_and_grad_at_arbitrary_X: 1e-11 relative)."""
    path, N, mm, _, X0 = tc.problem(fixtures_dir, "smallGrid3D")
    G = dpgo_amd.read_g2o(path, 2)
    grp = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(LOSS_HUBER, True), X0=X0).group
    ev = dpgo_amd.EdgeEval(G)
    star = GlobalProblem(N, mm, 2, OOptions.driver(LOSS_HUBER, True))
    for X in (X0, tc.random_point(np.random.default_rng(7), N, 3)):
        F = grp.evaluate(X)[0]
        sm = ev.summary(X, LOSS_HUBER, DELTA)
        assert abs(sm.F - F) <= 1e-11 * abs(F)
        assert abs(sm.F - star.evaluate_f(X)) <= 1e-11 * abs(F)
        assert 0 < sm.num_downweighted <= sm.num_inter < G.num_edges


# ---------------------------------------------------------------------------------------------------------------
# 2. the re-weighted certificate
# ---------------------------------------------------------------------------------------------------------------
_conv = {}


def converged(fixtures_dir, name, loss):
    """The point the device's AMM-PGO# reaches on 2 nodes with a robust loss and the driver's options (smallGrid3D: 200
    iterations, tinyGrid3D: 100), the graph, and the robust group."""
    key = (name, loss)
    if key not in _conv:
        path = tc.problem(fixtures_dir, name)[0]
        G = dpgo_amd.read_g2o(path, 2)
        drv = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(loss, True))
        for _ in range({"tinyGrid3D": 100, "smallGrid3D": 200}[name]):
            assert drv.step() == 0
        _conv[key] = (np.array(drv.X(), order="F"), G, drv)
    return _conv[key]


def reweighted_problem(fixtures_dir, name, X, loss, w=None):
    """(weights, scaled oracle measurements, GlobalProblem of them) at X; w: the device's weights (default: the restatement's)."""
    _, N, mm, _, _ = tc.problem(fixtures_dir, name)
    if w is None:
        w = np.asarray(er.evaluate(N, 2, mm.ipose, mm.jpose, mm.R, mm.t, mm.kappa, mm.tau, X, loss, DELTA)["w"], np.float64)
    mw = er.scaled(mm, w)
    return w, mw, GlobalProblem(N, mw, 1, OOptions.driver(LOSS_NONE, True))


def matrix_bound(N, mw, nn, xi, Mw, X, eta):
    """The entrywise bound of tests/test_gpu_cert_proof.py::test_matrix_against_the_restatement for S + eta I in pose-major
    order: 2 k u T for M (T: the terms' magnitudes, k: stored entries of the row), and on the diagonal blocks
    (1 + 2u)(bM + bLambda) + 2u (|M| + |Lambda| + |eta|)."""
    d, B = mw.d, mw.d + 1
    n = B * N
    z = np.zeros(len(mw.ipose), np.int64)
    Aabs, k = tc.abs_operator(N, og.Measurements(z, mw.ipose, z, mw.jpose, np.abs(mw.R), np.abs(mw.t), mw.kappa, mw.tau), nn, xi)
    perm = np.empty(n, np.int64)
    perm[0::B] = np.arange(N)
    for r in range(1, B):
        perm[r::B] = N + d * np.arange(N) + (r - 1)
    bM = (2 * k[:, None] * U * Aabs.toarray())[np.ix_(perm, perm)]
    Mref = sp.csr_matrix(Mw).toarray()[np.ix_(perm, perm)]
    Lam = cr.lambda_blocks(Mw, X, d)
    bL = tc.lambda_bound(Aabs, k, Mw, X, d)
    LamFull, bLFull = np.zeros((n, n)), np.zeros((n, n))
    for g in range(N):
        LamFull[B * g + 1:B * g + B, B * g + 1:B * g + B] = np.abs(Lam[g])
        bLFull[B * g + 1:B * g + B, B * g + 1:B * g + B] = bL[g]
    diag_blk = np.kron(np.eye(N), np.ones((B, B))) > 0
    bound = bM.copy()
    bound[diag_blk] = ((1 + 2 * U) * (bM + bLFull) + 2 * U * (np.abs(Mref) + LamFull + np.abs(eta) * np.eye(n)))[diag_blk]
    return bound, perm


@pytest.mark.parametrize("name", ["smallGrid3D", "tinyGrid3D"])
def test_reweighted_certificate_proves_the_huber_solutions(fixtures_dir, name):
    X, G, drv = converged(fixtures_dir, name, LOSS_HUBER)
    path, N, mm, gp, _ = tc.problem(fixtures_dir, name)
    d = 3
    # the guard: the restatement's S_w at the device's X is positive semidefinite with a margin, or the test says nothing
    w_ref, mw, gw = reweighted_problem(fixtures_dir, name, X, LOSS_HUBER)
    lam = np.linalg.eigvalsh(cr.S_matrix(gw.M, X, d).toarray())
    lam_plain = np.linalg.eigvalsh(cr.S_matrix(gp.M, X, d).toarray())
    print(name, "lambda_min(S_w) = %.3e, lambda_min(S) = %.3e, downweighted %d" % (lam[0], lam_plain[0], int(np.sum(w_ref < 1))))
    assert lam[0] > -ETA / 10
    assert lam_plain[0] < -ETA          # (and the plain certificate's question has another answer)
    assert np.any(w_ref < 1)
    res, x, fac, es = dpgo_amd.verify_reweighted(G, X, LOSS_HUBER, DELTA, eta=ETA)
    print(name, dpgo_amd.CERT_NAMES[res.status], dpgo_amd.CERT_FACTOR_NAMES[fac.outcome], "pivot_min %.3e stationarity %.3e" %
          (fac.pivot_min, res.stationarity), "downweighted %d/%d weight_min %.4f" % (es.num_downweighted, es.num_inter, es.weight_min))
    assert res.status == dpgo_amd.CERT_PROVEN and fac.outcome == dpgo_amd.CERT_FACTOR_PD
    assert res.iterations == 0 and fac.pivot_min > 0 and not x.any()
    inter = er.inter_mask(N, 2, mm.ipose, mm.jpose)
    s_ref = er.evaluate(N, 2, mm.ipose, mm.jpose, mm.R, mm.t, mm.kappa, mm.tau, X, LOSS_HUBER, DELTA, np.longdouble)["s"]
    b = er.s_bound(mm.ipose, mm.jpose, mm.R, mm.t, mm.kappa, mm.tau, X)[2]
    assert int(np.sum(inter & (s_ref > DELTA + b))) <= es.num_downweighted <= int(np.sum(inter & (s_ref > DELTA - b)))
    assert es.num_inter == int(inter.sum())
    # stationarity is |S_w X| = the robust gradient norm
    rob = GlobalProblem(N, mm, 2, OOptions.driver(LOSS_HUBER, True))
    go = rob.evaluate_grad(X)
    assert abs(res.stationarity - np.linalg.norm(go)) <= 1e-9 * max(np.linalg.norm(go), 1.0)
    assert res.stationarity == fac.stationarity
    # the plain certificate at the same X: a trivial-loss group of the UNSCALED graph
    plain, _ = tc.group(path, 2)
    pres, _, pfac = plain.verify(X, eta=ETA)
    assert pres.status != dpgo_amd.CERT_PROVEN and pfac.outcome == dpgo_amd.CERT_FACTOR_NOT_PD


@pytest.mark.parametrize("name", ["smallGrid3D", "tinyGrid3D"])
def test_scaled_group_matrix_and_gradients(fixtures_dir, name):
    """The group verify_reweighted builds, built by hand: its cert_matrix against the restatement's S_w + eta I, and its
    gradient -- like the robust group's -- against the oracle's robust evaluate_grad."""
    Xc, G, drv = converged(fixtures_dir, name, LOSS_HUBER)
    _, N, mm, _, X0 = tc.problem(fixtures_dir, name)
    d, B = 3, 4
    n = B * N
    ev = dpgo_amd.EdgeEval(G)
    rob = GlobalProblem(N, mm, 2, OOptions.driver(LOSS_HUBER, True))
    opt = dpgo_amd.Options.driver(LOSS_NONE, True, max_iterations=0)
    for what, X in (("converged", Xc), ("chordal", X0), ("random", tc.random_point(np.random.default_rng(17), N, d))):
        w = ev.run(X, LOSS_HUBER, DELTA)[3]
        assert np.any(w < 1)
        _, mw, gw = reweighted_problem(fixtures_dir, name, X, LOSS_HUBER, w)
        grp = dpgo_amd.NodeGroup(G.scale_edges(w), range(2), opt)
        ptr, col, val = grp.cert_matrix(X, ETA)
        dev = sp.csr_matrix((val, col, ptr), shape=(n, n)).toarray()
        bound, perm = matrix_bound(N, mw, 2, opt.regularizer, gw.M, X, ETA)
        Sref = (cr.S_matrix(gw.M, X, d) + ETA * sp.identity(n, format="csr")).toarray()[np.ix_(perm, perm)]
        err = np.abs(dev - Sref)
        print(name, what, "cert_matrix of the scaled group: worst error / bound = %.3f" % np.max(err / np.maximum(bound, 1e-300)))
        assert np.all(err <= bound), what
        go = rob.evaluate_grad(X)
        # the tolerance of test_evaluate_f_and_grad_at_arbitrary_X, 1e-10 of the largest entry.  At the converged point the
        # gradient is what is left of terms of the size of |M_w| |X| after they cancel, and that size takes the entry's place
        scale = np.abs(go).max() if what != "converged" else (abs(sp.csr_matrix(gw.M)) @ np.abs(X)).max()
        for g in (drv.group, grp):
            F, g2, grad = g.evaluate(X, want_grad=True)
            print(name, what, "gradient: worst |dev - oracle| = %.3e, tolerance %.3e" % (np.abs(grad - go).max(), 1e-10 * scale))
            assert np.all(np.abs(grad - go) <= 1e-10 * scale), what


@pytest.mark.parametrize("nn,loss", [(2, LOSS_NONE), (1, LOSS_HUBER), (1, LOSS_WELSCH)])
def test_unit_weights_equal_verify(fixtures_dir, nn, loss):
    """The trivial loss, or a partition of one node: every weight is 1 and the result is dpgo_group_verify's, field by
    field (but for the two wall times), at a point that is proven and at one that is not."""
    path, N, mm, _, X0 = tc.problem(fixtures_dir, "smallGrid3D")
    G = dpgo_amd.read_g2o(path, nn)
    grp = dpgo_amd.NodeGroup(G, range(nn), dpgo_amd.Options.driver(LOSS_NONE, True, max_iterations=0))
    for X in (tc.converged(fixtures_dir, "smallGrid3D"), X0):
        want, xw, fw = grp.verify(X, eta=ETA)
        got, xg, fg, es = dpgo_amd.verify_reweighted(G, X, loss, DELTA, eta=ETA)
        for f, _ in dpgo_amd.CertResult._fields_:
            assert getattr(got, f) == getattr(want, f), f
        for f, _ in dpgo_amd.CertFactor._fields_:
            if f not in ("symbolic_s", "numeric_s"):
                assert getattr(fg, f) == getattr(fw, f), f
        assert np.array_equal(xg, xw)
        assert es.num_downweighted == 0 and es.weight_min == 1.0 and es.num_inter == (0 if nn == 1 else es.num_inter)
    assert want.status == dpgo_amd.CERT_NEGATIVE            # (the chordal point)
    # SKIPPED and max_factor_bytes as in verify
    want, xw, fw = grp.verify(X0, eta=ETA, max_factor_bytes=1)
    got, xg, fg, _ = dpgo_amd.verify_reweighted(G, X0, loss, DELTA, eta=ETA, max_factor_bytes=1)
    assert fg.outcome == dpgo_amd.CERT_FACTOR_SKIPPED == fw.outcome and got.status == want.status and got.theta == want.theta


def test_welsch_zero_weights(fixtures_dir):
    """tinyGrid3D with Welsch reaches weights that are exactly 0.0: the scaled graph keeps those edges with zero values, its
    trivial-loss group builds, the matrix is finite and the call returns a status."""
    X, G, drv = converged(fixtures_dir, "tinyGrid3D", LOSS_WELSCH)
    w = dpgo_amd.EdgeEval(G).run(X, LOSS_WELSCH, DELTA)[3]
    print("tinyGrid3D Welsch: weights", np.sort(w)[:6], "zeros", int(np.sum(w == 0)))
    assert np.any(w == 0.0)
    res, x, fac, es = dpgo_amd.verify_reweighted(G, X, LOSS_WELSCH, DELTA, eta=ETA)
    assert res.status in (dpgo_amd.CERT_PROVEN, dpgo_amd.CERT_NEGATIVE, dpgo_amd.CERT_NONNEGATIVE, dpgo_amd.CERT_UNDECIDED)
    assert fac.outcome in (dpgo_amd.CERT_FACTOR_PD, dpgo_amd.CERT_FACTOR_NOT_PD)
    assert es.weight_min == 0.0 and np.isfinite([res.theta, res.residual, res.stationarity, fac.pivot_min]).all()
    H = G.scale_edges(w)
    assert H.num_edges == G.num_edges
    grp = dpgo_amd.NodeGroup(H, range(2), dpgo_amd.Options.driver(LOSS_NONE, True, max_iterations=0))
    ptr, col, val = grp.cert_matrix(X, ETA)
    assert np.isfinite(val).all() and len(val) > 0
    # every weight zero on the inter-node edges: the two nodes decouple, and it still builds
    inter = er.inter_mask(G.num_poses, 2, *G.edges()[:2])
    H0 = G.scale_edges(np.where(inter, 0.0, 1.0))
    g0 = dpgo_amd.NodeGroup(H0, range(2), dpgo_amd.Options.driver(LOSS_NONE, True, max_iterations=0))
    r0, _, f0 = g0.verify(X, eta=ETA)
    assert np.isfinite([r0.theta, r0.stationarity, f0.pivot_min]).all()


# ---------------------------------------------------------------------------------------------------------------
# 3. the driver and the facade
# ---------------------------------------------------------------------------------------------------------------
def test_dist_pgo_edge_report_and_verify_reweighted(fixtures_dir, tmp_path):
    exe = os.path.join(ROOT, "dpgo_amd", "dist_pgo")
    path = os.path.join(fixtures_dir, "smallGrid3D.g2o")
    base = [exe, "--dataset", path, "--num_nodes", "2", "--iters", "200", "--dist_init", "false", "--loss", "huber"]
    outs = {}
    for tag, extra in (("plain", []), ("off", ["--edge_report=", "--verify_reweighted=false"]),
                       ("on", ["--edge_report", "edges.txt", "--verify_reweighted", "--verify"])):
        cwd = tmp_path / tag
        cwd.mkdir()
        outs[tag] = (subprocess.run(base + extra, capture_output=True, text=True, cwd=cwd, timeout=300), cwd)
        assert outs[tag][0].returncode == 0, outs[tag][0].stderr[-2000:]

    def steady(text):   # (the summary's wall time differs from run to run)
        return "\n".join(l for l in text.splitlines(True) if not l.startswith("time: "))

    # with both flags off every output is what it is without them, byte for byte
    assert steady(outs["plain"][0].stdout) == steady(outs["off"][0].stdout)
    assert sorted(os.listdir(outs["plain"][1])) == sorted(os.listdir(outs["off"][1]))
    for f in os.listdir(outs["plain"][1]):
        if f.startswith("estimates"):
            assert open(outs["plain"][1] / f, "rb").read() == open(outs["off"][1] / f, "rb").read()
    assert "reweighted" not in outs["plain"][0].stdout and not os.path.exists(outs["plain"][1] / "edges.txt")
    # on: the line after the summary (after --verify's, which stays what it was under a robust loss)
    text = outs["on"][0].stdout.rstrip().splitlines()
    head = [l for l in text if not l.startswith(("verification: ", "reweighted verification: "))]
    assert steady("\n".join(head)) == steady("\n".join(outs["plain"][0].stdout.rstrip().splitlines()))
    assert text[-2].startswith("verification: not computed") and text[-1].startswith("reweighted verification: ")
    f = text[-1].split()
    assert len(f) == 11 and f[2] == "PROVEN" and f[3] == "PD" and float(f[4]) > 0 and int(f[7]) == 0
    down, nint = (int(v) for v in f[9].split("/"))
    # the rows.  Columns 0-3 are the graph's; the values are those of EdgeEval at the driver's final X.  That X is not
    # written anywhere in full precision, so: (a) the rows are consistent with themselves and with the line, and agree with
    # the point the Python driver reaches by the same native calls to the accuracy two runs of the optimiser are compared
    # at in tests/test_gpu_parity.py (1e-6); (b) with --iters 0 the final X is the chordal initialisation, which the
    # library computes with ordered sums, and the rows are EdgeEval's at that X to the 16 digits printed.
    X, G, drv = converged(fixtures_dir, "smallGrid3D", LOSS_HUBER)
    ev = dpgo_amd.EdgeEval(G)
    I, J = G.edges()[:2]
    inter = er.inter_mask(G.num_poses, 2, I, J)

    def rows_of(path):
        rows = np.loadtxt(path)
        assert rows.shape == (G.num_edges, 8)
        assert np.array_equal(rows[:, 0], np.arange(G.num_edges)) and np.array_equal(rows[:, 1], I) and np.array_equal(rows[:, 2], J)
        assert np.array_equal(rows[:, 3].astype(bool), inter)
        return rows[:, 4:].T

    sr, st, rho, w = rows_of(outs["on"][1] / "edges.txt")
    assert (down, nint) == (int(np.sum(w < 1)), int(inter.sum())) and abs(float(f[10]) - w.min()) <= 1e-15
    assert np.allclose(rho[~inter], (sr + st)[~inter], rtol=2e-15, atol=0) and np.all(w[~inter] == 1)
    rho_ref, w_ref = er.rho_w((sr + st)[inter], LOSS_HUBER, DELTA)
    assert np.allclose(rho[inter], rho_ref, rtol=1e-14, atol=0) and np.allclose(w[inter], w_ref, rtol=1e-14, atol=0)
    dev = ev.run(X, LOSS_HUBER, DELTA)
    for got, want in zip((sr, st, rho, w), dev[:4]):
        assert np.all(np.abs(got - want) <= 1e-6 * np.maximum(np.abs(want), 1.0))
    res = dpgo_amd.verify_reweighted(G, X, LOSS_HUBER, DELTA, eta=ETA)[0]
    assert abs(float(f[8]) - res.stationarity) <= 1e-6 * max(res.stationarity, 1.0)
    cwd = tmp_path / "init"
    cwd.mkdir()
    run = subprocess.run(base[:5] + ["--iters", "0", "--dist_init", "false", "--loss", "huber", "--save", "false",
                                     "--edge_report", "e0.txt"], capture_output=True, text=True, cwd=cwd, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    X0 = G.chordal_initialization()
    for got, want in zip(rows_of(cwd / "e0.txt"), ev.run(X0, LOSS_HUBER, DELTA)[:4]):
        assert np.all(np.abs(got - want) <= 1e-15 * np.abs(want))


def test_cpp_facade_reweighted(fixtures_dir):
    """examples/facade_mm.cpp with `reweighted` as its sixth argument: DPGO::EdgeEvaluation, Graph::scale_edges and
    DPGO::fast_verification_reweighted after the loop, one line on stderr, stdout the same trace as without."""
    exe = os.path.join(ROOT, "dpgo_amd", "facade_mm")
    args = [exe, os.path.join(fixtures_dir, "smallGrid3D.g2o"), "2", "200", "huber", "1"]
    plain = subprocess.run(args, check=True, capture_output=True, text=True, timeout=300)
    out = subprocess.run(args + ["reweighted"], check=True, capture_output=True, text=True, timeout=300)
    assert out.stdout == plain.stdout
    lines = [l for l in out.stderr.splitlines() if l.startswith("reweighted verification: ")]
    assert len(lines) == 1, out.stderr[-2000:]
    f = lines[0].split()
    assert f[2] == "PROVEN" and f[3] == "PD" and float(f[4]) > 0 and int(f[6]) == 0
    down, inter = (int(v) for v in f[8].split("/"))
    assert 0 < down <= inter and int(f[10]) == dpgo_amd.read_g2o(args[1], 2).num_edges
