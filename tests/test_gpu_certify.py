"""The solution certificate on the device (dpgo_amd/csrc/cert.hip, cert.cpp) against its numpy restatement
(tests/cert_restatement.py) on the oracle's explicit data matrix.

Operator parity is entrywise within rounding bounds derived from the operation (u = 2^-53):
  M V is computed as S V + G V with the node's assembled G and S (oracle.assemble.assemble_node): the 2 bd(E) blocks of
  the inter-node edges and the regulariser xi cancel between the two, so the bound is 2 k_i u ((|G| + |S|) |V|)_i, k_i
  the stored entries of row i in both -- |M| |V| alone would be too tight;
  Lambda_p = sym((M X)_Y Y^T): the bound of M X carried through, plus 2 (d + 1) u |(M X)_Y| |Y|^T for forming it;
  S V = M V - Lambda V_Y: the product bound, plus 2 d u |Lambda_p| |V_p| for the block term, plus |dLambda_p| |V_p|.
The search is held to what its result claims (theta and residual recomputed with the restatement's S), to dense eigvalsh
on the small fixtures (Kato-Temple), and to the decisions on the real fixtures."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import dpgo_amd
from oracle import g2o as og
from oracle.assemble import assemble_node
from oracle.hash import Options as OOptions
from oracle.problem import LOSS_NONE, project_to_SOdn
from oracle.star import GlobalProblem, chordal_initialization

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cert_restatement as cr  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
_cache = {}


def problem(fixtures_dir, name):
    """(path, num_poses, mm, GlobalProblem, chordal point) of a fixture."""
    if name not in _cache:
        path = os.path.join(fixtures_dir, name + ".g2o")
        num_poses, mm = og.read_g2o_file(path)
        gp = GlobalProblem(num_poses, mm, 1, OOptions.driver(LOSS_NONE, True))
        _cache[name] = (path, num_poses, mm, gp, chordal_initialization(num_poses, mm))
    return _cache[name]


def group(path, nn, iterate=False):
    """A LOSS_NONE group hosting all nn nodes; without `iterate` it is created with max_iterations = 0 (no refinement, so
    the optimiser's preconditioner is not factorised): all the certificate needs."""
    opt = dpgo_amd.Options.driver(LOSS_NONE, True) if iterate else dpgo_amd.Options.driver(LOSS_NONE, True, max_iterations=0)
    G = dpgo_amd.read_g2o(path, nn)
    return dpgo_amd.NodeGroup(G, range(nn), opt), opt


def random_point(rng, N, d):
    X = rng.standard_normal(((d + 1) * N, d))
    X[N:] = project_to_SOdn(X[N:], d)
    return X


_conv = {}


def converged(fixtures_dir, name):
    """The point the device's AMM-PGO# reaches on 2 nodes (LOSS_NONE, driver options): 100 / 200 iterations."""
    if name not in _conv:
        path = problem(fixtures_dir, name)[0]
        drv = dpgo_amd.DistPGO(dpgo_amd.read_g2o(path, 2), dpgo_amd.Options.driver(LOSS_NONE, True))
        for _ in range({"tinyGrid3D": 100, "smallGrid3D": 200}[name]):
            assert drv.step() == 0
        _conv[name] = np.array(drv.X())
    return _conv[name]


def abs_operator(num_poses, mm, nn, xi):
    """|G| + |S| of every node on the global ordering, and the stored entries per row (the k_i of the product bound)."""
    d = mm.d
    N = num_poses
    _, meas, g_index = og.partition_measurements(num_poses, mm, nn)
    rows, cols, vals = [], [], []
    k = np.zeros((d + 1) * N)
    for a in range(nn):
        info = og.generate_data_info(a, meas[a])
        n0, n1 = info.n
        m = assemble_node(info, d, xi, True)
        gl = np.zeros((d + 1) * (n0 + n1), np.int64)   # node-local row / column -> global
        for node, poses in info.index.items():
            for pose, (is_nbr, j) in poses.items():
                g = g_index[node][pose]
                t = (d + 1) * n0 + j if is_nbr else j
                r = (d + 1) * n0 + n1 + j * d if is_nbr else n0 + j * d
                gl[t] = g
                gl[r:r + d] = N + g * d + np.arange(d)
        for A in (sp.coo_matrix(m.G), sp.coo_matrix(m.S)):
            rows.append(gl[A.row]); cols.append(gl[A.col]); vals.append(np.abs(A.data))
        k[gl[:(d + 1) * n0]] = np.diff(sp.csr_matrix(m.G).indptr) + np.diff(sp.csr_matrix(m.S).indptr)
    Aabs = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=((d + 1) * N,) * 2).tocsr()
    return Aabs, k


def prod_bound(Aabs, k, V):
    """Per-entry bound on |fl(M V) - M V| for two independent evaluations (see the module docstring)."""
    return 2 * k[:, None] * U * (Aabs @ np.abs(V))


def lambda_bound(Aabs, k, M, X, d):
    N = X.shape[0] // (d + 1)
    bX = prod_bound(Aabs, k, X)[N:].reshape(N, d, d)
    MY = np.abs(M @ X)[N:].reshape(N, d, d)
    Y = np.abs(X[N:]).reshape(N, d, d)
    E = np.einsum("prc,psc->prs", bX + 2 * (d + 1) * U * MY, Y)
    return 0.5 * (E + E.transpose(0, 2, 1))


def apply_bound(Aabs, k, M, X, V, d):
    N = X.shape[0] // (d + 1)
    Lam = np.abs(cr.lambda_blocks(M, X, d))
    dL = lambda_bound(Aabs, k, M, X, d)
    b = prod_bound(Aabs, k, V)
    VY = np.abs(V[N:]).reshape(N, d, d)
    b[N:] += np.einsum("prk,pkc->prc", 2 * d * U * Lam + dL, VY).reshape(N * d, d)
    return b + 2 * U * np.abs(cr.apply(M, X, V, d))


def norm2(S):
    return float(abs(spla.eigsh(S, k=1, which="LM", return_eigenvectors=False, tol=1e-6)[0]))


def check_result(S, nS, res, x, eta, tau):
    """What the result claims, recomputed with the restatement's S.  1e-10 |S| is a rounding floor (4.5e5 u): the device
    sums up to 20 000 terms in another order."""
    assert abs(np.linalg.norm(x) - 1.0) <= 1e-12
    sx = S @ x
    th = float(x @ sx)
    assert abs(th - res.theta) <= 1e-10 * nS, (th, res.theta)
    assert abs(np.linalg.norm(sx - res.theta * x) - res.residual) <= 1e-10 * nS
    assert res.status == cr.status_of(res.theta, res.residual, res.S_norm_est, eta, tau)
    assert 0 < res.S_norm_est <= nS * (1 + 1e-9)


# ---------------------------------------------------------------------------------------------------------------
# the operator
# ---------------------------------------------------------------------------------------------------------------
CASES = [("tinyGrid3D", 1), ("tinyGrid3D", 2), ("smallGrid3D", 1), ("smallGrid3D", 2), ("smallGrid3D", 5), ("M3500", 4), ("torus3D", 8)]


@pytest.mark.parametrize("name,nn", CASES)
def test_lambda_and_apply_against_the_restatement(fixtures_dir, name, nn):
    path, N, mm, gp, X0 = problem(fixtures_dir, name)
    d = mm.d
    grp, opt = group(path, nn)
    Aabs, k = abs_operator(N, mm, nn, opt.regularizer)
    rng = np.random.default_rng(11)
    for what, X in (("chordal", X0), ("random", random_point(rng, N, d))):
        V = rng.standard_normal(X.shape)
        Lam = grp.cert_lambda(X)
        ref = cr.lambda_blocks(gp.M, X, d)
        bL = lambda_bound(Aabs, k, gp.M, X, d)
        assert np.all(np.abs(Lam - ref) <= bL), (what, np.max(np.abs(Lam - ref) / bL))
        assert np.array_equal(Lam, Lam.transpose(0, 2, 1))
        SV = grp.cert_apply(X, V)
        refSV = cr.apply(gp.M, X, V, d)
        b = apply_bound(Aabs, k, gp.M, X, V, d)
        assert np.all(np.abs(SV - refSV) <= b), (what, np.max(np.abs(SV - refSV) / b))
        # stationarity = |S X|_F = |grad F| of the group's own evaluation.  Held at points where the gradient is of the size
        # of the terms it is made of (chordal, random): at a converged point both sides are differences of terms 1e6 times
        # larger than the result and agree to their rounding only, not to 1e-10 of the result.
        res, _ = grp.certify(X, max_iters=0)
        _, g2 = grp.evaluate(X)
        print(name, nn, what, "stationarity %.12e sqrt(grad_sqnorm) %.12e" % (res.stationarity, np.sqrt(g2)))
        assert abs(res.stationarity - np.sqrt(g2)) <= 1e-10 * np.sqrt(g2)
        assert res.status == dpgo_amd.CERT_UNDECIDED or res.theta < -0.5e-3
        assert res.iterations == 0


def test_every_partition_gives_the_same_product(fixtures_dir):
    path, N, mm, gp, X0 = problem(fixtures_dir, "smallGrid3D")
    d = mm.d
    V = np.random.default_rng(5).standard_normal(X0.shape)
    out, bounds = [], []
    for nn in (1, 2, 5):
        grp, opt = group(path, nn)
        Aabs, k = abs_operator(N, mm, nn, opt.regularizer)
        out.append(grp.cert_apply(X0, V))
        bounds.append(apply_bound(Aabs, k, gp.M, X0, V, d))
    for i in (1, 2):   # the halo copy is the only thing that differs
        assert np.all(np.abs(out[i] - out[0]) <= 2 * np.maximum(bounds[i], bounds[0]))


# ---------------------------------------------------------------------------------------------------------------
# the search
# ---------------------------------------------------------------------------------------------------------------
def small_point(fixtures_dir, name, which):
    path, N, mm, gp, X0 = problem(fixtures_dir, name)
    X = X0 if which == "chordal" else converged(fixtures_dir, name)
    S = cr.S_matrix(gp.M, X, mm.d)
    lam = np.linalg.eigvalsh(S.toarray())
    return path, X, S, lam, max(abs(lam[0]), abs(lam[-1]))


@pytest.mark.parametrize("name,which", [("tinyGrid3D", "chordal"), ("tinyGrid3D", "converged"), ("smallGrid3D", "chordal")])
@pytest.mark.parametrize("precondition", [True, False])
def test_well_separated_minimum(fixtures_dir, name, which, precondition):
    path, X, S, lam, nS = small_point(fixtures_dir, name, which)
    grp, _ = group(path, 2)
    for seed in range(3):
        V0 = np.random.default_rng(seed).standard_normal(X.shape)
        res, x = grp.certify(X, tau=1e-9, max_iters=3000, stop_on_negative=False, precondition=precondition, V0=V0)
        print(name, which, precondition, seed, dpgo_amd.CERT_NAMES[res.status], res.iterations, res.restarts,
              "theta - lambda_min = %.3e, residual = %.3e" % (res.theta - lam[0], res.residual))
        check_result(S, nS, res, x, 1e-3, 1e-9)
        assert res.status != dpgo_amd.CERT_UNDECIDED
        assert res.theta < lam[1]
        assert -1e-10 * nS <= res.theta - lam[0] <= res.residual ** 2 / (lam[1] - res.theta) + 1e-10 * nS   # Kato-Temple


@pytest.mark.parametrize("precondition", [True, False])
def test_clustered_minimum(fixtures_dir, precondition):
    """smallGrid3D converged: d + 1 gauge eigenvalues within a few 1e-9 of zero, then a gap to 1.96."""
    path, X, S, lam, nS = small_point(fixtures_dir, "smallGrid3D", "converged")
    grp, _ = group(path, 2)
    for seed in range(3):
        V0 = np.random.default_rng(seed).standard_normal(X.shape)
        res, x = grp.certify(X, tau=1e-9, max_iters=3000, stop_on_negative=False, precondition=precondition, V0=V0)
        print("smallGrid3D converged", precondition, seed, dpgo_amd.CERT_NAMES[res.status], res.iterations, res.restarts,
              "theta = %.3e, residual = %.3e, lambda = %s" % (res.theta, res.residual, lam[:5]))
        check_result(S, nS, res, x, 1e-3, 1e-9)
        assert res.status == dpgo_amd.CERT_NONNEGATIVE
        assert lam[0] - 1e-10 * nS <= res.theta <= lam[3] + res.residual ** 2 / (lam[4] - res.theta) + 1e-10 * nS


def test_decisions_on_the_converged_small_fixtures(fixtures_dir):
    """Default options, preconditioner on: the tinyGrid3D run every parity test treats as the answer is NOT certified
    (lambda_min = -3.65); the smallGrid3D run is."""
    for name, want in (("tinyGrid3D", dpgo_amd.CERT_NEGATIVE), ("smallGrid3D", dpgo_amd.CERT_NONNEGATIVE)):
        path, X, S, lam, nS = small_point(fixtures_dir, name, "converged")
        grp, _ = group(path, 2)
        res, x = grp.certify(X)
        print(name, dpgo_amd.CERT_NAMES[res.status], res.iterations, res.theta, res.residual, res.stationarity)
        check_result(S, nS, res, x, 1e-3, 1e-6)
        assert res.status == want
        if want == dpgo_amd.CERT_NEGATIVE:
            assert float(x @ (S @ x)) < -0.5e-3


@pytest.mark.parametrize("name,nn,eta", [("torus3D", 8, 1e-3), ("sphere2500", 4, 1e-5), ("M3500", 4, 1e-5)])
def test_decisions_at_the_chordal_points(fixtures_dir, name, nn, eta):
    """NEGATIVE, checked by recomputing x' S x < -eta / 2 with the restatement's S.  sphere2500 and M3500 with eta = 1e-5:
    their lambda_min of -5.65e-4 / -5.39e-4 is too close to -eta/2 = -5e-4 for the default to be a fair test."""
    path, N, mm, gp, X0 = problem(fixtures_dir, name)
    S = cr.S_matrix(gp.M, X0, mm.d)
    grp, _ = group(path, nn)
    res, x = grp.certify(X0, eta=eta)
    print(name, nn, dpgo_amd.CERT_NAMES[res.status], res.iterations, res.restarts, res.theta, res.residual, res.stationarity)
    check_result(S, norm2(S), res, x, eta, 1e-6)
    assert res.status == dpgo_amd.CERT_NEGATIVE
    assert float(x @ (S @ x)) < -0.5 * eta


def test_undecided_is_reachable_and_honest(fixtures_dir):
    path, X, S, lam, nS = small_point(fixtures_dir, "smallGrid3D", "converged")
    grp, _ = group(path, 2)
    res, x = grp.certify(X, max_iters=3)
    assert res.status == dpgo_amd.CERT_UNDECIDED and res.iterations == 3
    check_result(S, nS, res, x, 1e-3, 1e-6)


def test_reproducible(fixtures_dir):
    path, X, S, lam, nS = small_point(fixtures_dir, "smallGrid3D", "chordal")
    grp, _ = group(path, 2)
    V0 = np.random.default_rng(4).standard_normal(X.shape)
    for kw in (dict(V0=V0), dict(seed=7)):
        a, xa = grp.certify(X, stop_on_negative=False, **kw)
        b, xb = grp.certify(X, stop_on_negative=False, **kw)
        assert (a.theta, a.residual, a.iterations, a.status) == (b.theta, b.residual, b.iterations, b.status)
        assert np.array_equal(xa, xb)
        assert a.status == dpgo_amd.CERT_NEGATIVE
    c, xc = grp.certify(X, stop_on_negative=False, seed=8)
    assert not np.array_equal(xc, xa)


def test_certify_does_not_disturb_the_optimiser(fixtures_dir):
    """30 AMM-PGO# iterations with a certify call after every fifth: bit for bit the run without."""
    path = problem(fixtures_dir, "smallGrid3D")[0]
    runs = []
    for with_cert in (False, True):
        drv = dpgo_amd.DistPGO(dpgo_amd.read_g2o(path, 2), dpgo_amd.Options.driver(LOSS_NONE, True))
        trace = []
        for it in range(30):
            assert drv.step() == 0
            if with_cert and it % 5 == 4:
                res, _ = drv.group.certify(drv.X(), max_iters=40)
                assert res.iterations > 0
            trace.append([getattr(drv.group.results(a), f) for a in range(2) for f in ("fobj", "gamma", "gradFnorm", "Gk")])
        runs.append((np.array(drv.X()), [drv.group[a].Xk() for a in range(2)], np.array(trace)))
    assert np.array_equal(runs[0][0], runs[1][0])
    for a in range(2):
        assert np.array_equal(runs[0][1][a], runs[1][1][a])
    assert np.array_equal(runs[0][2], runs[1][2])


def test_refusals(fixtures_dir):
    path, N, mm, gp, X0 = problem(fixtures_dir, "smallGrid3D")
    G = dpgo_amd.read_g2o(path, 2)
    # a robust loss
    hub = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(dpgo_amd.LOSS_HUBER, True), X0=X0)
    with pytest.raises(RuntimeError):
        hub.group.certify(X0)
    with pytest.raises(RuntimeError):
        hub.group.cert_lambda(X0)
    assert hub.step() == 0
    # a group that hosts one of two nodes
    part = dpgo_amd.NodeGroup(G, [0], dpgo_amd.Options.driver(LOSS_NONE, True))
    with pytest.raises(RuntimeError):
        part.certify(X0)
    # sizes
    drv = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(LOSS_NONE, True), X0=X0)
    with pytest.raises(RuntimeError):
        drv.group.certify(X0[:-1])
    with pytest.raises(ValueError):
        drv.group.certify(X0, V0=X0[:, :2])
    with pytest.raises(ValueError):
        drv.group.cert_apply(X0, X0[:-1])
    o, r = dpgo_amd.CertOptions(), dpgo_amd.CertResult()
    Xf = np.asfortranarray(X0)
    assert dpgo_amd.lib().dpgo_group_certify(drv.group._h, dpgo_amd._dp(Xf), Xf.shape[0], C_byref(o), dpgo_amd._dp(Xf),
                                             Xf.shape[0] - 1, C_byref(r), None, 0) == -1
    assert drv.step() == 0 and drv.step() == 0
    res, _ = drv.group.certify(X0)
    assert res.status == dpgo_amd.CERT_NEGATIVE


def C_byref(s):
    import ctypes
    return ctypes.byref(s)


# ---------------------------------------------------------------------------------------------------------------
# the facade and the driver
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,iters,want", [("smallGrid3D", 200, "NONNEGATIVE"), ("tinyGrid3D", 100, "NEGATIVE")])
def test_cpp_facade_verify_solution(fixtures_dir, name, iters, want):
    """examples/facade_mm.cpp with its sixth argument: DPGOHashGroup::verify_solution after the loop, the outcome on
    stderr, stdout the same trace as without."""
    exe = os.path.join(ROOT, "dpgo_amd", "facade_mm")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    args = [exe, os.path.join(fixtures_dir, name + ".g2o"), "2", str(iters), "trivial", "1"]
    plain = subprocess.run(args, check=True, capture_output=True, text=True, timeout=300)
    out = subprocess.run(args + ["certify"], check=True, capture_output=True, text=True, timeout=300)
    assert out.stdout == plain.stdout and "certificate" not in plain.stderr
    lines = [l for l in out.stderr.splitlines() if l.startswith("certificate: ")]
    assert len(lines) == 1, out.stderr[-2000:]
    f = lines[0].split()
    assert f[1] == want
    theta, residual, its, stat = float(f[2]), float(f[3]), int(f[4]), float(f[5])
    assert its > 0 and residual >= 0 and stat < 1e-3
    assert (theta < -0.5e-3) == (want == "NEGATIVE")


def test_dist_pgo_certify_flag(fixtures_dir, tmp_path):
    """--certify adds one line after the summary; without it stdout and the result files are what they were."""
    exe = os.path.join(ROOT, "dpgo_amd", "dist_pgo")
    base = [exe, "--dataset", os.path.join(fixtures_dir, "smallGrid3D.g2o"), "--num_nodes", "2", "--iters", "200", "--dist_init", "false"]
    outs = {}
    for tag, extra in (("plain", []), ("cert", ["--certify"])):
        cwd = tmp_path / tag
        cwd.mkdir()
        outs[tag] = (subprocess.run(base + extra, capture_output=True, text=True, cwd=cwd, timeout=300), cwd)
        assert outs[tag][0].returncode == 0, outs[tag][0].stderr[-2000:]

    def steady(text):   # (the summary's wall time differs from run to run)
        return [l for l in text.splitlines() if not l.startswith("time: ") and not l.startswith("certificate: ")]

    assert steady(outs["plain"][0].stdout) == steady(outs["cert"][0].stdout)
    assert "certificate" not in outs["plain"][0].stdout
    lines = [l for l in outs["cert"][0].stdout.splitlines() if l.startswith("certificate: ")]
    assert len(lines) == 1 and outs["cert"][0].stdout.rstrip().splitlines()[-1] == lines[0]
    f = lines[0].split()
    assert f[1] == "NONNEGATIVE" and abs(float(f[2])) < 0.5e-3 and int(f[4]) > 0
    a = open(outs["plain"][1] / "estimates_trivial.txt").read()
    assert a == open(outs["cert"][1] / "estimates_trivial.txt").read()
    # a robust loss: the line says why there is no certificate
    hub = subprocess.run(base[:-4] + ["--iters", "5", "--dist_init", "false", "--loss", "huber", "--certify", "--save", "false"],
                         capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert hub.returncode == 0 and "certificate: not computed" in hub.stdout
