"""Marginal pose covariances on the device (dpgo_amd/csrc/cov.h): NodeGroup.cov_hessian against the restated tangent-space
Hessian, NodeGroup.covariance against the dense long-double inverse of the restated anchored Hessian, on tinyGrid3D x {1, 2}
nodes, smallGrid3D x {1, 2, 5} and the d = 2 graph of tests/test_gpu_cert_proof.py (block rows of 1 - 41 blocks) x 6, at
converged points.

Bounds (u = 2^-53); nothing in them comes from the device.
  the matrix   An entry of H is a sum of at most k = 4 d products s y y' of an entry of S_pq with entries of Y_p and Y_q.
               The device's S differs from the restatement's by at most bS entrywise -- tests/test_gpu_cert_proof.py's bound of
               the certificate matrix with eta = 0: two independent assemblies of M, Lambda_p and one subtraction on the
               diagonal blocks -- and both sides then round k products of three factors and k - 1 additions:
                   |H_dev - H_ref| <= |J|^T bS |J| + 2 (k + 2) u |J|^T |S| |J|        (sums of absolute products)
  the blocks   C u kappa_2(A) ||A^-1||_2 of tests/cov_restatement.py for the factorisation and the selected inversion of A, the
               anchored H (C was fixed on the CPU, tests/test_covariance_host.py), plus what the matrix's own error moves the
               inverse by to first order, ||A^-1||_2^2 || bound of the matrix ||_2.
The device's figure per case is printed and held below 1.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cert_restatement as cert  # noqa: E402
import cov_restatement as cr  # noqa: E402
import factor_restatement as fr  # noqa: E402
import test_gpu_certify as tc  # noqa: E402  (its inputs, caches and derived bounds; none of its tests is imported)
import test_gpu_cert_proof as tp  # noqa: E402  (likewise: the d = 2 graph and the bound of the certificate matrix)

import dpgo_amd  # noqa: E402
from oracle.problem import LOSS_NONE  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ROOT = tc.ROOT
CASES = [("tinyGrid3D", 1), ("tinyGrid3D", 2), ("smallGrid3D", 1), ("smallGrid3D", 2), ("smallGrid3D", 5), ("ladder2", 6)]

_pt = {}


def converged(fixtures_dir, name):
    if name != "ladder2":
        return tc.converged(fixtures_dir, name)
    if name not in _pt:
        g, N, mm, gp, X0, nn = tp.ladder2()
        G = dpgo_amd.graph_from_edges(2, N, g["I"], g["J"], g["R"], g["t"], g["kappa"], g["tau"], nn)
        drv = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(LOSS_NONE, True), X0=X0)
        for _ in range(300):
            assert drv.step() == 0
        _pt[name] = np.array(drv.X())
    return _pt[name]


_ref = {}


def reference(fixtures_dir, name, anchor):
    """At the converged point, computed once: X, the restated anchored H, the bound of the matrix, the long-double inverse
    and the bound of its blocks, the graph's edges."""
    key = (name, anchor)
    if key not in _ref:
        N, mm, gp, _, _ = tp.instance(fixtures_dir, name)
        d = mm.d
        dof = cr.dof_of(d)
        X = converged(fixtures_dir, name)
        n = (d + 1) * N
        S = cert.S_matrix(gp.M, X, d).toarray()
        A = cr.anchored(cr.hessian(S, X, d), anchor, dof)
        # the bound of the certificate matrix in the reference layout, eta = 0 (tests/test_gpu_cert_proof.py); the partition
        # with the most stored entries per row bounds them all
        bS = np.zeros((n, n))
        Mabs = np.abs(sp.csr_matrix(gp.M).toarray())
        for nn in sorted({c[1] for c in CASES if c[0] == name}):
            opt = dpgo_amd.Options.driver(LOSS_NONE, True, max_iterations=0)
            Aabs, k = tp.abs_terms_operator(N, mm, nn, opt.regularizer)
            bM = 2 * k[:, None] * U * Aabs.toarray()
            bL = tc.lambda_bound(Aabs, k, gp.M, X, d)
            Lam = np.abs(cert.lambda_blocks(gp.M, X, d))
            b = bM.copy()
            for g in range(N):
                r = slice(N + d * g, N + d * g + d)
                b[r, r] = (1 + 2 * U) * (bM[r, r] + bL[g]) + 2 * U * (Mabs[r, r] + Lam[g])
            bS = np.maximum(bS, b)
        Sabs = Mabs.copy()
        Lam = np.abs(cert.lambda_blocks(gp.M, X, d))
        for g in range(N):
            r = slice(N + d * g, N + d * g + d)
            Sabs[r, r] += Lam[g]
        J = np.abs(cr.tangent_basis(X, d))
        kk = 4 * d
        bH = sum(J[c].T @ bS @ J[c] for c in range(d)) + 2 * (kk + 2) * U * sum(J[c].T @ Sabs @ J[c] for c in range(d))
        lam = np.linalg.eigvalsh(A)
        assert lam[0] > 0, "the restated anchored Hessian is not positive definite at this point"
        L, kstar, _ = fr.cholesky_ld(A)
        assert kstar < 0
        Xi = fr.lower_inverse_ld(L)
        Sigma = Xi.T @ Xi
        bSigma = cr.C * U * float(lam[-1] / lam[0]) / float(lam[0]) + float(np.linalg.norm(bH, 2)) / float(lam[0]) ** 2
        edges = np.unique(np.stack([np.asarray(mm.ipose), np.asarray(mm.jpose)], axis=1), axis=0).astype(np.int32)
        _ref[key] = dict(N=N, d=d, dof=dof, X=X, A=A, bH=bH, Sigma=Sigma, bSigma=bSigma, edges=edges, gp=gp)
    return _ref[key]


def make_group(fixtures_dir, name, nn):
    return tp.instance(fixtures_dir, name)[4](nn)[0]


def blocks_of(Sigma, dof, pairs):
    return np.stack([Sigma[dof * p:dof * p + dof, dof * q:dof * q + dof] for p, q in pairs])


@pytest.mark.parametrize("name,nn", CASES)
def test_hessian_against_the_restatement(fixtures_dir, name, nn):
    grp = make_group(fixtures_dir, name, nn)
    for a in (0, tp.instance(fixtures_dir, name)[0] - 1):
        R = reference(fixtures_dir, name, a)
        N, dof = R["N"], R["dof"]
        n = dof * N
        ptr, col, val = grp.cov_hessian(R["X"], anchor=a)
        assert ptr.shape == (n + 1,) and ptr[0] == 0 and ptr[-1] == len(col) == len(val) and len(val) % (dof * dof) == 0
        stored = sp.csr_matrix((np.ones(len(col)), col, ptr), shape=(n, n)).toarray() > 0
        assert int(stored.sum()) == len(col) and np.array_equal(stored, stored.T)
        blocks = stored.reshape(N, dof, N, dof).transpose(0, 2, 1, 3).reshape(N, N, dof * dof)
        assert np.all(blocks.all(axis=2) | ~blocks.any(axis=2))
        D = sp.csr_matrix((val, col, ptr), shape=(n, n)).toarray()
        assert np.all(R["A"][~stored] == 0.0)                      # every restatement entry has a place
        r = slice(dof * a, dof * a + dof)
        assert np.array_equal(D[r, r], np.eye(dof)) and not D[r, :r.start].any() and not D[r, r.stop:].any()
        assert not D[:r.start, r].any() and not D[r.stop:, r].any()
        err = np.abs(D - R["A"])
        worst = np.max(err / np.maximum(R["bH"], 1e-300))
        print("%s x %d, anchor %d: worst error / bound of the matrix = %.3f" % (name, nn, a, worst))
        assert np.all(err <= R["bH"]), worst


_blocks = {}


@pytest.mark.parametrize("name,nn", CASES)
def test_marginals_and_edge_blocks_against_the_dense_inverse(fixtures_dir, name, nn):
    grp = make_group(fixtures_dir, name, nn)
    N = tp.instance(fixtures_dir, name)[0]
    for a in (0, N - 1):
        R = reference(fixtures_dir, name, a)
        dof = R["dof"]
        marg, cross, res = grp.covariance(R["X"], anchor=a, pairs=R["edges"])
        assert res.outcome == dpgo_amd.COV_OK and res.unknowns == dof * N and res.fronts >= 1 and res.levels >= 1
        assert res.device_bytes > 0 and res.pivot_min > 0 and res.pivot_max >= res.pivot_min and res.numeric_ms > 0
        want_m = blocks_of(R["Sigma"], dof, [(p, p) for p in range(N)])
        want_c = blocks_of(R["Sigma"], dof, R["edges"])
        touch = (R["edges"] == a).any(axis=1)
        want_m[a] = 0
        want_c[touch] = 0
        assert not marg[a].any() and not cross[touch].any()      # the anchor's blocks: exactly zero
        em = float(np.abs(np.asarray(marg, fr.LD) - want_m).max()) / R["bSigma"]
        ec = float(np.abs(np.asarray(cross, fr.LD) - want_c).max()) / R["bSigma"]
        print("%s x %d, anchor %d: fronts %d, levels %d, max front %d; marginals %.3g, edge blocks %.3g of the bound; max|Sigma| %.3g"
              % (name, nn, a, res.fronts, res.levels, res.max_front, em, ec, np.abs(marg).max()))
        assert em < 1.0 and ec < 1.0
        for p in range(N):
            assert np.array_equal(marg[p], marg[p].T)            # S_pp is one product stored into both triangles
        # the transposed pair is the transposed block, and p == q is the marginal
        p, q = [int(v) for v in R["edges"][len(R["edges"]) // 2]]
        _, c2, _ = grp.covariance(R["X"], anchor=a, pairs=[[q, p], [p, p]])
        k = len(R["edges"]) // 2
        assert np.array_equal(c2[0], cross[k].T) and np.array_equal(c2[1], marg[p])
        # every partition: other orderings, other fronts, the same blocks
        first = _blocks.setdefault((name, a), (marg, cross))
        assert np.abs(marg - first[0]).max() <= 2 * R["bSigma"] and np.abs(cross - first[1]).max() <= 2 * R["bSigma"]
        again = grp.covariance(R["X"], anchor=a, pairs=R["edges"])
        assert np.array_equal(again[0], marg) and np.array_equal(again[1], cross)


@pytest.mark.parametrize("name", ["tinyGrid3D", "smallGrid3D"])
def test_a_point_that_is_no_minimum(fixtures_dir, name):
    """Every rotation replaced by a seeded random one (tests/test_covariance_host.py: an eigenvalue below -1e-3 ||H||_2):
    COV_NOT_PD, zero blocks -- and the converged point's bits afterwards, through the same factor."""
    R = reference(fixtures_dir, name, 0)
    grp = make_group(fixtures_dir, name, 2)
    before = grp.covariance(R["X"], pairs=R["edges"])
    Z = cr.random_rotations_point(R["X"], R["d"], 5)
    marg, cross, res = grp.covariance(Z, pairs=R["edges"])
    assert res.outcome == dpgo_amd.COV_NOT_PD and not marg.any() and not cross.any()
    after = grp.covariance(R["X"], pairs=R["edges"])
    assert after[2].outcome == dpgo_amd.COV_OK
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_skipped_allocates_nothing(fixtures_dir):
    import torch
    R = reference(fixtures_dir, "smallGrid3D", 0)
    grp = make_group(fixtures_dir, "smallGrid3D", 2)
    grp.covariance(R["X"], max_bytes=1)          # (the certificate's buffers and M's values, shared with cert_factor, come here)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    marg, _, res = grp.covariance(R["X"], max_bytes=1)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0
    assert res.outcome == dpgo_amd.COV_SKIPPED and not marg.any()
    assert res.unknowns == 6 * R["N"] and res.fronts >= 4 and res.levels >= 3 and res.max_front > 0 and res.device_bytes > 1
    assert res.stationarity > 0
    assert grp.covariance(R["X"], max_bytes=res.device_bytes - 1)[2].outcome == dpgo_amd.COV_SKIPPED
    ok = grp.covariance(R["X"], max_bytes=res.device_bytes)[2]
    assert ok.outcome == dpgo_amd.COV_OK and ok.device_bytes == res.device_bytes and ok.symbolic_s == 0.0


def test_refusals(fixtures_dir):
    path, N, mm, gp, X0 = tc.problem(fixtures_dir, "smallGrid3D")
    R = reference(fixtures_dir, "smallGrid3D", 0)
    X = R["X"]
    G = dpgo_amd.read_g2o(path, 2)
    hub = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(dpgo_amd.LOSS_HUBER, True), X0=X0)
    with pytest.raises(RuntimeError):
        hub.group.covariance(X)                  # a robust loss
    part = dpgo_amd.NodeGroup(G, [0], dpgo_amd.Options.driver(LOSS_NONE, True))
    with pytest.raises(RuntimeError):
        part.covariance(X)                       # a group that does not host every node
    grp = make_group(fixtures_dir, "smallGrid3D", 2)
    for bad in (dict(anchor=N), dict(anchor=-1), dict(pairs=[[0, N]]), dict(pairs=[[-1, 0]])):
        with pytest.raises(RuntimeError):
            grp.covariance(X, **bad)
    have = {(int(p), int(q)) for p, q in R["edges"]} | {(int(q), int(p)) for p, q in R["edges"]}
    non_edge = next((p, q) for p in range(N) for q in range(N) if p != q and (p, q) not in have)
    with pytest.raises(RuntimeError):
        grp.covariance(X, pairs=[non_edge])      # a pair that is not an edge
    with pytest.raises(RuntimeError):
        grp.covariance(X[:-1])
    with pytest.raises(RuntimeError):
        grp.cov_hessian(X, anchor=N)
    assert grp.covariance(X)[2].outcome == dpgo_amd.COV_OK


def test_covariance_does_not_disturb_the_optimiser(fixtures_dir):
    """30 AMM-PGO# iterations with a covariance call on a sibling trivial-loss group after every fifth: bit for bit the run
    without."""
    path = tc.problem(fixtures_dir, "smallGrid3D")[0]
    runs = []
    for with_cov in (False, True):
        drv = dpgo_amd.DistPGO(dpgo_amd.read_g2o(path, 2), dpgo_amd.Options.driver(LOSS_NONE, True))
        sib = tc.group(path, 2)[0] if with_cov else None
        trace = []
        for it in range(30):
            assert drv.step() == 0
            if with_cov and it % 5 == 4:
                assert sib.covariance(drv.X())[2].outcome in (dpgo_amd.COV_OK, dpgo_amd.COV_NOT_PD)
            trace.append([getattr(drv.group.results(a), f) for a in range(2) for f in ("fobj", "gamma", "gradFnorm", "Gk")])
        runs.append((np.array(drv.X()), [drv.group[a].Xk() for a in range(2)], np.array(trace)))
    assert np.array_equal(runs[0][0], runs[1][0])
    for a in range(2):
        assert np.array_equal(runs[0][1][a], runs[1][1][a])
    assert np.array_equal(runs[0][2], runs[1][2])


def test_reweighted_with_unit_weights_is_the_group_call(fixtures_dir):
    """LOSS_NONE: every weight is 1, the scaled graph is the graph, and the blocks are those of NodeGroup.covariance."""
    path = tc.problem(fixtures_dir, "smallGrid3D")[0]
    R = reference(fixtures_dir, "smallGrid3D", 0)
    G = dpgo_amd.read_g2o(path, 2)
    marg, cross, res, summ = dpgo_amd.covariance_reweighted(G, R["X"], LOSS_NONE, pairs=R["edges"])
    want = make_group(fixtures_dir, "smallGrid3D", 2).covariance(R["X"], pairs=R["edges"])
    assert res.outcome == dpgo_amd.COV_OK and summ.num_downweighted == 0
    assert np.array_equal(marg, want[0]) and np.array_equal(cross, want[1])
    # Huber with a small delta: the surrogate of the re-weighted graph, an answer of its own
    m2, _, r2, s2 = dpgo_amd.covariance_reweighted(G, R["X"], dpgo_amd.LOSS_HUBER, loss_reg=1e-6)
    assert r2.outcome in (dpgo_amd.COV_OK, dpgo_amd.COV_NOT_PD) and s2.num_inter > 0
    if s2.num_downweighted > 0 and r2.outcome == dpgo_amd.COV_OK:
        assert not np.array_equal(m2, marg)


# ---------------------------------------------------------------------------------------------------------------
# the facade and the driver
# ---------------------------------------------------------------------------------------------------------------
def upper(marg):
    dof = marg.shape[1]
    iu = np.triu_indices(dof)
    return np.stack([m[iu] for m in marg])


_py = {}


def python_run(fixtures_dir):
    """What the driver and the facade example do, through Python: chordal point, 200 AMM-PGO# iterations on 2 nodes, the
    covariance call on the group that iterated."""
    if not _py:
        path = tc.problem(fixtures_dir, "smallGrid3D")[0]
        drv = dpgo_amd.DistPGO(dpgo_amd.read_g2o(path, 2), dpgo_amd.Options.driver(LOSS_NONE, True))
        for _ in range(200):
            assert drv.step() == 0
        _py["v"] = drv.group.covariance(drv.X())
        assert _py["v"][2].outcome == dpgo_amd.COV_OK
    return _py["v"]


def test_cpp_facade_marginal_covariances(fixtures_dir):
    """examples/facade_mm.cpp with `covariance`: DPGOHashGroup::marginal_covariances after the loop, on stderr; stdout the same
    trace as without; the blocks those of NodeGroup.covariance bit for bit."""
    exe = os.path.join(ROOT, "dpgo_amd", "facade_mm")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    args = [exe, os.path.join(fixtures_dir, "smallGrid3D.g2o"), "2", "200", "trivial", "1"]
    plain = subprocess.run(args, check=True, capture_output=True, text=True, timeout=300)
    out = subprocess.run(args + ["covariance"], check=True, capture_output=True, text=True, timeout=300)
    assert out.stdout == plain.stdout and "covariance" not in plain.stderr
    lines = [l.split() for l in out.stderr.splitlines() if l.startswith("covariance: ")]
    marg, _, res = python_run(fixtures_dir)
    assert lines[-1][1] == "OK" and int(lines[-1][2]) == res.fronts and int(lines[-1][3]) == res.levels
    got = np.array([[float(v) for v in l[2:]] for l in lines[:-1]])
    assert [int(l[1]) for l in lines[:-1]] == list(range(len(marg)))
    assert np.array_equal(got, upper(marg))


def test_dist_pgo_covariance_flag(fixtures_dir, tmp_path):
    """--covariance FILE adds the file and one line after the summary; without it stdout and the result files are what they
    were.  The file holds NodeGroup.covariance's marginals bit for bit."""
    exe = os.path.join(ROOT, "dpgo_amd", "dist_pgo")
    base = [exe, "--dataset", os.path.join(fixtures_dir, "smallGrid3D.g2o"), "--num_nodes", "2", "--iters", "200", "--dist_init", "false"]
    outs = {}
    for tag, extra in (("plain", []), ("cov", ["--covariance", "cov.txt"])):
        cwd = tmp_path / tag
        cwd.mkdir()
        outs[tag] = (subprocess.run(base + extra, capture_output=True, text=True, cwd=cwd, timeout=300), cwd)
        assert outs[tag][0].returncode == 0, outs[tag][0].stderr[-2000:]

    def steady(text):   # (the summary's wall time differs from run to run)
        return [l for l in text.splitlines() if not l.startswith("time: ") and not l.startswith("covariance: ")]

    assert steady(outs["plain"][0].stdout) == steady(outs["cov"][0].stdout)
    assert "covariance" not in outs["plain"][0].stdout and not (outs["plain"][1] / "cov.txt").exists()
    assert sorted(os.listdir(outs["plain"][1])) == sorted(f for f in os.listdir(outs["cov"][1]) if f != "cov.txt")
    lines = [l for l in outs["cov"][0].stdout.splitlines() if l.startswith("covariance: ")]
    assert len(lines) == 1 and outs["cov"][0].stdout.rstrip().splitlines()[-1] == lines[0]
    marg, _, res = python_run(fixtures_dir)
    f = lines[0].split()
    assert f[1] == "OK" and int(f[2]) == res.unknowns and int(f[3]) == res.fronts and int(f[6]) == res.device_bytes
    rows = np.loadtxt(outs["cov"][1] / "cov.txt")
    assert np.array_equal(rows[:, 0], np.arange(len(marg))) and np.array_equal(rows[:, 1:], upper(marg))
    assert open(outs["plain"][1] / "estimates_trivial.txt").read() == open(outs["cov"][1] / "estimates_trivial.txt").read()
    # a robust loss: the line says why there is no covariance
    hub = subprocess.run(base[:-4] + ["--iters", "5", "--dist_init", "false", "--loss", "huber", "--covariance", "c.txt", "--save", "false"],
                         capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert hub.returncode == 0 and "covariance: not computed" in hub.stdout and not (tmp_path / "c.txt").exists()
