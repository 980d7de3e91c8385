"""The certificate's proof on the device -- fast_verification STEP 1, the Cholesky factorisation of S + eta I
(dpgo_amd/csrc/cert.cpp: Group::cert_factor / verify / cert_matrix; cert.hip: k_cert_matrix; spd_dev.hip in factor-only
mode) -- against the numpy restatement (tests/cert_restatement.py) on the oracle's data matrix and dense eigvalsh.

The matrix is compared entrywise within bounds derived from how it is formed (u = 2^-53), in the terms
tests/test_gpu_certify.py derives for the operator:
  M is the host's sum of a node's assembled G and S blocks, in which the inter-node and xi terms cancel, against the
  oracle's own assembly: per entry 2 k_i u T_ij, k_i the stored entries of row i in both (prod_bound on e_j) and T_ij the
  sum of the MAGNITUDES of the terms either side adds into the entry.  For a product, |G| + |S| stands in for T (what
  cancels inside an entry is small against the row's sum); entry by entry it does not: a translation-rotation entry of
  a pose with 40 edges is a sum of 40 terms tau_e (R_e t_e) of either sign, and two assemblies of the oracle itself
  (per node and global) already differ by 1.9 times 2 k u (|G| + |S|)_ij there.  T is what the same assembly gives for
  the measurements (|R_e|, |t_e|, kappa_e, tau_e): every term then enters its entry with the sign the entry's position
  fixes, so nothing cancels inside G or S, and |G'| + |S'| of that assembly is T (abs_terms_operator);
  a rotation entry of a diagonal block is fl(fl(M - Lambda) + eta [r == c]): the bound of M, lambda_bound for the
  device's Lambda, and one rounding each for the difference and the sum, (1 + 2u)(bM + bL) + 2u (|M| + |Lambda| + |eta|);
  the translation entry of a diagonal block is fl(M + eta): bM + u (|M| + |eta|) (the same expression with Lambda = 0
  covers it); every other entry is M itself.
The decision is tested on both sides of the threshold at eta = -lambda_min -+ 1e-8 |S|: Higham's condition for the
success of a floating-point Cholesky factorisation (Accuracy and Stability of Numerical Algorithms, thm 10.7) is
lambda_min(A) > ~20 n^(3/2) u |A| = 2.5e-11 |A| at n = 500 (9.3e-11 |A| at the 1209 unknowns of the d = 2 instance), so
the margin leaves a factor of 400 (100).

The d = 2 instance is synthetic.ladder(d=2) with its pose ids compacted: the generator leaves ids without edges (130
ids per node, 81 / 1 / 63 / 64 / 65 / 129 used), and a group whose own poses are fewer than the graph's is refused by
every certificate entry ("the group must host every node"), the new ones included.  Compacted, the same 403 poses
and all edges -- block rows of 1 to 41 blocks, reversed and parallel edges -- are split over the same 6 nodes by the
contiguous partition, with many more inter-node edges than the original."""
import json
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
from oracle.problem import LOSS_NONE
from oracle.star import GlobalProblem, chordal_initialization

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cert_restatement as cr  # noqa: E402
import test_gpu_certify as tc  # noqa: E402  (its inputs, caches and derived bounds; none of its tests is imported)

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ROOT = tc.ROOT
NOT_PD, PD, SKIPPED = dpgo_amd.CERT_FACTOR_NOT_PD, dpgo_amd.CERT_FACTOR_PD, dpgo_amd.CERT_FACTOR_SKIPPED


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
_ladder = {}


def ladder2():
    """(device graph maker, num_poses, mm, GlobalProblem, chordal point) of the compacted synthetic.ladder(d=2)."""
    if not _ladder:
        g = synthetic.ladder(2)
        used = np.unique(np.concatenate([g["I"], g["J"]]))
        assert len(used) == sum(synthetic.LADDER_SIZES)
        new = np.full(g["num_poses"], -1, np.int64)
        new[used] = np.arange(len(used))
        g = dict(g, I=new[g["I"]], J=new[g["J"]], num_poses=len(used))
        z = np.zeros(len(g["I"]), np.int64)
        mm = og.Measurements(z, g["I"], z, g["J"], g["R"], g["t"], g["kappa"], g["tau"])
        N, nn = g["num_poses"], g["num_nodes"]
        gp = GlobalProblem(N, mm, 1, OOptions.driver(LOSS_NONE, True))
        _ladder["v"] = (g, N, mm, gp, chordal_initialization(N, mm), nn)
    return _ladder["v"]


def instance(fixtures_dir, name):
    """(N, mm, GlobalProblem, chordal point, make_group(nn)) of a fixture or of "ladder2"."""
    if name == "ladder2":
        g, N, mm, gp, X0, _ = ladder2()

        def make(nn):
            G = dpgo_amd.graph_from_edges(2, N, g["I"], g["J"], g["R"], g["t"], g["kappa"], g["tau"], nn)
            opt = dpgo_amd.Options.driver(LOSS_NONE, True, max_iterations=0)
            return dpgo_amd.NodeGroup(G, range(nn), opt), opt
        return N, mm, gp, X0, make
    path, N, mm, gp, X0 = tc.problem(fixtures_dir, name)
    return N, mm, gp, X0, lambda nn: tc.group(path, nn)


def pose_major(N, d):
    """perm[(d+1) g + r] = the reference row of unknown r of pose g (r = 0: the translation, r >= 1: row r - 1 of Y_g)."""
    B = d + 1
    perm = np.empty(B * N, np.int64)
    perm[0::B] = np.arange(N)
    for r in range(1, B):
        perm[r::B] = N + d * np.arange(N) + (r - 1)
    return perm


def abs_terms_operator(N, mm, nn, xi):
    """tc.abs_operator on the measurements (|R|, |t|, kappa, tau): per entry the sum of the magnitudes of the terms G and
    S are made of (see the module docstring), and the stored entries per row."""
    z = np.zeros(len(mm.ipose), np.int64)
    return tc.abs_operator(N, og.Measurements(z, mm.ipose, z, mm.jpose, np.abs(mm.R), np.abs(mm.t), mm.kappa, mm.tau), nn, xi)


_spec = {}


def spectrum(fixtures_dir, name, which):
    """(X, S as CSR in the reference layout, ascending eigenvalues of S, |S|_2) at a named point, computed once."""
    key = (name, which)
    if key not in _spec:
        N, mm, gp, X0, _ = instance(fixtures_dir, name)
        if which == "chordal":
            X = X0
        elif which == "random":
            X = tc.random_point(np.random.default_rng(23), N, mm.d)
        else:
            X = tc.converged(fixtures_dir, name)
        S = cr.S_matrix(gp.M, X, mm.d)
        lam, vec = np.linalg.eigh(S.toarray())
        _spec[key] = (X, S, lam, vec, max(abs(lam[0]), abs(lam[-1])))
    return _spec[key]


NODES = {"tinyGrid3D": 2, "smallGrid3D": 2, "ladder2": 6}


# ---------------------------------------------------------------------------------------------------------------
# 1. the matrix
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nn", [("tinyGrid3D", 1), ("tinyGrid3D", 2), ("smallGrid3D", 1), ("smallGrid3D", 2),
                                     ("smallGrid3D", 5), ("ladder2", 6)])
def test_matrix_against_the_restatement(fixtures_dir, name, nn):
    N, mm, gp, X0, make = instance(fixtures_dir, name)
    d, B = mm.d, mm.d + 1
    n = B * N
    grp, opt = make(nn)
    Aabs, k = abs_terms_operator(N, mm, nn, opt.regularizer)
    perm = pose_major(N, d)
    bM = (2 * k[:, None] * U * Aabs.toarray())[np.ix_(perm, perm)]
    Mref = sp.csr_matrix(gp.M).toarray()[np.ix_(perm, perm)]
    Mcsr = sp.csr_matrix(gp.M)
    Mstruct = (sp.csr_matrix((np.ones(len(Mcsr.data)), Mcsr.indices, Mcsr.indptr), shape=(n, n)).toarray() > 0)[np.ix_(perm, perm)]
    rng = np.random.default_rng(31)
    for what, X, eta in (("chordal", X0, 1e-3), ("random", tc.random_point(rng, N, d), 0.37)):
        ptr, col, val = grp.cert_matrix(X, eta)
        assert ptr.shape == (n + 1,) and ptr[0] == 0 and ptr[-1] == len(col) == len(val)
        assert len(val) % (B * B) == 0
        dev = sp.csr_matrix((val, col, ptr), shape=(n, n))
        assert np.all(np.diff(ptr) % B == 0)
        stored = sp.csr_matrix((np.ones(len(col)), col, ptr), shape=(n, n)).toarray() > 0
        assert int(stored.sum()) == len(col)   # (no entry twice)
        # dense B x B blocks: every stored block is whole
        blocks = stored.reshape(N, B, N, B).transpose(0, 2, 1, 3).reshape(N, N, B * B)
        assert np.all(blocks.all(axis=2) | ~blocks.any(axis=2))
        assert np.array_equal(stored, stored.T)
        Sref = cr.S_matrix(gp.M, X, d) + eta * sp.identity(n, format="csr")
        Sref = Sref.tocsr()[perm][:, perm].tocsr()
        # its pattern: M's entries, the whole d x d block of every Lambda_p, the diagonal (NOT the entries scipy happens to
        # keep: a difference of sparse matrices drops results that are exactly zero, e.g. an off-diagonal of Lambda_p)
        present = Mstruct | (np.kron(np.eye(N), np.pad(np.ones((d, d)), ((1, 0), (1, 0)))) > 0) | np.eye(n, dtype=bool)
        assert np.all(stored[present]), what                      # every restatement entry is there
        D = dev.toarray()
        assert np.all(D[stored & ~present] == 0.0), what           # what it does not have is exactly zero
        # the bounds
        Lam = cr.lambda_blocks(gp.M, X, d)
        bL = tc.lambda_bound(Aabs, k, gp.M, X, d)
        LamFull, bLFull = np.zeros((n, n)), np.zeros((n, n))
        for g in range(N):
            LamFull[B * g + 1:B * g + B, B * g + 1:B * g + B] = np.abs(Lam[g])
            bLFull[B * g + 1:B * g + B, B * g + 1:B * g + B] = bL[g]
        diag_blk = np.kron(np.eye(N), np.ones((B, B))) > 0
        bound = bM.copy()
        shift = np.abs(eta) * np.eye(n)
        bound[diag_blk] = ((1 + 2 * U) * (bM + bLFull) + 2 * U * (np.abs(Mref) + LamFull + shift))[diag_blk]
        err = np.abs(D - Sref.toarray())
        worst = np.max(err[stored] / np.maximum(bound[stored], 1e-300))
        print(name, nn, what, "worst error / bound = %.3f, entries %d" % (worst, len(val)))
        assert np.all(err <= bound), (what, worst)


# ---------------------------------------------------------------------------------------------------------------
# 2. + 3. the decision on both sides of the threshold, and the pivots
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,which", [("tinyGrid3D", "chordal"), ("tinyGrid3D", "random"), ("smallGrid3D", "chordal"),
                                        ("smallGrid3D", "random"), ("ladder2", "chordal"), ("ladder2", "random")])
def test_decision_on_both_sides_of_the_threshold(fixtures_dir, name, which):
    X, S, lam, _, nS = spectrum(fixtures_dir, name, which)
    assert lam[0] < -1e-6 * nS   # (a point that is not certifiable: the threshold is away from a singular shift)
    grp, _ = instance(fixtures_dir, name)[4](NODES[name])
    below = grp.cert_factor(X, eta=-lam[0] - 1e-8 * nS)
    above = grp.cert_factor(X, eta=-lam[0] + 1e-8 * nS)
    far = grp.cert_factor(X, eta=-lam[0] + 0.5 * nS)
    print(name, which, "lambda_min %.6e |S| %.6e" % (lam[0], nS), "pivots above: %.6e .. %.6e" % (above.pivot_min, above.pivot_max),
          "far: %.6e .. %.6e" % (far.pivot_min, far.pivot_max), "fronts %d levels %d max_front %d entries %d bytes %d" %
          (above.fronts, above.levels, above.max_front, above.factor_entries, above.factor_bytes))
    assert below.outcome == NOT_PD
    assert above.outcome == PD and far.outcome == PD
    for f in (above, far):
        lo, hi = lam[0] + f.eta, lam[-1] + f.eta   # the spectrum of S + eta I
        # pivots are diagonal entries of Schur complements of S + eta I: inside its spectrum
        assert f.pivot_min > 0
        assert f.pivot_min >= lo * (1 - 1e-9) - 1e-10 * nS
        assert f.pivot_max <= hi * (1 + 1e-9)
        assert f.pivot_min <= f.pivot_max
    for f in (below, above, far):
        assert f.fronts > 0 and f.levels > 0 and f.factor_entries > 0 and f.factor_bytes > 0 and f.numeric_s > 0
        assert abs(f.stationarity - np.linalg.norm(S @ X)) <= 1e-9 * max(np.linalg.norm(S @ X), 1.0)


# ---------------------------------------------------------------------------------------------------------------
# 4. more than one level
# ---------------------------------------------------------------------------------------------------------------
def test_elimination_tree_shapes(fixtures_dir):
    """smallGrid3D (500 unknowns) is a tree of fronts -- so the tests above cover the assembly of Schur complements between
    fronts -- and tinyGrid3D (36 unknowns) the single front."""
    for name, nn in (("smallGrid3D", 1), ("smallGrid3D", 2), ("smallGrid3D", 5)):
        N, mm, gp, X0, make = instance(fixtures_dir, name)
        f = make(nn)[0].cert_factor(X0, eta=1e-3)
        assert f.levels >= 3 and f.fronts >= 4, (f.levels, f.fronts)
        assert f.max_front < 4 * N and f.factor_entries >= 4 * N
        assert f.symbolic_s > 0
    N, mm, gp, X0, make = instance(fixtures_dir, "tinyGrid3D")
    f = make(2)[0].cert_factor(X0, eta=1e-3)
    assert (f.fronts, f.levels, f.max_front, f.factor_entries) == (1, 1, 36, 36 * 36)


# ---------------------------------------------------------------------------------------------------------------
# 5. failure, then success, in one group; nothing on stderr
# ---------------------------------------------------------------------------------------------------------------
CHILD = r"""
import json, os, sys, tempfile
import numpy as np
sys.path.insert(0, sys.argv[1])
import dpgo_amd
z = np.load(sys.argv[2])
Xa, Xb = z["Xa"], z["Xb"]

def group():
    opt = dpgo_amd.Options.driver(0, True, max_iterations=0)
    return dpgo_amd.NodeGroup(dpgo_amd.read_g2o(sys.argv[3], 2), range(2), opt)

grp, fresh = group(), group()
sys.stderr.flush()
keep = os.dup(2)
tmp = tempfile.TemporaryFile()
os.dup2(tmp.fileno(), 2)
try:
    out = [grp.cert_factor(Xa, 1e-3), grp.cert_factor(Xb, 1e-3), grp.cert_factor(Xa, 1e-3), fresh.cert_factor(Xb, 1e-3)]
finally:
    os.dup2(keep, 2)
tmp.seek(0)
print(json.dumps(dict(stderr=tmp.read().decode(), outcome=[f.outcome for f in out], pmin=[f.pivot_min.hex() for f in out],
                      pmax=[f.pivot_max.hex() for f in out], symbolic=[f.symbolic_s for f in out])))
"""


def test_failure_then_success_in_one_group(fixtures_dir, tmp_path):
    """A fresh group is asked about a point that is not certifiable first (smallGrid3D's chordal point, lambda_min = -1.22),
    then about one that is (its converged run), then about the first again."""
    path = tc.problem(fixtures_dir, "smallGrid3D")[0]
    Xa = tc.problem(fixtures_dir, "smallGrid3D")[4]
    Xb = tc.converged(fixtures_dir, "smallGrid3D")
    np.savez(tmp_path / "points.npz", Xa=Xa, Xb=Xb)
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    run = subprocess.run([sys.executable, str(script), ROOT, str(tmp_path / "points.npz"), path], capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    r = json.loads(run.stdout.strip().splitlines()[-1])
    assert r["outcome"] == [NOT_PD, PD, NOT_PD, PD]
    assert r["stderr"] == ""                                   # the quiet switch: a failed pivot is a verdict
    assert "pivot" not in run.stderr
    a = np.array([float.fromhex(r["pmin"][1]), float.fromhex(r["pmax"][1])])
    b = np.array([float.fromhex(r["pmin"][3]), float.fromhex(r["pmax"][3])])
    assert np.array_equal(a, b) and a[0] > 0                   # the failed call left nothing behind
    assert r["symbolic"][0] > 0 and r["symbolic"][1] == 0 and r["symbolic"][2] == 0   # analysed once


# ---------------------------------------------------------------------------------------------------------------
# 6. the refuted evidence
# ---------------------------------------------------------------------------------------------------------------
def test_converged_ritz_pair_is_refuted_by_the_factorisation(fixtures_dir):
    """smallGrid3D's chordal point, started on the eigenvectors of the first clearly positive eigenvalues of S: the search
    converges at once to theta = 0.7524 and calls it NONNEGATIVE although lambda_min = -1.22 -- the documented limit of
    the search, which the restatement shows too.  The factorisation refutes it."""
    X, S, lam, vec, nS = spectrum(fixtures_dir, "smallGrid3D", "chordal")
    N, mm, gp, X0, make = instance(fixtures_dir, "smallGrid3D")
    assert lam[0] < -1.0 and lam[3] < 1e-9 * nS < 0.5 < lam[4]
    V0, eta = np.ascontiguousarray(vec[:, 4:7]), 0.61
    grp, _ = make(2)
    ref = cr.lobpcg(gp.M, X, 3, V0, eta=eta)
    assert ref["status"] == cr.NONNEGATIVE
    res, x = grp.certify(X, eta=eta, V0=V0)
    print("certify:", dpgo_amd.CERT_NAMES[res.status], res.iterations, res.theta, res.residual)
    assert res.status == dpgo_amd.CERT_NONNEGATIVE
    assert abs(res.theta - lam[4]) <= 1e-6 * nS
    ver, xv, fac = grp.verify(X, eta=eta, V0=V0)
    print("verify:", dpgo_amd.CERT_NAMES[ver.status], dpgo_amd.CERT_FACTOR_NAMES[fac.outcome], ver.iterations, ver.theta, ver.residual)
    assert fac.outcome == NOT_PD and ver.status == dpgo_amd.CERT_UNDECIDED
    assert (ver.theta, ver.residual, ver.iterations) == (res.theta, res.residual, res.iterations)   # kept
    assert np.array_equal(xv, x)
    # a Gaussian start finds the direction
    neg, xn, fac2 = grp.verify(X, eta=eta, seed=3)
    assert fac2.outcome == NOT_PD and neg.status == dpgo_amd.CERT_NEGATIVE
    assert float(xn @ (S @ xn)) < -0.5 * eta


# ---------------------------------------------------------------------------------------------------------------
# 7. decisions on the project's points
# ---------------------------------------------------------------------------------------------------------------
def test_decisions_on_the_converged_small_fixtures(fixtures_dir):
    """The tinyGrid3D run is NOT certified (lambda_min = -3.65): NEGATIVE, by the search.  The smallGrid3D run is PROVEN, by
    the factorisation alone."""
    X, S, lam, _, nS = spectrum(fixtures_dir, "tinyGrid3D", "converged")
    grp, _ = instance(fixtures_dir, "tinyGrid3D")[4](2)
    res, x, fac = grp.verify(X)
    assert fac.outcome == NOT_PD and res.status == dpgo_amd.CERT_NEGATIVE and res.iterations > 0
    assert float(x @ (S @ x)) < -0.5e-3
    X, S, lam, _, nS = spectrum(fixtures_dir, "smallGrid3D", "converged")
    assert lam[0] > -1e-6
    Xc = tc.problem(fixtures_dir, "smallGrid3D")[4]
    for nn in (1, 2, 5):
        grp, _ = instance(fixtures_dir, "smallGrid3D")[4](nn)
        res, x, fac = grp.verify(X)
        print("smallGrid3D converged", nn, dpgo_amd.CERT_NAMES[res.status], fac.pivot_min, fac.pivot_max, res.stationarity)
        assert fac.outcome == PD and res.status == dpgo_amd.CERT_PROVEN
        assert res.iterations == 0 and res.theta == 0 and res.residual == 0 and not x.any()
        assert res.stationarity < 1e-3 and res.stationarity == fac.stationarity
        assert 0 < fac.pivot_min <= fac.pivot_max <= (lam[-1] + 1e-3) * (1 + 1e-9)
        assert grp.cert_factor(Xc, eta=1e-3).outcome == NOT_PD   # the chordal point: lambda_min = -1.22
        res, x, fac = grp.verify(Xc)
        assert fac.outcome == NOT_PD and res.status == dpgo_amd.CERT_NEGATIVE


@pytest.mark.parametrize("name,nn,eta,want", [("torus3D", 8, 1e-3, NOT_PD), ("sphere2500", 4, 1e-3, PD), ("sphere2500", 4, 1e-5, NOT_PD)])
def test_decisions_at_the_chordal_points(fixtures_dir, name, nn, eta, want):
    """Against the eigenvalues DESIGN 12 records: torus3D's chordal point has lambda_min far below -1e-3; sphere2500's has
    lambda_min = -5.65e-4, so S + 1e-3 I IS positive definite -- at a point with |S X|_F = 265 that is no minimum at all:
    the warning example of the header.  S + 1e-5 I is not."""
    path, N, mm, gp, X0 = tc.problem(fixtures_dir, name)
    grp, _ = tc.group(path, nn)
    f = grp.cert_factor(X0, eta=eta)
    print(name, nn, eta, dpgo_amd.CERT_FACTOR_NAMES[f.outcome], "pivots %.6e .. %.6e" % (f.pivot_min, f.pivot_max), "stationarity %.6e" % f.stationarity,
          "fronts %d levels %d max_front %d entries %d bytes %d symbolic %.3f s numeric %.4f s" %
          (f.fronts, f.levels, f.max_front, f.factor_entries, f.factor_bytes, f.symbolic_s, f.numeric_s))
    assert f.outcome == want
    if name == "sphere2500":
        assert f.stationarity > 1
    if want == PD:
        assert f.pivot_min > 0
        res, x, f2 = grp.verify(X0, eta=eta)
        assert res.status == dpgo_amd.CERT_PROVEN and res.iterations == 0 and res.stationarity > 1


# ---------------------------------------------------------------------------------------------------------------
# 8. SKIPPED
# ---------------------------------------------------------------------------------------------------------------
def test_skipped_is_todays_answer(fixtures_dir):
    path, N, mm, gp, X0 = tc.problem(fixtures_dir, "smallGrid3D")
    grp, _ = tc.group(path, 2)
    f = grp.cert_factor(X0, max_factor_bytes=1)
    assert f.outcome == SKIPPED and f.factor_entries > 0 and f.factor_bytes > 1 and f.fronts >= 4 and f.levels >= 3
    assert f.pivot_min == 0 and f.pivot_max == 0 and f.numeric_s == 0 and f.stationarity > 0
    for X in (X0, tc.converged(fixtures_dir, "smallGrid3D")):
        want, xw = grp.certify(X)
        got, xg, fac = grp.verify(X, max_factor_bytes=1)
        assert fac.outcome == SKIPPED
        for name, _ in dpgo_amd.CertResult._fields_:
            assert getattr(got, name) == getattr(want, name), name
        assert np.array_equal(xg, xw)
    assert want.status == dpgo_amd.CERT_NONNEGATIVE   # (not downgraded: nothing refuted it)
    # a cap that is large enough, afterwards, in the same group
    assert grp.cert_factor(X0, max_factor_bytes=f.factor_bytes).outcome == NOT_PD
    assert grp.cert_factor(X0, max_factor_bytes=f.factor_bytes - 1).outcome == SKIPPED


# ---------------------------------------------------------------------------------------------------------------
# 9. the optimiser is not disturbed
# ---------------------------------------------------------------------------------------------------------------
def test_verify_does_not_disturb_the_optimiser(fixtures_dir):
    """30 AMM-PGO# iterations with a verify call after every fifth: bit for bit the run without."""
    path = tc.problem(fixtures_dir, "smallGrid3D")[0]
    runs = []
    for with_cert in (False, True):
        drv = dpgo_amd.DistPGO(dpgo_amd.read_g2o(path, 2), dpgo_amd.Options.driver(LOSS_NONE, True))
        trace = []
        for it in range(30):
            assert drv.step() == 0
            if with_cert and it % 5 == 4:
                res, _, fac = drv.group.verify(drv.X(), max_iters=40)
                assert fac.outcome != SKIPPED and (res.iterations > 0 or res.status == dpgo_amd.CERT_PROVEN)
            trace.append([getattr(drv.group.results(a), f) for a in range(2) for f in ("fobj", "gamma", "gradFnorm", "Gk")])
        runs.append((np.array(drv.X()), [drv.group[a].Xk() for a in range(2)], np.array(trace)))
    assert np.array_equal(runs[0][0], runs[1][0])
    for a in range(2):
        assert np.array_equal(runs[0][1][a], runs[1][1][a])
    assert np.array_equal(runs[0][2], runs[1][2])


# ---------------------------------------------------------------------------------------------------------------
# 10. refusals
# ---------------------------------------------------------------------------------------------------------------
def test_refusals(fixtures_dir):
    path, N, mm, gp, X0 = tc.problem(fixtures_dir, "smallGrid3D")
    G = dpgo_amd.read_g2o(path, 2)

    def every_entry(grp, X):
        for call in (lambda: grp.cert_factor(X), lambda: grp.verify(X), lambda: grp.cert_matrix(X, 1e-3)):
            with pytest.raises(RuntimeError):
                call()

    hub = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(dpgo_amd.LOSS_HUBER, True), X0=X0)
    every_entry(hub.group, X0)                                                                   # a robust loss
    assert hub.step() == 0
    every_entry(dpgo_amd.NodeGroup(G, [0], dpgo_amd.Options.driver(LOSS_NONE, True)), X0)        # one of two nodes
    drv = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(LOSS_NONE, True), X0=X0)
    every_entry(drv.group, X0[:-1])                                                              # a short X
    with pytest.raises(ValueError):
        drv.group.verify(X0, V0=X0[:, :2])
    with pytest.raises(RuntimeError):
        drv.group.cert_factor(X0, eta=float("nan"))
    with pytest.raises(RuntimeError):
        drv.group.verify(X0, eta=-1.0)
    import ctypes as C
    L, Xf = dpgo_amd.lib(), np.asfortranarray(X0)
    o, r, f = dpgo_amd.CertOptions(), dpgo_amd.CertResult(), dpgo_amd.CertFactor()
    assert L.dpgo_group_verify(drv.group._h, dpgo_amd._dp(Xf), Xf.shape[0], C.byref(o), 0, dpgo_amd._dp(Xf), Xf.shape[0] - 1,
                               C.byref(r), None, 0, C.byref(f)) == -1                            # a short V0
    nnz = C.c_longlong(0)
    assert L.dpgo_group_cert_matrix(drv.group._h, dpgo_amd._dp(Xf), Xf.shape[0], 1e-3, None, None, None, 0, C.byref(nnz)) == 0
    ptr, col, val = np.zeros(4 * N + 1, np.int32), np.zeros(nnz.value, np.int32), np.zeros(nnz.value)
    assert L.dpgo_group_cert_matrix(drv.group._h, dpgo_amd._dp(Xf), Xf.shape[0], 1e-3, dpgo_amd._ip(ptr), dpgo_amd._ip(col),
                                    dpgo_amd._dp(val), nnz.value - 1, C.byref(nnz)) == -1        # a short value array
    assert not val.any()
    assert drv.step() == 0 and drv.step() == 0
    res, _, fac = drv.group.verify(X0)
    assert res.status == dpgo_amd.CERT_NEGATIVE and fac.outcome == NOT_PD


# ---------------------------------------------------------------------------------------------------------------
# 11. the facade and the driver
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,iters,want,outcome", [("smallGrid3D", 200, "PROVEN", "PD"), ("tinyGrid3D", 100, "NEGATIVE", "NOT_PD")])
def test_cpp_facade_fast_verification(fixtures_dir, name, iters, want, outcome):
    """examples/facade_mm.cpp with `verify` as its sixth argument: DPGOHashGroup::fast_verification after the loop, one line
    on stderr, stdout the same trace as without."""
    exe = os.path.join(ROOT, "dpgo_amd", "facade_mm")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    args = [exe, os.path.join(fixtures_dir, name + ".g2o"), "2", str(iters), "trivial", "1"]
    plain = subprocess.run(args, check=True, capture_output=True, text=True, timeout=300)
    out = subprocess.run(args + ["verify"], check=True, capture_output=True, text=True, timeout=300)
    assert out.stdout == plain.stdout and "verification" not in plain.stderr
    lines = [l for l in out.stderr.splitlines() if l.startswith("verification: ")]
    assert len(lines) == 1, out.stderr[-2000:]
    assert "pivot" not in out.stderr.replace(lines[0], "") and "certificate: " not in out.stderr
    f = lines[0].split()
    assert len(f) == 8 and f[1] == want and f[2] == outcome
    pivot_min, theta, residual, its, stat = float(f[3]), float(f[4]), float(f[5]), int(f[6]), float(f[7])
    assert stat < 1e-3 and residual >= 0
    if want == "PROVEN":
        assert pivot_min > 0 and its == 0 and theta == 0 and residual == 0
    else:
        assert its > 0 and theta < -0.5e-3


def test_dist_pgo_verify_flag(fixtures_dir, tmp_path):
    """--verify adds one line after the summary (after --certify's, when both are given); without it stdout and the result
    files are what they were."""
    exe = os.path.join(ROOT, "dpgo_amd", "dist_pgo")
    base = [exe, "--dataset", os.path.join(fixtures_dir, "smallGrid3D.g2o"), "--num_nodes", "2", "--iters", "200", "--dist_init", "false"]
    outs = {}
    for tag, extra in (("plain", []), ("verify", ["--verify"]), ("both", ["--certify", "--verify"])):
        cwd = tmp_path / tag
        cwd.mkdir()
        outs[tag] = (subprocess.run(base + extra, capture_output=True, text=True, cwd=cwd, timeout=300), cwd)
        assert outs[tag][0].returncode == 0, outs[tag][0].stderr[-2000:]

    def steady(text):   # (the summary's wall time differs from run to run)
        return [l for l in text.splitlines() if not l.startswith(("time: ", "certificate: ", "verification: "))]

    assert steady(outs["plain"][0].stdout) == steady(outs["verify"][0].stdout) == steady(outs["both"][0].stdout)
    assert "verification" not in outs["plain"][0].stdout and "certificate" not in outs["verify"][0].stdout
    for tag in ("verify", "both"):
        text = outs[tag][0].stdout.rstrip().splitlines()
        lines = [l for l in text if l.startswith("verification: ")]
        assert len(lines) == 1 and text[-1] == lines[0]
        f = lines[0].split()
        assert len(f) == 8 and f[1] == "PROVEN" and f[2] == "PD" and float(f[3]) > 0 and int(f[6]) == 0 and float(f[7]) < 1e-3
        assert "pivot" not in outs[tag][0].stderr
    both = outs["both"][0].stdout.rstrip().splitlines()
    cert = [l for l in both if l.startswith("certificate: ")]
    assert len(cert) == 1 and both[-2] == cert[0] and cert[0].split()[1] == "NONNEGATIVE"
    a = open(outs["plain"][1] / "estimates_trivial.txt").read()
    for tag in ("verify", "both"):
        assert a == open(outs[tag][1] / "estimates_trivial.txt").read()
    # a robust loss: the line says why there is no verification
    hub = subprocess.run(base[:-4] + ["--iters", "5", "--dist_init", "false", "--loss", "huber", "--verify", "--save", "false"],
                         capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert hub.returncode == 0 and "verification: not computed" in hub.stdout
