"""Host side of the Hessian modes (dpgo_amd/csrc/modes.h): the numpy restatement (tests/modes_restatement.py) against
numpy.linalg.eigvalsh of the anchored Hessian with the anchor's rows struck out, the constant of the rounding allowance, the
hash start's properties, the host's eigenproblem (modes_ritz through dpgo_amd.modes_ritz_debug) against scipy's generalised
eigh, and the argument checks of the C ABI.  No GPU.

Inputs: tinyGrid3D and smallGrid3D at their polished points, synthetic.twisted_ring(d, 12) for d = 2, 3 at its local minimum
(tests/test_staircase_host.py: ring12), the compacted synthetic.ladder(d = 2) of tests/test_gpu_cert_proof.py (403 poses, 1209
unknowns) at its polished point, and one indefinite point: tinyGrid3D's chordal point with every rotation replaced by a seeded
random one (cov_restatement.random_rotations_point, seed 5; lambda_0 = -246 with hmax = 300).  With the shift rule
mu = max(10 mu, 1e-3 hmax) that point is factored at mu = hmax and the default 100 iterations serve k = 8 (58 are taken); the
same construction on smallGrid3D needs 103 to 191 iterations for k = 4 and 8 and is not used.

The rounding allowance C n u hmax.  A computed lambda_j differs from the j-th eigenvalue by at most the residual (the matrix
is symmetric) plus what fp64 adds to the value and to the residual's own recurrence.  C is fixed here, before any device is
asked: per input and k the GAP is the larger of |values_fp64 - values_ld| (the restatement in fp64 against the restatement
whose solves, products and Rayleigh quotients run in long double) and | |H v - lambda v|_ld - residual_fp64 | (what long double
says of the pairs the fp64 run reports against what that run says itself), in units of n u hmax.  The largest gap over the
inputs is 0.142 (tinyGrid3D's indefinite point, k = 8; the polished points stay below 0.07); times the margin of 4 that is 0.57,
and C = 1 is the smallest power of two above it.  test_rounding_allowance asserts 4 gap <= C on every input.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import scipy.linalg as sla

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_restatement as cr  # noqa: E402
import modes_restatement as mr  # noqa: E402
import newton_restatement as nr  # noqa: E402
import test_certify_host as tch  # noqa: E402  (its iteration counts; none of its tests is imported)
import test_polish_host as tph  # noqa: E402  (its points; none of its tests is imported)
import test_staircase_host as tsh  # noqa: E402  (the rings; none of its tests is imported)

import dpgo_amd  # noqa: E402

U = 2.0 ** -53
C_ROUND = 1.0
KS = (1, 4, 8)
INPUTS = ["tinyGrid3D", "smallGrid3D", "ring2", "ring3", "ladder2", "tinyGrid3D-indefinite"]
INDEFINITE_SEED = 5
_inputs = {}


def point(fixtures_dir, name):
    """(M, X, d) of a named input: computed once."""
    if name not in _inputs:
        if name in ("tinyGrid3D", "smallGrid3D"):
            gp, X = tph.start_point(fixtures_dir, name, tch.ITERS[name])
            r = nr.polish_full(gp.M, X, gp.d)
            assert r["outcome"] == nr.CONVERGED
            _inputs[name] = (gp.M, r["X"], gp.d)
        elif name in ("ring2", "ring3"):
            gp, mm, g, Xt, Xc = tsh.ring12(int(name[-1]))
            _inputs[name] = (gp.M, Xt, gp.d)
        elif name == "ladder2":
            gp, X = tph.start_point(fixtures_dir, name, 300)
            r = nr.polish_full(gp.M, X, gp.d)
            assert r["outcome"] == nr.CONVERGED
            _inputs[name] = (gp.M, r["X"], gp.d)
        else:
            gp, X = tph.start_point(fixtures_dir, "tinyGrid3D", "chordal")
            _inputs[name] = (gp.M, cr.random_rotations_point(X, gp.d, INDEFINITE_SEED), gp.d)
    return _inputs[name]


_dense = {}


def dense(fixtures_dir, name, anchor=0):
    """Once per input: the restated anchored Hessian, n, dof, hmax and the ascending eigenvalues without the anchor's rows."""
    key = (name, anchor)
    if key not in _dense:
        M, X, d = point(fixtures_dir, name)
        dof = cr.dof_of(d)
        A = nr.anchored_hessian(M, X, d, anchor)
        _dense[key] = dict(A=A, n=A.shape[0], d=d, dof=dof, hmax=mr.hmax_of(A, anchor, dof), lam=mr.spectrum(A, anchor, dof), X=X, M=M)
    return _dense[key]


_runs = {}


def restated(fixtures_dir, name, k, ld=False):
    key = (name, k, ld)
    if key not in _runs:
        D = dense(fixtures_dir, name)
        _runs[key] = mr.iterate(D["A"], 0, D["dof"], k, ld=ld)
    return _runs[key]


def allowance(D):
    return C_ROUND * D["n"] * U * D["hmax"]


@pytest.mark.parametrize("name", INPUTS)
def test_spectrum_against_eigvalsh(fixtures_dir, name):
    D = dense(fixtures_dir, name)
    lam, hmax = D["lam"], D["hmax"]
    if name.endswith("indefinite"):
        assert lam[0] < -1e-3 * hmax
    else:
        assert lam[0] > 0
    for k in KS:
        r = restated(fixtures_dir, name, k)
        err = np.abs(r["values"] - lam[:k])
        true = mr.true_residuals(D["A"], r["values"], r["vectors"])
        print("%s k = %d: %d iterations, %d shift tries, mu %.4g, lambda_0 %.6g, lambda_k-1 %.6g, worst error / (residual + allowance) "
              "%.3g, residual %.3g, true residual %.3g, decisive %s" %
              (name, k, r["iterations"], r["shift_tries"], r["mu"], r["values"][0], r["values"][-1],
               float((err / (r["residuals"] + allowance(D))).max()), r["residuals"].max(), true.max(),
               mr.decisive(r["history"], k, 1e-8 * hmax)))
        assert r["outcome"] == mr.CONVERGED and r["block"] == 16
        assert np.all(r["residuals"] <= 1e-8 * hmax)
        assert np.all(err <= r["residuals"] + allowance(D))
        assert np.all(true <= r["residuals"] + allowance(D))
        assert np.all(np.diff(r["values"]) >= -2 * allowance(D))
        G = r["vectors"] @ r["vectors"].T
        assert np.abs(G - np.eye(k)).max() <= 8 * (D["n"] + 16 * 16) * U
        assert not r["vectors"][:, :D["dof"]].any()
        assert r["negative"] == int(np.sum(lam[:k] < 0))
        if name.endswith("indefinite"):
            assert r["shift_tries"] >= 1 and r["mu"] > 0 and r["negative"] >= 1
        else:
            assert r["shift_tries"] == 0 and r["mu"] == 0.0 and r["factorisations"] == 1


@pytest.mark.parametrize("name", INPUTS)
def test_rounding_allowance(fixtures_dir, name):
    """The constant of the module docstring: 4 x the gap between the fp64 and the long-double restatement stays within C.  The
    long-double run is taken at k = 8 everywhere (the widest report) and at every k on the inputs below 100 unknowns."""
    D = dense(fixtures_dir, name)
    unit = D["n"] * U * D["hmax"]
    worst = 0.0
    for k in (KS if D["n"] < 100 else (8,)):
        r, rl = restated(fixtures_dir, name, k), restated(fixtures_dir, name, k, ld=True)
        assert rl["outcome"] == mr.CONVERGED and rl["iterations"] == r["iterations"]
        true = mr.true_residuals(D["A"], r["values"], r["vectors"])
        gap = max(float(np.abs(r["values"] - rl["values"]).max()), float(np.abs(true - r["residuals"]).max())) / unit
        print("%s k = %d: gap %.3g n u hmax" % (name, k, gap))
        worst = max(worst, gap)
    assert 4 * worst <= C_ROUND, worst


def test_indefinite_seed_is_clearly_indefinite(fixtures_dir):
    D = dense(fixtures_dir, "tinyGrid3D-indefinite")
    assert D["lam"][0] < -1e-3 * D["hmax"] and D["lam"][0] < -0.5 * D["hmax"]


# ---------------------------------------------------------------------------------------------------------------
# the start block
# ---------------------------------------------------------------------------------------------------------------
def entry_by_hand(seed, i, j):
    """modes_start_entry with Python integers."""
    m64 = (1 << 64) - 1
    z = (seed + 0x9E3779B97F4A7C15 * (64 * i + j + 1)) & m64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m64
    z = z ^ (z >> 31)
    m = 2 * (z >> 12) + 1 - (1 << 52)
    assert abs(m) < (1 << 52) and m % 2 == 1
    return float(m) / float(1 << 52)


def test_start_block():
    V = mr.start_block(1030, 64, seed=1, anchor_row0=12, dof=6)
    assert V.shape == (1030, 64) and not V[12:18].any()
    free = np.ones(1030, bool)
    free[12:18] = False
    assert np.all(np.abs(V[free]) < 1.0) and np.all(V[free] != 0.0)
    for i, j in ((0, 0), (0, 63), (1, 0), (11, 5), (18, 17), (1029, 63)):
        assert V[i, j] == entry_by_hand(1, i, j)
    # a column does not depend on b, a row not on n; another seed is another block
    assert np.array_equal(mr.start_block(300, 16, 1), mr.start_block(1030, 64, 1)[:300, :16])
    assert np.array_equal(mr.start_block(40, 32, 7, 0, 3)[3:], mr.start_block(40, 32, 7)[3:])
    assert not np.array_equal(mr.start_block(40, 16, 1), mr.start_block(40, 16, 2))
    # balanced and uncorrelated enough to start from: the mean of 65920 entries of variance 1/3 within five deviations
    assert abs(mr.start_block(1030, 64, 3).mean()) < 5 * np.sqrt(1.0 / 3.0 / 65920)
    W = mr.start_block(1030, 16, 1)
    Gn = W.T @ W / (1030 / 3.0)
    assert np.linalg.cond(Gn) < 2.0


# ---------------------------------------------------------------------------------------------------------------
# the host's eigenproblem
# ---------------------------------------------------------------------------------------------------------------
def pencil(rng, b, n=200):
    """G = W'W, T = W'A W for a random tall W and a random symmetric A: a pencil as the iteration meets it."""
    W = rng.standard_normal((n, b)) * np.exp(rng.uniform(-2, 2, b))[None, :]
    A = rng.standard_normal((n, n))
    A = 0.5 * (A + A.T)
    return W.T @ W, W.T @ A @ W


@pytest.mark.parametrize("b", [1, 9, 16, 17, 64])
def test_ritz_hook_against_scipy(b):
    rng = np.random.default_rng(400 + b)
    for _ in range(5):
        G, T = pencil(rng, b)
        theta, Cm, used = dpgo_amd.modes_ritz_debug(G, T)
        assert used == b and theta.shape == (b,) and np.all(np.diff(theta) >= 0)
        want = sla.eigh(T, G, eigvals_only=True)
        ds = 1.0 / np.sqrt(np.diag(G))
        kappa = float(np.linalg.cond(G * ds[:, None] * ds[None, :]))
        tol = 8 * b * b * U * kappa * float(np.abs(want).max())
        print("order %d: kappa of the scaled G %.3g, worst |theta - eigh| %.3g, tolerance %.3g" % (b, kappa, np.abs(theta - want).max(), tol))
        assert np.abs(theta - want).max() <= tol
        assert np.abs(Cm.T @ G @ Cm - np.eye(b)).max() <= 8 * b * b * U * kappa
        assert np.abs(Cm.T @ T @ Cm - np.diag(theta)).max() <= tol
        # only the lower triangles are read
        G2, T2 = np.tril(G) + 7.0 * np.triu(np.ones((b, b)), 1), np.tril(T) - 3.0 * np.triu(np.ones((b, b)), 1)
        th2, C2, u2 = dpgo_amd.modes_ritz_debug(G2, T2)
        assert u2 == b and np.array_equal(th2, theta) and np.array_equal(C2, Cm)
        # the restatement's twin
        th3, C3, u3 = mr.ritz(G, T)
        assert u3 == b and np.abs(th3 - theta).max() <= tol


@pytest.mark.parametrize("b,p", [(9, 8), (16, 5), (17, 16), (64, 40)])
def test_ritz_hook_drops_a_nearly_dependent_column(b, p):
    """Column p of W is a combination of the columns before it up to 1e-9: the scaled pivot is 1e-18, below 1e-12, and the
    columns p ... b - 1 are dropped -- used = p, the leading p x p problem solved, the others carried as e_j / sqrt(G_jj)."""
    rng = np.random.default_rng(900 + b)
    n = 200
    W = rng.standard_normal((n, b))
    W[:, p] = W[:, :p] @ rng.standard_normal(p) + 1e-9 * rng.standard_normal(n)
    A = rng.standard_normal((n, n))
    A = 0.5 * (A + A.T)
    G, T = W.T @ W, W.T @ A @ W
    theta, Cm, used = dpgo_amd.modes_ritz_debug(G, T)
    assert used == p and theta.shape == (p,)
    want = sla.eigh(T[:p, :p], G[:p, :p], eigvals_only=True)
    ds = 1.0 / np.sqrt(np.diag(G))
    kappa = float(np.linalg.cond((G * ds[:, None] * ds[None, :])[:p, :p]))
    assert np.abs(theta - want).max() <= 8 * p * p * U * kappa * float(np.abs(want).max())
    assert not Cm[p:, :p].any() and not Cm[:p, p:].any()
    assert np.array_equal(Cm[p:, p:], np.diag(ds[p:]))
    assert mr.ritz(G, T)[2] == p
    # nothing positive on the diagonal: refused
    with pytest.raises(RuntimeError):
        dpgo_amd.modes_ritz_debug(np.zeros((4, 4)), np.eye(4))


# ---------------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------------
def test_modes_abi():
    o = dpgo_amd.ModesOptions()
    assert (o.guard, o.max_iters, o.max_tries, o.want_escape, o.rel_tol, o.shift, o.seed) == (4, 100, 8, 0, 1e-8, 0.0, 1)
    assert (mr.DEFAULTS["guard"], mr.DEFAULTS["max_iters"], mr.DEFAULTS["max_tries"], mr.DEFAULTS["rel_tol"], mr.DEFAULTS["shift"],
            mr.DEFAULTS["seed"]) == (4, 100, 8, 1e-8, 0.0, 1)
    assert (dpgo_amd.MODES_CONVERGED, dpgo_amd.MODES_MAX_ITERS, dpgo_amd.MODES_STALLED, dpgo_amd.MODES_SKIPPED) == (0, 1, 2, 3)
    assert (mr.CONVERGED, mr.MAX_ITERS, mr.STALLED, mr.SKIPPED) == (0, 1, 2, 3)
    assert [mr.block_of(k) for k in (1, 12, 13, 28, 29, 44, 45, 60)] == [16, 16, 32, 32, 48, 48, 64, 64]
    # four ints, two doubles, a 64-bit seed; twelve ints, a long long, fifteen doubles
    assert C.sizeof(dpgo_amd.ModesOptions) == 16 + 16 + 8
    assert C.sizeof(dpgo_amd.ModesResult) == 48 + 8 + 15 * 8
    L = dpgo_amd.lib()
    X = np.zeros((8, 3), order="F")
    out = np.zeros(64)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    r = dpgo_amd.ModesResult()
    fake = C.c_void_p(0)
    for h in (None, fake):
        assert L.dpgo_group_hessian_modes(h, dp(X), 8, 0, 1, C.byref(o), 0, dp(out), dp(out), dp(out), dp(out), None, C.byref(r)) == -1
    L.dpgo_modes_options_default(None)   # (no crash)
    th, Cm, used = np.zeros(4), np.zeros((4, 4)), C.c_int(0)
    G = np.eye(4)
    assert L.dpgo_debug_modes_ritz_host(4, dp(G), dp(G), dp(th), dp(Cm), C.byref(used)) == 0 and used.value == 4
    assert L.dpgo_debug_modes_ritz_host(0, dp(G), dp(G), dp(th), dp(Cm), C.byref(used)) == -1
    assert L.dpgo_debug_modes_ritz_host(65, dp(G), dp(G), dp(th), dp(Cm), C.byref(used)) == -1
    assert L.dpgo_debug_modes_ritz_host(4, None, dp(G), dp(th), dp(Cm), C.byref(used)) == -1
    assert L.dpgo_debug_modes_ritz_host(4, dp(G), dp(G), None, dp(Cm), C.byref(used)) == -1
    # the kernels' hooks refuse bad shapes before they touch a device
    V = np.zeros((4, 16))
    for n, b, ld in ((0, 16, 16), (4, 8, 16), (4, 24, 24), (4, 80, 80), (4, 16, 15)):
        assert L.dpgo_debug_modes_init(0, n, b, ld, -1, 0, 1, dp(V)) == -1
        assert L.dpgo_debug_modes_gram(0, n, b, ld, dp(V), dp(V), dp(out), dp(out)) == -1
    assert L.dpgo_debug_modes_init(0, 4, 16, 16, -1, 0, 1, None) == -1
    header = open(os.path.join(os.path.dirname(dpgo_amd.__file__), "..", "include", "dpgo_amd.h")).read()
    for sym in ("dpgo_modes_options_default", "dpgo_group_hessian_modes", "dpgo_debug_modes_init", "dpgo_debug_modes_gram",
                "dpgo_debug_modes_update", "dpgo_debug_modes_ritz_host", "dpgo_debug_modes_ritz"):
        assert sym + "(" in header and sym in dpgo_amd.SYMBOLS and hasattr(L, sym)
    for name in ("hessian_modes",):
        assert hasattr(dpgo_amd.NodeGroup, name)
    for name in ("modes_init_debug", "modes_gram_debug", "modes_update_debug", "modes_ritz_debug", "ModesOptions", "ModesResult"):
        assert hasattr(dpgo_amd, name)
    with pytest.raises(TypeError):
        dpgo_amd.ModesOptions(no_such_field=1)
