"""That the comparisons of tests/test_gpu_cert_search.py can fail, and do not fail a correct evaluation (no GPU).

tests/cert_search_checks.py holds a kernel's output to the longdouble step functions of tests/cert_restatement.py within bounds
derived from the operation.  Here the "kernel" is the float64 evaluation of the same step functions:
  * as it is, it stays within every bound on every instance the GPU tests use (the worst error / bound per quantity is printed);
  * with one fault applied to its output -- the faults that an eigenvalue iteration repairs by itself and that cost iterations
    only: one entry of B^T S B taken from its neighbour, the W-P cross block of B^T S B zeroed, two entries of B^T B swapped,
    B_c^T (S B)_a in place of B_a^T (S B)_c, T_p applied without its translation row and column, the old P dropped from P',
    and the T_p of another pose -- the comparison flags the quantity the fault is in, every time."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cert_restatement as cr  # noqa: E402
import cert_search_checks as ck  # noqa: E402
import test_gpu_certify as tc  # noqa: E402  (its inputs and derived bounds; none of its tests is imported)
import test_gpu_cert_proof as tp  # noqa: E402  (the d = 2 instance)

SMALL = [("tinyGrid3D", 1), ("smallGrid3D", 5), ("ladder2", 6)]
ALL = SMALL + [("torus3D", 8)]
XI = tp.OOptions.driver(tp.LOSS_NONE, True).regularizer   # (what the groups of the GPU tests are created with)
_inst = {}


def inst(fixtures_dir, name, nn):
    if name not in _inst:
        N, mm, gp, X0, _ = tp.instance(fixtures_dir, name)
        s = dict(N=N, mm=mm, d=mm.d, gp=gp, X=X0, nn=nn, Lam=cr.lambda_blocks(gp.M, X0, mm.d), T=cr.block_jacobi(gp.M, mm.d))
        s["Aabs"], s["k"] = tc.abs_operator(N, mm, nn, XI)
        _inst[name] = s
    return _inst[name]


def gram64(s, b):
    G, A, SW = cr.gram_step(s["gp"].M, s["Lam"], b["V"], b["W"], b["P"], b["SV"], b["SP"], s["d"], MW=b["MW"])
    return G, A, SW


def update64(s, Cf, theta, b, T):
    return cr.update_step(Cf, theta, b["V"], b["W"], b["P"], b["SV"], b["SW"], b["SP"], T, s["d"])


def restart_C(s, b):
    """The coefficients of a restart: the Rayleigh-Ritz step on the sums of a basis with P = W."""
    G, A, SW = gram64(s, b)
    A3, B3 = ck.ritz_matrices(cr.upper_triangles(G, A), s["d"], 3)
    theta, C, used = cr.rayleigh_ritz(A3, B3, s["d"], 3)
    assert used == 2 and np.all(C[2 * s["d"]:] == 0.0)
    return theta, C, SW


@pytest.mark.parametrize("name,nn", ALL)
def test_the_float64_steps_stay_within_every_bound(fixtures_dir, name, nn):
    s = inst(fixtures_dir, name, nn)
    d, worst, bad = s["d"], {}, []
    rng = np.random.default_rng(40)
    for variant in ("full", "P=0", "W=P=0", "P=W"):
        b = ck.gaussian_blocks(rng, s["X"].shape, variant)
        G, A, SW = gram64(s, b)
        bad += ck.worst(ck.gram_ratios(d, s["Lam"], b, cr.upper_triangles(G, A), SW), worst)
    b = dict(ck.gaussian_blocks(rng, s["X"].shape), MW=None)   # M W formed by either side
    G, A, SW = gram64(s, b)
    r = ck.gram_ratios(d, s["Lam"], b, cr.upper_triangles(G, A), SW, M=s["gp"].M, bMW=tc.prod_bound(s["Aabs"], s["k"], b["W"]))
    bad += ck.worst(dict(("%s (M W formed)" % q, v) for q, v in r.items()), worst)
    for T in (s["T"], None):
        b = ck.gaussian_blocks(rng, s["X"].shape)
        b["SW"] = b.pop("MW")
        Cf, theta = rng.standard_normal((3 * d, d)), rng.standard_normal(d)
        bad += ck.worst(ck.update_ratios(d, Cf, theta, b, update64(s, Cf, theta, b, T), T), worst)
        b = ck.gaussian_blocks(rng, s["X"].shape, "P=W")
        theta, C3, b["SW"] = restart_C(s, b)
        bad += ck.worst(ck.update_ratios(d, C3, theta, b, update64(s, C3, theta, b, T), T), worst)
    # the preconditioner: the restatement's blocks inverted another way (Cholesky, in longdouble)
    ratios = ck.inverse_ratios(s["gp"].M, s["N"], d)
    Mb, _ = ck.pose_blocks(s["gp"].M, s["N"], d)
    Tld = ck.cholesky_inverse_ld(Mb).astype(np.float64)
    bad += ck.worst(dict(T_p=ck.precon_ratio(s["gp"].M, s["Aabs"], s["k"], s["N"], d, Tld, 10 * float(np.max(ratios)))), worst)
    print(name, nn, "inversion ratio %.3g;" % np.max(ratios), "worst error / bound:", " ".join("%s %.3g" % kv for kv in sorted(worst.items())))
    assert not bad, (bad, worst)


def gram_faults(d):
    NT, n3 = ck.ntri(d), 3 * d
    tri = lambda a, c: cr.tri_index(n3, a, c)   # noqa: E731

    def neighbour(G, A):
        A = A.copy()
        A[n3 - 1, n3 - 1] = A[n3 - 2, n3 - 1]
        return G, A

    def cross_block(G, A):
        A = A.copy()
        A[d:2 * d, 2 * d:] = 0.0
        return G, A

    def swap(G, A):
        G = G.copy()
        G[0, 1], G[0, 2] = G[0, 2], G[0, 1]
        return G, A

    def transposed(G, A):
        return G, A.T

    assert tri(0, 0) == 0 and tri(n3 - 1, n3 - 1) == NT - 1
    return [("one entry of B^T S B from its neighbour", neighbour, "BtSB"), ("W-P cross block of B^T S B zeroed", cross_block, "BtSB"),
            ("two entries of B^T B swapped", swap, "BtB"), ("B_c^T (S B)_a in place of B_a^T (S B)_c", transposed, "BtSB")]


@pytest.mark.parametrize("name,nn", ALL)
def test_every_fault_in_the_sums_is_flagged(fixtures_dir, name, nn):
    s = inst(fixtures_dir, name, nn)
    d = s["d"]
    b = ck.gaussian_blocks(np.random.default_rng(41), s["X"].shape)
    G, A, SW = gram64(s, b)
    clean = ck.gram_ratios(d, s["Lam"], b, cr.upper_triangles(G, A), SW)
    assert max(clean.values()) <= 1.0
    for what, fault, where in gram_faults(d):
        Gf, Af = fault(G, A)
        r = ck.gram_ratios(d, s["Lam"], b, cr.upper_triangles(Gf, Af), SW)
        print(name, "%-45s %s error / bound %.3g: detected" % (what, where, r[where]))
        assert r[where] > 1e3, (what, r)
        assert all(v <= 1.0 for q, v in r.items() if q != where), (what, r)   # ... and nothing else is blamed


@pytest.mark.parametrize("name,nn", ALL)
def test_every_fault_in_the_update_is_flagged(fixtures_dir, name, nn):
    s = inst(fixtures_dir, name, nn)
    d, T = s["d"], s["T"]
    rng = np.random.default_rng(42)
    b = ck.gaussian_blocks(rng, s["X"].shape)
    b["SW"] = b.pop("MW")
    Cf, theta = rng.standard_normal((3 * d, d)), rng.standard_normal(d)
    out = update64(s, Cf, theta, b, T)
    assert max(ck.update_ratios(d, Cf, theta, b, out, T).values()) <= 1.0
    # T_p applied without its translation row and column
    Tf = T.copy()
    Tf[:, 0, :] = 0.0
    Tf[:, :, 0] = 0.0
    r = ck.update_ratios(d, Cf, theta, b, dict(out, W=cr.apply_block_jacobi(Tf, out["R"], d)), T)
    print(name, "T_p without its translation row and column: W error / bound %.3g: detected" % r["W"])
    assert r["W"] > 1e3 and all(v <= 1.0 for q, v in r.items() if q != "W"), r
    # the old P dropped from P'
    r = ck.update_ratios(d, Cf, theta, b, dict(out, P=b["W"] @ Cf[d:2 * d]), T)
    print(name, "P' = W C_w: P error / bound %.3g: detected" % r["P"])
    assert r["P"] > 1e3 and all(v <= 1.0 for q, v in r.items() if q != "P"), r
    # ... and from S P' (a stale S P)
    r = ck.update_ratios(d, Cf, theta, b, dict(out, SP=b["SW"] @ Cf[d:2 * d]), T)
    print(name, "S P' = S W C_w: SP error / bound %.3g: detected" % r["SP"])
    assert r["SP"] > 1e3 and all(v <= 1.0 for q, v in r.items() if q != "SP"), r
    # a norm sum that misses one pose
    r = ck.update_ratios(d, Cf, theta, b, dict(out, rr=out["rr"] - out["R"][0] ** 2), T)
    print(name, "|R'|^2 without one row: rr error / bound %.3g: detected" % r["rr"])
    assert r["rr"] > 1e3, r


@pytest.mark.parametrize("name,nn", ALL)
def test_a_wrong_preconditioner_block_is_flagged(fixtures_dir, name, nn):
    s = inst(fixtures_dir, name, nn)
    c = 10 * float(np.max(ck.inverse_ratios(s["gp"].M, s["N"], s["d"])))
    args = (s["gp"].M, s["Aabs"], s["k"], s["N"], s["d"])
    assert ck.precon_ratio(*args, s["T"], c) == 0.0
    r = ck.precon_ratio(*args, np.roll(s["T"], 1, axis=0), c)
    print(name, "T_p of the pose before: error / bound %.3g: detected" % r)
    assert r > 1e3
