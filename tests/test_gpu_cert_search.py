"""The certificate's LOBPCG search on the device kernel by kernel and step by step: k_cert_gram, k_cert_update, k_cert_reduce
(dpgo_amd/csrc/cert.hip) and cert_build_precon (cert.cpp), through the hooks of dpgo_amd/csrc/debug_cert.cpp, against the
step functions of tests/cert_restatement.py evaluated in np.longdouble on the same input bits.  The bounds, and where they come
from, are in tests/cert_search_checks.py; tests/test_cert_search_host.py shows that each of them flags a wrong kernel.

The search repairs its own mistakes -- a wrong Gram entry, a stale S P or a wrong preconditioner cost iterations and nothing
else -- so the tests of its result (tests/test_gpu_certify.py) cannot see them.  Here every sum, every entry of the
recurrences and every block of the preconditioner is compared, and the production loop is tied to the hooks: a traced run of
certify must agree bit for bit, pass by pass, with the same passes made from the hooks.

Instances: tinyGrid3D on 1 node (one segment, 9 live lanes) and on 9 (nine segments of one row), smallGrid3D on 5 nodes
(d = 3, five partly filled segments), ladder2 on 6 nodes (d = 2 -- wave_store_sums<21, 24> --; test_gpu_cert_proof.instance
compacts the ladder's pose ids, and the contiguous partition of the 403 poses gives own sizes 68 / 67 x 5, NOT the generator's
81 / 1 / 63 / 64 / 65 / 129: twelve segments, a full one and one of 4 or 3 rows per node) and, for k_cert_reduce's strided
loop, torus3D on 8 nodes (80 segments: a second round).

The inversion constant of the preconditioner's bound is measured when the tests run (cert_search_checks.inverse_ratios):
the worst |numpy inverse - longdouble Cholesky inverse| / (u kappa_2 |T_p|_2) over the blocks of the four instances is 1.68
(tinyGrid3D 0.20, smallGrid3D 0.37, ladder2 1.59, torus3D 1.68); the bound uses 10 times the measured value.

Not tested: the identity fallback of cert_build_precon for a pose without an edge.  The graph builder accepts such a pose, but
no node owns it, and every certificate entry refuses a group whose own poses are fewer than the graph's (see
tests/test_gpu_cert_proof.py on the ladder's unused ids): the branch cannot be reached through the API."""
import os
import sys

import numpy as np
import pytest

import dpgo_amd

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cert_search_checks as ck  # noqa: E402
import test_gpu_certify as tc  # noqa: E402  (its inputs and derived bounds; none of its tests is imported)
import test_gpu_cert_proof as tp  # noqa: E402  (the d = 2 instance)

pytestmark = pytest.mark.gpu

SMALL = [("tinyGrid3D", 1), ("smallGrid3D", 5), ("ladder2", 6)]
ALL = SMALL + [("torus3D", 8)]
KERNELS = ALL + [("tinyGrid3D", 9)]   # (one-row segments: for the two kernels only)
SEGMENTS = {("tinyGrid3D", 1): [1], ("tinyGrid3D", 9): [1] * 9, ("smallGrid3D", 5): [1] * 5, ("ladder2", 6): [2] * 6}
SENTINEL = -1.2345e77
_setup = {}


def setup(fixtures_dir, name, nn):
    """The instance, its group (kept for the module: a group's first certificate call allocates), the device's own Lambda at
    the chordal point and the operator's bound."""
    if (name, nn) not in _setup:
        N, mm, gp, X0, make = tp.instance(fixtures_dir, name)
        grp, opt = make(nn)
        s = dict(N=N, mm=mm, d=mm.d, gp=gp, X=X0, grp=grp, opt=opt, nn=nn, Lam=grp.cert_lambda(X0))
        _setup[name, nn] = s
    return _setup[name, nn]


def operator_bound(s):
    if "Aabs" not in s:
        s["Aabs"], s["k"] = tc.abs_operator(s["N"], s["mm"], s["nn"], s["opt"].regularizer)
    return s["Aabs"], s["k"]


def report(label, ratios, into=None):
    bad = ck.worst(ratios, {} if into is None else into)
    print(label, " ".join("%s %.3g" % kv for kv in sorted(ratios.items())))
    return bad


def gram(s, b):
    return s["grp"].debug_cert_gram(s["X"], b["V"], b["W"], b["P"], b["SV"], b["SP"], MW=b["MW"])


def test_the_instances_have_the_segments_they_are_chosen_for(fixtures_dir):
    for (name, nn), segs in SEGMENTS.items():
        s = setup(fixtures_dir, name, nn)
        _, own, _ = s["grp"].debug_seg_layout()
        assert list(np.diff(own)) == segs, (name, own)
    s = setup(fixtures_dir, "ladder2", 6)
    assert [s["grp"].sizes[a][0] for a in range(6)] == [68, 67, 67, 67, 67, 67]
    s = setup(fixtures_dir, "tinyGrid3D", 9)
    assert [s["grp"].sizes[a][0] for a in range(9)] == [1] * 9
    s = setup(fixtures_dir, "torus3D", 8)
    assert s["grp"].debug_seg_layout()[1][-1] > 64   # k_cert_reduce: lanes 0..63 take a second segment each


# ---------------------------------------------------------------------------------------------------------------
# k_cert_gram + k_cert_reduce
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["full", "P=0", "W=P=0", "P=W"])
@pytest.mark.parametrize("name,nn", KERNELS)
def test_gram_sums(fixtures_dir, name, nn, variant):
    """Every one of the 2 ntri sums, for independent Gaussian blocks: a misrouted sum, a transposed index, a dropped or doubled
    pose are 1e10 bounds away."""
    s = setup(fixtures_dir, name, nn)
    d = s["d"]
    b = ck.gaussian_blocks(np.random.default_rng(20 + len(variant)), s["X"].shape, variant)
    sums, SW = gram(s, b)
    r = ck.gram_ratios(d, s["Lam"], b, sums, SW)
    report("%s/%d %s" % (name, nn, variant), r)
    assert not [q for q, v in r.items() if not v <= 1.0], r
    if variant == "W=P=0":   # the first pass of the loop: S W is M W, and the sums with a zero block are zeros, not small
        assert np.array_equal(SW, b["MW"])
        G = np.zeros((3 * d, 3 * d))
        G[np.triu_indices(3 * d)] = sums[:ck.ntri(d)]
        assert np.all(G[:, d:] == 0.0)
    if variant == "P=W":     # a singular mass matrix: the Rayleigh-Ritz step drops P
        A, B = ck.ritz_matrices(sums, d, 3)
        assert dpgo_amd.rayleigh_ritz(A, B, 3)[2] == 2


@pytest.mark.parametrize("name,nn", SMALL)
def test_gram_finishes_S_W(fixtures_dir, name, nn):
    """S W = M W - [0 ; Lambda W_Y] entrywise within 2 d u |Lambda_p| |W_p| + u |result|, the translation rows copies.

    This test found sub_lambda (cert.hip; shared by k_cert_gram, k_cert_apply and k_cert_lambda) subtracting the d products from
    M W one fma at a time, which rounds each of the d partial results: d u |result| + 2 (d - 1) u |Lambda_p| |W_p|, up to d times
    the u |result| of the bound where Lambda_p W_p is small against M W -- measured 1.098 x the bound on ladder2 here, 1.05 ..
    1.38 with the blocks of test_gram_sums, 1.74 on torus3D's 60 000 entries.  The kernel now sums the products first and
    subtracts once: d u |Lambda_p| |W_p| + u |result| (measured since: at most 0.93 x the bound, on every instance)."""
    s = setup(fixtures_dir, name, nn)
    b = ck.gaussian_blocks(np.random.default_rng(20), s["X"].shape)
    sums, SW = gram(s, b)
    r = ck.gram_ratios(s["d"], s["Lam"], b, sums, SW)
    report("%s/%d S W" % (name, nn), r)
    assert np.array_equal(SW[:s["N"]], b["MW"][:s["N"]])
    assert r["SW"] <= 1.0, r


@pytest.mark.parametrize("name,nn", SMALL)
def test_gram_forms_M_W_as_the_loop_does(fixtures_dir, name, nn):
    """MW = None: the hook makes the loop's own product M W before the launch."""
    s = setup(fixtures_dir, name, nn)
    Aabs, k = operator_bound(s)
    b = ck.gaussian_blocks(np.random.default_rng(21), s["X"].shape)
    b["MW"] = None
    sums, SW = gram(s, b)
    r = ck.gram_ratios(s["d"], s["Lam"], b, sums, SW, M=s["gp"].M, bMW=tc.prod_bound(Aabs, k, b["W"]))
    assert not report("%s/%d M W formed" % (name, nn), r), r


# ---------------------------------------------------------------------------------------------------------------
# k_cert_update + k_cert_reduce
# ---------------------------------------------------------------------------------------------------------------
def update(s, Cf, theta, b, precondition):
    out = s["grp"].debug_cert_update(Cf, theta, b["V"], b["W"], b["P"], b["SV"], b["SW"], b["SP"], precondition, nbr_fill=SENTINEL)
    assert np.array_equal(out["SW"], b["SW"])                      # read only
    assert (out["nbr"].shape[1] > 0) == (s["nn"] > 1)
    assert np.all(out["nbr"] == SENTINEL)                           # the neighbour segments' rows are not the launch's
    return out


@pytest.mark.parametrize("precondition", [True, False])
@pytest.mark.parametrize("name,nn", KERNELS)
def test_update(fixtures_dir, name, nn, precondition):
    s = setup(fixtures_dir, name, nn)
    d, grp = s["d"], s["grp"]
    T = grp.debug_cert_precon() if precondition else None
    rng = np.random.default_rng(22)
    # a Gaussian C and theta
    b = ck.gaussian_blocks(rng, s["X"].shape)
    b["SW"] = b.pop("MW")
    Cf, theta = rng.standard_normal((3 * d, d)), rng.standard_normal(d)
    out = update(s, Cf, theta, b, precondition)
    assert not report("%s/%d gaussian C" % (name, nn), ck.update_ratios(d, Cf, theta, b, out, T))
    # the C of a restart: P = W, the device's own sums, the host's Rayleigh-Ritz step with its P rows zero
    b = ck.gaussian_blocks(rng, s["X"].shape, "P=W")
    sums, SW = gram(s, b)
    A, B = ck.ritz_matrices(sums, d, 3)
    theta, C3, used = dpgo_amd.rayleigh_ritz(A, B, 3)
    assert used == 2 and np.all(C3[2 * d:] == 0.0) and np.any(C3[d:2 * d] != 0.0)
    b["SW"] = SW
    del b["MW"]
    out = update(s, C3, theta, b, precondition)
    assert not report("%s/%d restart C" % (name, nn), ck.update_ratios(d, C3, theta, b, out, T))


# ---------------------------------------------------------------------------------------------------------------
# cert_build_precon
# ---------------------------------------------------------------------------------------------------------------
_cinv = {}


def inverse_constant(fixtures_dir):
    if not _cinv:
        for name, nn in ALL:
            N, mm, gp, _, _ = tp.instance(fixtures_dir, name)
            _cinv[name] = float(np.max(ck.inverse_ratios(gp.M, N, mm.d)))
        print("inversion ratios", _cinv)
    return max(_cinv.values())


@pytest.mark.parametrize("name,nn", ALL)
def test_preconditioner(fixtures_dir, name, nn):
    s = setup(fixtures_dir, name, nn)
    Aabs, k = operator_bound(s)
    c = 10 * inverse_constant(fixtures_dir)
    T = s["grp"].debug_cert_precon()
    assert np.array_equal(T, T.transpose(0, 2, 1))
    assert not np.any(np.all(T == np.eye(s["d"] + 1), axis=(1, 2)))   # (no pose took the identity fallback)
    r = ck.precon_ratio(s["gp"].M, Aabs, k, s["N"], s["d"], T, c)
    print(name, nn, "T_p: worst error / bound %.3g (c = %.3g)" % (r, c))
    assert r <= 1.0


# ---------------------------------------------------------------------------------------------------------------
# the production loop, pass by pass
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precondition", [True, False])
@pytest.mark.parametrize("name,nn", SMALL)
def test_production_search_is_the_hooks_pass_by_pass(fixtures_dir, name, nn, precondition):
    """12 traced passes of certify against the same passes made from the hooks: sums, used, theta and C bit for bit (the
    hooks make the same launches on the same bits; upload and download are copies), nblk = 1, 2, 3, 3, .., a refresh after
    every fifth; every replayed pass is also held to the longdouble step functions."""
    s = setup(fixtures_dir, name, nn)
    d, grp, X, N = s["d"], s["grp"], s["X"], s["N"]
    Aabs, k = operator_bound(s)
    NT = ck.ntri(d)
    V0 = np.random.default_rng(0).standard_normal(X.shape)
    grp.debug_cert_trace(True)
    try:
        res, x_on = grp.certify(X, V0=V0, max_iters=12, refresh_every=5, stop_on_negative=False, tau=1e-300, precondition=precondition)
        trace = grp.debug_cert_trace_get()
    finally:
        grp.debug_cert_trace(False)
    assert res.iterations == 12 and len(trace) == 12
    # the trace is a record and nothing else: the same call without it returns the same bits, and leaves no record
    kw = dict(V0=V0, max_iters=12, refresh_every=5, stop_on_negative=False, tau=1e-300, precondition=precondition)
    off, x_off = grp.certify(X, **kw)
    assert (off.theta, off.residual, off.iterations, off.status, off.restarts) == (res.theta, res.residual, res.iterations, res.status, res.restarts)
    assert np.array_equal(x_off, x_on) and grp.debug_cert_trace_get() == []
    T = grp.debug_cert_precon() if precondition else None
    Z = np.zeros(X.shape)
    cur = dict(V=V0, W=Z, P=Z, SV=grp.cert_apply(X, V0), SP=Z, MW=Z)   # (the loop's start: W = P = S W = S P = 0)
    worst, restarts = {}, 0
    for it in range(1, 13):
        t = trace[it - 1]
        nblk = min(it, 3)
        sums, SW = gram(s, cur)
        assert np.array_equal(sums[:2 * NT], t["sums"][:2 * NT]), it
        if it > 1:   # the sums of the previous pass's update ride with this pass's reduction
            assert np.array_equal(t["sums"][2 * NT:], np.concatenate([out["rr"], out["vv"]])), it
        A, B = ck.ritz_matrices(sums, d, nblk)
        theta, C, used = dpgo_amd.rayleigh_ritz(A, B, nblk)
        Cf = np.zeros((3 * d, d))
        Cf[:d * nblk] = C
        assert (t["nblk"], t["used"], t["refresh"]) == (nblk, used, it % 5 == 0), (it, t)
        assert np.array_equal(t["theta"], theta) and np.array_equal(t["C"], Cf), it
        restarts += used < nblk
        bMW = None if it == 1 else tc.prod_bound(Aabs, k, cur["W"])   # (pass 1: M W is given, zeros)
        bad = report("pass %d gram" % it, ck.gram_ratios(d, s["Lam"], cur, sums, SW, M=s["gp"].M, bMW=bMW), worst)
        b = dict(cur, SW=SW)
        out = update(s, Cf, theta, b, precondition)
        bad += report("pass %d update" % it, ck.update_ratios(d, Cf, theta, b, out, T), worst)
        assert not bad, (it, bad)
        cur = dict(V=out["V"], W=out["W"], P=out["P"], SV=out["SV"], SP=out["SP"], MW=None)
        if it % 5 == 0:
            cur["SV"], cur["SP"] = grp.cert_apply(X, cur["V"]), grp.cert_apply(X, cur["P"])
    assert restarts == res.restarts
    print(name, nn, precondition, "worst error / bound over 12 passes:", " ".join("%s %.3g" % kv for kv in sorted(worst.items())))
