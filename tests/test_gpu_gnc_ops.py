"""The edge pass of graduated non-convexity on the device (k_gnc_edge, k_gnc_final through NodeGroup.gnc_eval) against its
restatement (tests/gnc_restatement.py), WEIGH and FIXED, with the robust set by the inter rule, given, empty and every edge.

Held on every input: s_rot and s_trans bit-equal to EdgeEval at the same point; on the robust set w within the bound of
tests/gnc_restatement.py (TLS 16 u (mu+1), GM 36 u w) of the long-double weight of the device's own s; the three counts, the
maximum of s and the minimum of w exact; every sum within m u sum |terms| of the long-double sum of the device's own terms
(for the surrogate's sum 12 u sum of the magnitudes rho is made of are added: rho is itself a rounded function of s); the
same bits on a second call; the weight array untouched outside the robust set, and everywhere under FIXED.

Inputs: the four chains of tests/gnc_inputs.py; robust_inputs.named("rand3_40") (one-pose nodes); random_graph(d, 64) and
random_graph(d, 65), d = 2 and 3 (one full workgroup, and one lane more), on 20 poses -- on random_graph's default of 40 a pose
is left without an edge, and no group hosts such a graph; random_graph(3, 4161, N=150), whose 66 partials exceed the final wave's
64 lanes.

The counts can be exact because the restatement evaluates the thresholds in the kernel's operation order: the test first
asserts that no robust s lies within 8 u (relative) of a threshold.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gnc_inputs as gi  # noqa: E402
import gnc_restatement as gr  # noqa: E402
import robust_inputs as ri  # noqa: E402
import robust_restatement as rr  # noqa: E402
import edge_restatement as er  # noqa: E402

import dpgo_amd  # noqa: E402

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = gr.U
C2 = 4.0
MUS = (0.05, 1.0, 20.0)
SENTINEL = 0.625

_obj = {}


def big():
    g = er.random_graph(3, 4161, N=150)     # 66 workgroups: more partials than the final wave has lanes
    return rr.problem(3, 150, g["I"], g["J"], g["R"], g["t"], g["kappa"], g["tau"], 2), np.asfortranarray(g["X"])


INPUTS = {name: (lambda n=name: gi.case(n)[:2]) for name in gi.CASES}
INPUTS.update({"rand3_40": lambda: ri.named("rand3_40"), "rand2_64": lambda: ri.random(2, 64, 20), "rand3_64": lambda: ri.random(3, 64, 20),
               "rand2_65": lambda: ri.random(2, 65, 20), "rand3_65": lambda: ri.random(3, 65, 20), "rand3_4161": big})


def objects(name):
    if name not in _obj:
        P, X = INPUTS[name]()
        G = ri.graph(P)
        _obj[name] = (P, X, G, ri.group(G), dpgo_amd.EdgeEval(G).run(X))
    return _obj[name]


def robust_sets(P):
    m = len(P["I"])
    rng = np.random.default_rng(5 + m)
    return {"inter": (None, P["inter"]), "given": ((rng.uniform(size=m) < 0.4).astype(np.int32),) * 2,
            "empty": (np.zeros(m, np.int32),) * 2, "all": (np.full(m, 7, np.int32),) * 2}     # (any non-zero int is membership)


def check_pass(tag, kind, mu, s, w, sums, R, weigh):
    m = len(s)
    R = np.asarray(R, bool)
    sl = np.asarray(s, LD)
    if kind == gr.TLS and R.any():
        for t in gr.thresholds(mu, C2):
            assert np.min(np.abs(s[R] - t)) > 8 * U * t, (tag, "a robust s on a threshold")
    w_ref, rho_ref = gr.weight_rho(kind, mu, C2, sl, LD)
    if weigh:
        err, bound = np.abs(np.asarray(w, LD) - w_ref)[R], gr.w_bound(kind, mu, w_ref)[R]
        assert np.all(err <= bound), (tag, float(np.max(err / np.maximum(bound, 1e-300))))
        assert np.array_equal(w[R], gr.weight_rho(kind, mu, C2, s[R])[0])      # (and the float64 restatement to the bit)
    wl = np.asarray(w, LD)
    want = dict(sum_out=np.sum(sl[~R]), sum_ws=np.sum(wl[R] * sl[R]), sum_rho=np.sum(rho_ref[R]))
    mag = dict(sum_out=np.sum(np.abs(sl[~R])), sum_ws=np.sum(np.abs(wl[R] * sl[R])), sum_rho=np.sum(np.abs(rho_ref[R])))
    extra = 0.0
    if R.any():
        parts = 2 * np.sqrt(LD(C2) * LD(mu) * (LD(mu) + 1) * sl[R]) + LD(mu) * (LD(C2) + sl[R]) if kind == gr.TLS else rho_ref[R]
        extra = 12 * U * float(np.sum(np.maximum(parts, rho_ref[R])))
    for k, (name, tol_extra) in enumerate((("sum_out", 0.0), ("sum_ws", 0.0), ("sum_rho", extra))):
        tol = m * U * float(mag[name]) + tol_extra
        assert abs(LD(sums[k]) - want[name]) <= tol, (tag, name, float(abs(LD(sums[k]) - want[name])), tol)
    assert sums[3] == (s[R].max() if R.any() else 0.0)
    assert sums[4] == (w[R].min() if R.any() else np.inf)
    assert tuple(int(v) for v in sums[5:]) == (int(np.sum(w[R] == 0)), int(np.sum(w[R] == 1)), int(np.sum((w[R] > 0) & (w[R] < 1)))), tag
    return tuple(int(v) for v in sums[5:])


@pytest.mark.parametrize("name", list(INPUTS))
def test_edge_pass_against_the_restatement(name):
    P, X, G, grp, ev = objects(name)
    m = len(P["I"])
    seen = np.zeros(3, np.int64)
    for rname, (arg, R) in robust_sets(P).items():
        R = np.asarray(R, bool)
        for kind in (gr.TLS, gr.GM):
            for mu in MUS:
                tag = (name, rname, kind, mu)
                start = np.full(m, SENTINEL)
                sr, st, w, sums = grp.gnc_eval(G, X, kind, mu, C2, robust_set=arg, w_start=start)
                assert np.array_equal(sr, ev[0]) and np.array_equal(st, ev[1]), tag
                assert np.all(w[~R] == SENTINEL), tag                        # untouched outside the robust set
                s = sr + st
                counts = check_pass(tag, kind, mu, s, w, sums, R, True)
                if kind == gr.TLS and rname != "empty":
                    seen += counts
                again = grp.gnc_eval(G, X, kind, mu, C2, robust_set=arg, w_start=start)
                assert all(np.array_equal(a, b) for a, b in zip((sr, st, w, sums), again)), tag
                # FIXED: an array of the caller's, with exact zeros and ones in it
                rng = np.random.default_rng(11)
                w_in = rng.uniform(0, 1, m)
                w_in[rng.uniform(size=m) < 0.2] = 0.0
                w_in[rng.uniform(size=m) < 0.2] = 1.0
                fr, ft, wf, fsums = grp.gnc_eval(G, X, kind, mu, C2, robust_set=arg, w_in=w_in)
                assert np.array_equal(fr, sr) and np.array_equal(ft, st) and np.array_equal(wf, w_in), tag
                check_pass(tag + ("fixed",), kind, mu, s, w_in, fsums, R, False)
                assert fsums[0] == sums[0] and fsums[2] == sums[2] and fsums[3] == sums[3]     # (what does not depend on w)
    print("%s: %d edges; TLS weights seen over the sets and mus: %d zero, %d one, %d between" % (name, m, *seen))
    assert np.all(seen > 0), "the input does not reach every branch of the TLS weight"


def test_refusals():
    P, X, G, grp, _ = objects("c2_40")
    for bad in (dict(kind=2), dict(kind=-1), dict(mu=0.0), dict(mu=float("nan")), dict(barc2=0.0), dict(barc2=float("inf"))):
        kw = dict(kind=0, mu=1.0, barc2=C2)
        kw.update(bad)
        with pytest.raises(RuntimeError):
            grp.gnc_eval(G, X, **kw)
    with pytest.raises(RuntimeError):
        grp.gnc_eval(objects("c3_24")[2], X, 0, 1.0, C2)                      # another pose count
    with pytest.raises(ValueError):
        grp.gnc_eval(G, X, 0, 1.0, C2, robust_set=np.zeros(3, np.int32))
    # a robust_polish behind a pass with a given set sees the inter rule again (the plan is keyed on its records)
    first = grp.robust_polish(X, 2, 1.0, graph=G)
    grp.gnc_eval(G, X, 0, 1.0, C2, robust_set=np.ones(len(P["I"]), np.int32))
    second = grp.robust_polish(X, 2, 1.0, graph=G)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[2], second[2])
