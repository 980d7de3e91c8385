"""The gate of the speculative update -- k_reduce_gate, amm_gate_node -- on GIVEN partial sums, through the launch
Group::speculate_update makes (NodeGroup.debug_cg_scalars, kinds "reduce_gate" and "reduce"), against tests/gate_restatement.py,
which tests/test_gate_restatement_host.py pins to the oracle's runs.

A case is one script: begin_host (every node live), scal_begin (the refinement's start and its first CG step: the gate reads
what THIS launch left in device memory and in the CG records), reduce (launch_reduce over own rows), reduce_gate (the same
sums).  One node of the group plays the case, the others take the common course; the gate's word is the AND over the nodes, so
  go, h_gate    exact: all ones / 1.0 iff the restatement says every node is common, and the restatement's conjuncts of the
                case's node are the ones the case declares false
  sums          the pinned scalars, their device copy and launch_reduce's pinned scalars: bit for bit the same, and the
                exact values the table was built from; slots >= nslots untouched
  flag          arrived back at 0, the flag at the last sequence number, one number per flag-raising launch
The sums are small integers times powers of two split unevenly over a node's own segments (exact in every order); a value
with no spare low bits (a threshold's neighbour, a contraction operand) sits in ONE segment, the others hold 0.0.  Neighbour
segments hold +-3e200, unused slots NaN.

Thresholds are probed at equality and one ulp either side with inputs whose intermediate expressions are exact (checked with
fractions.Fraction below): the probed operand is the stored value itself.  The contraction cases come from a random search
(SEED) for inputs on which ONE fused multiply-add changes the verdict; 0.5 (..) + f and -t1 - 0.5 t2 have an exact product
unless it is subnormal, so those inputs are multiples of 2^-1074.

Groups: synthetic.ladder(3) (6 nodes, 1 to 3 own segments), the one-node synthetic.grid(17, 17, 16) (73 own segments) and a
64-node grid (MAX_LOCAL_NODES) with the case at node 63.

The last test drives real lattices through step() in child processes under options that force the iteration off the common
course; its docstring has the counters.
"""
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import gate_restatement as GR
import test_gpu_cg_scalars as S
from test_gpu_cg_scalars import ladder_group, wide_group   # noqa: F401  (fixtures)

NAN, INF = float("nan"), float("inf")
U = 2.0 ** -1074                  # the smallest subnormal
NSLOTS = GR.DS + 3                # what run_tnt() reduces for a trial point that carries the half step's parked sums
MAX_SLOTS = 32
ALL_ONES = 0xFFFFFFFFFFFFFFFF
SEED = 20241019                   # of the contraction search
STEP = {"boundary": ([1.0, 16.0, 4.0, -4.0], 2.0),     # the CG ends at the trust-region boundary with its first step
        "plain": ([8.0, 16.0, 4.0, -4.0], 64.0)}       # ... goes on to a second step: the record stays live


def nxt(x):
    return float(np.nextafter(x, INF))


def prv(x):
    return float(np.nextafter(x, -INF))


# ---------------------------------------------------------------------------------------------------------------------
# nodes and options.  BASE takes the common course: fx = 1, fx_prop = 1/2, df = dm = 1/2, rho = 1, |h| = 2^-20 < step_tol,
# Gk = 1/4, Gkh = 1/2, minG = 7/8, Fk0 - Gk = 3/4 >= phi (Fk0 - Gkh) = 1/4
BASE = dict(g2=9.0, b1=5.0, b2=-3.0, b3=7.0, step="boundary", f=0.0, Fk0=1.0, Fk1=1.0, fobj=1.0, hits0=0, hits1=0,
            t={0: 2.0 ** -40, 1: -1.0, 2: 1.0, 3: -2.0, 4: -2.25, 5: 3.0, GR.DS: 0.25, GR.DS + 1: 0.5})
BASE_OPT = dict(max_it=1, max_acc=1, max_hits0=10, max_hits1=25, rel_tol=2.0 ** -20, step_tol=2.0 ** -10, psi=0.5, phi=0.5)
# PROBE: fx_prop = 0 and t3 = 0, so Gk = t4 and df = fx = b1 / 2 are stored values themselves
PROBE = dict(b1=2.0, b2=0.0, t={3: 0.0, 5: 0.0, 4: 0.25})
NO_REDO_NO_FALL = {GR.DS: -4.0, GR.DS + 1: 2.0}   # minG = Fk0 + 2 > Gkh = 2 and phi (Fk0 - 2) <= 0 for Fk0 in [1, 2]


def node(*overrides):
    nd = dict(BASE, t=dict(BASE["t"]))
    for o in overrides:
        for k, v in o.items():
            if k == "t":
                nd["t"].update(v)
            else:
                nd[k] = v
    return nd


def case(name, false=(), opt=None, probe=None, contract=None, **nd):
    return dict(name=name, node=node(*nd.pop("of", ()), nd), opt=dict(BASE_OPT, **(opt or {})), false=set(false), probe=probe,
                contract=contract)


def b_of(nd):
    active = 0.0 if math.sqrt(nd["g2"]) < S.TOL["grad_tol"] else 1.0
    return [nd["g2"], nd["b1"], nd["b2"], nd["b3"], 0.0, 0.0, active, 0.0]


def t_of(nd):
    return [nd["t"].get(q, NAN) for q in range(16)]


def restate(nd, opt, b=None, live=None, contract=None):
    b = b_of(nd) if b is None else b
    live = (nd["step"] == "plain" and b[6] != 0.0) if live is None else live
    return GR.gate_node(t_of(nd), b, live, nd["f"], nd["Fk0"], nd["Fk1"], nd["fobj"], nd["hits0"], nd["hits1"], opt, contract)


# ---- one case per conjunct, the ways a refinement ends, the special values
def conjunct_cases():
    two = dict(max_it=2, max_acc=2)
    out = [
        case("all nine true"),
        case("inactive: b[6] == 0", {"active"}, g2=2.0 ** -30),
        case("the CG is still live", {"cg_over"}, step="plain"),
        case("rho <= eta1", {"accepted"}, t={1: -64.0}),
        case("rho NaN: df = dm = 0", {"accepted"}, b1=0.0, b2=0.0, t={1: 0.0, 2: 0.0, 3: 0.0, 5: 0.0}),
        case("a second trust-region iteration follows", {"ends"}, opt=two, t={0: 0.25}),
        case("ends by rel_dec", opt=dict(two, rel_tol=0.75), t={0: 0.25}),
        case("ends by h_norm", opt=two),
        case("ends by max_it alone", opt=dict(max_it=1, max_acc=2), t={0: 0.25}),
        case("ends by max_acc alone", opt=dict(max_it=2, max_acc=1), t={0: 0.25}),
        case("redo of the half step", {"no_redo"}, t={GR.DS + 1: 0.90625}),
        case("hard restart", {"no_hard_restart"}, t={**NO_REDO_NO_FALL, 4: -1.25}),
        case("soft restart, first arm", {"no_soft_restart0"}, Fk0=2.0, fobj=2.0, hits0=10, t={4: -1.25, GR.DS + 1: 1.0}),
        case("soft restart, second arm", {"no_soft_restart1"}, Fk0=2.0, Fk1=2.0, hits1=26, t={4: -1.25, GR.DS + 1: 1.0}),
        case("first arm's counter reached, Gk below Fk1", Fk0=2.0, fobj=2.0, hits0=10, hits1=26),
        case("fall back", {"no_fall_back"}, t={4: -1.75, GR.DS + 1: 0.0}),
        # dm < 0 with df < 0: rho = 1 > eta1, accepted as the host accepts it (fx_prop = 2, Gk = 1/4)
        case("dm < 0 and df < 0", t={1: 1.0, 2: 0.0, 3: 0.0, 5: 4.0, 4: -1.75}),
        # df = +inf (fx = +inf): rho = +inf, rel_dec = NaN (no stop by it), ends by h_norm
        case("df infinite", b1=INF),
        case("dm infinite", {"accepted"}, t={1: -INF}),
        case("df and dm infinite", {"accepted"}, b1=INF, t={1: -INF}),
    ]
    return out


# ---- every threshold at equality and one ulp either side.  probe: (the comparison, the conjunct it decides, its sense:
# the conjunct is FALSE when the comparison holds (True) / TRUE when it holds (False))
def threshold_cases():
    out = []
    two = dict(max_it=2, max_acc=2)
    for x in (prv(0.05), 0.05, nxt(0.05)):          # rho = df / dm = (b1 / 2) / 1
        out.append(case("rho = %r against eta1" % x, () if x > 0.05 else {"accepted"}, probe=("rho > eta1", x > 0.05),
                        of=(PROBE,), b1=2.0 * x, t={1: -1.0, 2: 0.0}))
    df = 0.5 - 2.0 ** -26                            # fx = 1 - 2^-26: sqrt_eps + |fx| = 1, rel_dec = df = fx - 1/2
    for tol in (prv(df), df, nxt(df)):
        out.append(case("rel_tol = %r against rel_dec" % tol, () if df < tol else {"ends"}, opt=dict(two, rel_tol=tol),
                        probe=("rel_dec < rel_tol", df < tol), b1=2.0 * (1.0 - 2.0 ** -26), b2=0.0, t={0: 0.25, 3: 0.0, 5: 1.0, 4: -0.25}))
    for tol in (prv(0.5), 0.5, nxt(0.5)):            # h_norm = sqrt(1/4)
        out.append(case("step_tol = %r against h_norm" % tol, () if 0.5 < tol else {"ends"}, opt=dict(two, step_tol=tol),
                        probe=("h_norm < step_tol", 0.5 < tol), t={0: 0.25}))
    for x in (prv(0.875), 0.875, nxt(0.875)):        # Gkh = t13 against minG = 1 - 1/2 * 1/4
        out.append(case("Gkh = %r against minG" % x, {"no_redo"} if x > 0.875 else (), probe=("Gkh > minG", x > 0.875),
                        t={GR.DS + 1: x}))
    for x in (prv(1.0), 1.0, nxt(1.0)):              # Gk = t4
        hit = x > 1.0
        out.append(case("Gk = %r against Fk0" % x, {"no_hard_restart"} if hit else (), probe=("Gk > Fk0", hit),
                        of=(PROBE,), Fk0=1.0, Fk1=2.0, fobj=2.0, t={**NO_REDO_NO_FALL, 4: x}))
        out.append(case("Gk = %r against Fk1" % x, {"no_soft_restart0"} if hit else (), probe=("Gk > Fk1", hit),
                        of=(PROBE,), Fk0=2.0, Fk1=1.0, fobj=2.0, hits0=10, t={**NO_REDO_NO_FALL, 4: x}))
        out.append(case("Gk = %r against fobj" % x, {"no_soft_restart1"} if hit else (), probe=("Gk > fobj", hit),
                        of=(PROBE,), Fk0=2.0, Fk1=2.0, fobj=1.0, hits1=26, t={**NO_REDO_NO_FALL, 4: x}))
    for h in (9, 10, 11):                            # >=
        out.append(case("hits0 = %d against max_hits0" % h, {"no_soft_restart0"} if h >= 10 else (),
                        probe=("hits0 >= max_hits0", h >= 10), of=(PROBE,), Fk0=2.0, Fk1=1.0, fobj=2.0, hits0=h,
                        t={**NO_REDO_NO_FALL, 4: 1.5}))
    for h in (24, 25, 26):                           # >
        out.append(case("hits1 = %d against max_hits1" % h, {"no_soft_restart1"} if h > 25 else (),
                        probe=("hits1 > max_hits1", h > 25), of=(PROBE,), Fk0=2.0, Fk1=2.0, fobj=1.0, hits1=h,
                        t={**NO_REDO_NO_FALL, 4: 1.5}))
    for x in (prv(0.75), 0.75, nxt(0.75)):           # Fk0 - Gk = 1 - t4 (exact) against phi (Fk0 - Gkh) = 1/4
        hit = 1.0 - x < 0.25
        out.append(case("Fk0 - Gk = 1 - %r against phi (Fk0 - Gkh)" % x, {"no_fall_back"} if hit else (),
                        probe=("Fk0 - Gk < phi (Fk0 - Gkh)", hit), of=(PROBE,), t={4: x}))
    return out


def exact_values(nd, opt):
    """the gate's expressions in exact rational arithmetic (finite inputs; rho and rel_dec None where the divisor is 0)"""
    F = Fraction
    b, t, f = [F(x) for x in b_of(nd)], {q: F(v) for q, v in nd["t"].items()}, F(nd["f"])
    fx, fx_prop = (b[1] + b[2]) / 2 + f, (t[5] + t[3]) / 2 + f
    dm, df = -t[1] - t[2] / 2, fx - fx_prop
    Gk, Gkh = fx_prop - t[3] + t[4], t[GR.DS + 1] + f
    return dict(fx=fx, fx_prop=fx_prop, dm=dm, df=df, rho=df / dm if dm else None, rel_dec=df / (F(GR.SQRT_EPS) + abs(fx)),
                h_norm2=t[0], Gk=Gk, Gkh=Gkh, minG=F(nd["Fk0"]) - F(opt["psi"]) * t[GR.DS], fall_lhs=F(nd["Fk0"]) - Gk,
                fall_rhs=F(opt["phi"]) * (F(nd["Fk0"]) - Gkh))


# ---- contraction: a search for inputs on which one fused multiply-add flips the verdict
def _draw(rng, expr):
    k = lambda lo, hi: int(rng.integers(lo, hi + 1))   # noqa: E731
    if expr == "fx":        # fx = 0.5 b1 + f in subnormals, fx_prop = f, dm = m u
        return dict(b1=(2 * k(0, 7) + 1) * U, b2=0.0, f=k(-7, 7) * U, t={3: 0.0, 5: 0.0, 4: 0.25, 1: -k(1, 64) * U, 2: 0.0}), {}
    if expr == "fx_prop":   # fx = f, fx_prop = 0.5 t5 + f
        return dict(b1=0.0, b2=0.0, f=k(-7, 7) * U, t={3: 0.0, 5: (2 * k(0, 7) + 1) * U, 4: 0.25, 1: k(-64, 64) * U, 2: 0.0}), {}
    if expr == "dm":        # df = fx = d u, dm = m u - 0.5 (2 j + 1) u
        return dict(b1=2 * k(1, 4) * U, b2=0.0, t={3: 0.0, 5: 0.0, 4: 0.25, 1: -k(1, 64) * U, 2: (2 * k(0, 7) + 1) * U}), {}
    if expr == "minG":      # Gkh = the larger of the two minG
        psi, Fk0, t12 = float(rng.uniform(0.1, 0.9)), float(rng.uniform(1, 2)), float(rng.uniform(0.1, 1))
        return dict(PROBE, Fk0=Fk0, Fk1=2.0, fobj=2.0, t={3: 0.0, 5: 0.0, 4: 0.25, GR.DS: t12,
                                                          GR.DS + 1: max(Fk0 - psi * t12, GR.fma(-psi, t12, Fk0))}), dict(psi=psi)
    if expr == "fall":      # Fk0 - Gk = Fk0 = fl(phi x), x = Fk0 - Gkh: the rounded product is not below itself, the exact one may be
        phi, x = float(rng.uniform(0.1, 0.9)), float(rng.uniform(0.5, 1.5))
        Fk0 = phi * x
        return dict(PROBE, Fk0=Fk0, Fk1=2.0, fobj=2.0, t={3: 0.0, 5: 0.0, 4: 0.0, GR.DS: -4.0, GR.DS + 1: Fk0 - x}), dict(phi=phi)
    raise KeyError(expr)


CONTRACTED = {"fx": ("fx", "accepted"), "fx_prop": ("fx_prop", "accepted"), "dm": ("dm", "accepted"), "minG": ("minG", "no_redo"),
              "fall": (None, "no_fall_back")}


# "fall": the rounded product is not below itself, only the exact one can be.  "dm": eta1 = 0.05 lies between d / (20 d - 1) and
# d / (20 d); with 20 d even, ties-to-even never rounds the fused value DOWN to 20 d - 1 where the rounded product gives 20 d
ONE_WAY = ("dm", "fall")


def contraction_cases(per_expr=2):
    """per expression `per_expr` inputs for which (1) the contracted value of the expression differs from the rounded product
    plus add and (2) the node's verdict differs with it, every other conjunct being true -- both proved here on the host"""
    rng = np.random.default_rng(SEED)
    out, draws = [], {}
    for expr, (value, conj) in CONTRACTED.items():
        found, seen = [], set()
        for n in range(1, 2001):
            nd, o = _draw(rng, expr)
            c = case("contraction of %s, draw %d" % (expr, n), opt=o, contract=expr, **nd)
            vu, vf = restate(c["node"], c["opt"]), restate(c["node"], c["opt"], contract=expr)
            differs = vu.conjuncts[conj] != vf.conjuncts[conj] and (value is None or vu.values[value] != vf.values[value])
            others = all(vu.conjuncts[k] and vf.conjuncts[k] for k in GR.CONJUNCTS if k != conj)
            if differs and others and vu.common not in seen:
                if expr not in ONE_WAY:
                    seen.add(vu.common)     # one input per direction where both directions exist
                c["false"] = set() if vu.common else {conj}
                found.append(c)
                if len(found) == per_expr:
                    break
        draws[expr] = n
        out += found
    return out, draws


# ---------------------------------------------------------------------------------------------------------------------
# host part: the cases take the branches they are meant to take

def _check_case(c):
    v = restate(c["node"], c["opt"])
    false = {k for k in GR.CONJUNCTS if not v.conjuncts[k]}
    assert false == c["false"], (c["name"], false, c["false"], v.values)
    assert v.common == (not c["false"])
    return v


def test_cases_on_the_restatement():
    cs = conjunct_cases()
    for c in cs:
        _check_case(c)
    # each conjunct is the only false one in some case, and the base case has none
    singles = {next(iter(c["false"])) for c in cs if len(c["false"]) == 1}
    assert singles == set(GR.CONJUNCTS) and not cs[0]["false"]
    assert all(len(c["false"]) <= 1 for c in cs)
    # the other nodes of a launch take the common course under every option set a case brings
    for c in cs + threshold_cases() + contraction_cases()[0]:
        assert restate(node(), c["opt"]).common, c["name"]


def test_thresholds_are_exact():
    """the probed comparison's operands are exactly what the rational evaluation gives (no rounding anywhere on the way), its
    outcome is the rational one, and the three probes of a threshold give False, False, True or the like: both outcomes"""
    cs = threshold_cases()
    outcomes = {}
    for c in cs:
        v = _check_case(c)
        what, want = c["probe"]
        lhs, rhs, got = next((l, r, res) for w, l, _, r, res in v.comparisons if w == what)
        assert got == want, (c["name"], lhs, rhs)
        ex = exact_values(c["node"], c["opt"])
        o = c["opt"]
        exact = {"rho > eta1": (ex["rho"], Fraction(GR.ETA1)), "rel_dec < rel_tol": (ex["rel_dec"], Fraction(o["rel_tol"])),
                 "h_norm < step_tol": (None, Fraction(o["step_tol"])), "Gkh > minG": (ex["Gkh"], ex["minG"]),
                 "Gk > Fk0": (ex["Gk"], Fraction(c["node"]["Fk0"])), "Gk > Fk1": (ex["Gk"], Fraction(c["node"]["Fk1"])),
                 "Gk > fobj": (ex["Gk"], Fraction(c["node"]["fobj"])), "hits0 >= max_hits0": (Fraction(c["node"]["hits0"]), Fraction(o["max_hits0"])),
                 "hits1 > max_hits1": (Fraction(c["node"]["hits1"]), Fraction(o["max_hits1"])),
                 "Fk0 - Gk < phi (Fk0 - Gkh)": (ex["fall_lhs"], ex["fall_rhs"])}[what]
        if exact[0] is None:
            assert Fraction(lhs) ** 2 == ex["h_norm2"]        # the square root is exact
        else:
            assert Fraction(lhs) == exact[0], (c["name"], lhs, exact[0])
        assert Fraction(rhs) == exact[1], (c["name"], rhs, exact[1])
        outcomes.setdefault(what, []).append(got)
    assert len(outcomes) == 10
    for what, got in outcomes.items():
        assert len(got) == 3 and sorted(got) in ([False, False, True], [False, True, True]), (what, got)
        # the outcome at equality tells a strict comparison from its non-strict twin
        assert got[1] == (what == "hits0 >= max_hits0"), (what, got)


def test_contraction_cases_tell_the_two_evaluations_apart():
    cs, draws = contraction_cases()
    assert len(cs) == 2 * len(CONTRACTED), [c["name"] for c in cs]
    assert max(draws.values()) <= 400, draws       # (a handful of draws each; seed SEED)
    for c in cs:
        _check_case(c)
        expr = c["contract"]
        value, conj = CONTRACTED[expr]
        vu, vf = restate(c["node"], c["opt"]), restate(c["node"], c["opt"], contract=expr)
        assert vu.common != vf.common and vu.conjuncts[conj] != vf.conjuncts[conj]
        if value:
            assert vu.values[value] != vf.values[value]
            # the emulation: the exact value of the expression, rounded once
            ex = exact_values(c["node"], c["opt"])
            assert vf.values[value] == float(ex[value]) and Fraction(vu.values[value]) != ex[value]
        else:
            ex = exact_values(c["node"], c["opt"])
            assert Fraction(vu.values["fall_lhs"]) == ex["fall_lhs"] and Fraction(vu.values["fall_rhs"]) != ex["fall_rhs"]
    print("draws until the last case of each expression:", draws)
    # both directions for the expressions that have both
    for expr in ("fx", "fx_prop", "minG"):
        assert {bool(c["false"]) for c in cs if c["contract"] == expr} == {True, False}, expr


def test_single_segment_placement_is_exact():
    for v in (nxt(0.05), prv(0.875), 3 * U, -7 * U, INF, 0.25, -2.25, 0.90625):
        for nseg in (1, 2, 3, 73):
            p = place(v, nseg, 5)
            assert len(p) == nseg
            lanes = [sum(p[k::64]) for k in range(min(64, nseg))]
            assert sum(lanes) == v and sum(reversed(p)) == v


# ---------------------------------------------------------------------------------------------------------------------
# the partial-sum tables

def _spare_bits(v):
    m = int(abs(math.frexp(v)[0]) * 2 ** 53)
    return 53 if m == 0 else (m & -m).bit_length() - 1


def place(v, nseg, k):
    """v over nseg segments so that every summation order gives v exactly: S._split where v has low bits to spare, else v in one
    segment (the k-th, cyclically) and zeros"""
    if math.isnan(v):
        return [NAN] * nseg
    if nseg > 1 and math.isfinite(v) and abs(v) > 2.0 ** -900 and _spare_bits(v) >= 16:
        return S._split(v, nseg)
    p = [0.0] * nseg
    p[k % nseg] = v
    return p


def table(layout, sums, nslots):
    """sums: {slot: {node: value}}; own segments of a node without a value and slots without an entry hold NaN, neighbour
    segments +-3e200"""
    nseg_all, own, _ = layout
    T = np.full((nslots, nseg_all), NAN)
    for s in range(nslots):
        T[s, own[-1]:] = [(-1.0) ** k * 3.0e200 for k in range(nseg_all - own[-1])]
        for a, v in sums.get(s, {}).items():
            T[s, own[a]:own[a + 1]] = place(v, own[a + 1] - own[a], a + s)
    return T


def launches_of(layout, nodes, opt, nslots=NSLOTS, twice=False):
    """begin_host, scal_begin, reduce, reduce_gate [, reduce_gate] of one case"""
    L = len(nodes)
    start = {}
    for a, nd in enumerate(nodes):
        for q, v in enumerate([nd["g2"], nd["b1"], nd["b2"], nd["b3"]] + [None] * (S.FIRST - 4) + STEP[nd["step"]][0]):
            if v is not None:
                start.setdefault(q, {})[a] = v
    tsum = {s: {a: nd["t"][s] for a, nd in enumerate(nodes) if s in nd["t"]} for s in range(nslots)}
    T = table(layout, tsum, nslots)
    gate = dict(opt, nslots=nslots, **{k: [nd[k] for nd in nodes] for k in ("f", "Fk0", "Fk1", "fobj", "hits0", "hits1")})
    out = [dict(kind="begin_host", bits=(1 << L) - 1, max_it=10, rv=[4.0] * L, Delta=[64.0] * L, target=[2.0 ** -10] * L),
           dict(kind="scal_begin", bits=(1 << L) - 1, use_precon=0, max_it=10, Delta=[STEP[nd["step"]][1] for nd in nodes],
                partials=table(layout, start, S.FIRST + 4), **S.TOL),
           dict(kind="reduce", partials=T, gate=dict(nslots=nslots)),
           dict(kind="reduce_gate", partials=T, gate=gate)]
    return out + ([out[-1]] if twice else [])


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def check_on_device(group, cases, at=None):
    """every case as one script; the case's node at index `at` (default: moving through the group), base nodes around it"""
    grp, layout = group
    L = len(layout[1]) - 1
    script, where = [], []
    for i, c in enumerate(cases):
        k = (i % L) if at is None else at
        nodes = [c["node"] if a == k else node() for a in range(L)]
        where.append((k, nodes))
        script += launches_of(layout, nodes, c["opt"])
    dev = grp.debug_cg_scalars(script)
    for i, c in enumerate(cases):
        k, nodes = where[i]
        _, start, red, gate = dev[4 * i:4 * i + 4]
        verdicts = []
        for a, nd in enumerate(nodes):
            # the hand-over: what scal_begin left in device memory is the start the table held, and the CG's record
            b = list(start["dev_tnt"][a]) + [0.0]
            assert np.array_equal(_bits(b[:7]), _bits(b_of(nd)[:7])), (c["name"], a, b)
            live = start["records"][a]["live"]
            assert live == int(nd["step"] == "plain" and b[6] != 0.0), (c["name"], a)
            assert gate["records"][a]["live"] == live
            verdicts.append(restate(nd, c["opt"], b, bool(live)))
        v = verdicts[k]
        assert {q for q in GR.CONJUNCTS if not v.conjuncts[q]} == c["false"], (c["name"], v.conjuncts)
        assert all(w.common for a, w in enumerate(verdicts) if a != k), c["name"]
        # ---- the decision: exact
        want = GR.gate_group(verdicts)
        assert want == (0 if c["false"] else ALL_ONES)
        assert gate["go"] == want, (c["name"], hex(gate["go"]), v.conjuncts, v.values)
        assert gate["h_gate"] == (1.0 if want else 0.0), (c["name"], gate["h_gate"])
        # ---- the sums: the table's exact values; pinned = device copy = launch_reduce's, bit for bit; the rest untouched
        for a, nd in enumerate(nodes):
            assert np.array_equal(_bits(gate["host_scalars"][a, :NSLOTS]), _bits(t_of(nd)[:NSLOTS])), (c["name"], a)
        assert np.array_equal(_bits(gate["host_scalars"][:, :NSLOTS]), _bits(gate["dev_sums"][:, :NSLOTS])), c["name"]
        assert np.array_equal(_bits(gate["host_scalars"]), _bits(red["host_scalars"])), c["name"]
        assert np.array_equal(_bits(gate["dev_sums"][:, NSLOTS:]), _bits(red["dev_sums"][:, NSLOTS:])), c["name"]
        # ---- the flag
        for o, before in ((red, start), (gate, red)):
            assert o["arrived"] == 0 and o["flag"] == o["seq"] == before["seq"] + 1, (c["name"], o["flag"], o["seq"])
    return dev


# ---------------------------------------------------------------------------------------------------------------------
# GPU part

@pytest.fixture(scope="module")
def full_group():
    """MAX_LOCAL_NODES = 64 nodes of two poses each"""
    import dpgo_amd
    from dpgo_amd import synthetic
    g = synthetic.grid(8, 4, 4)
    grp = dpgo_amd.NodeGroup(S._measurements_graph(g, 64), range(64), dpgo_amd.Options.driver(0, True))
    layout = grp.debug_seg_layout()
    assert len(layout[1]) == 65
    return grp, layout


@pytest.mark.gpu
def test_one_case_per_conjunct(ladder_group):
    check_on_device(ladder_group, conjunct_cases())


@pytest.mark.gpu
def test_thresholds_at_equality_and_one_ulp_either_side(ladder_group):
    check_on_device(ladder_group, threshold_cases())


@pytest.mark.gpu
def test_products_are_rounded_before_they_are_added(ladder_group):
    """the device takes the uncontracted side of every contraction case (check_on_device compares with the restatement, which
    rounds every product; test_contraction_cases_tell_the_two_evaluations_apart shows the fused evaluation decides otherwise)"""
    cs, _ = contraction_cases()
    check_on_device(ladder_group, cs)


@pytest.mark.gpu
def test_one_node_group(wide_group):
    """nnodes = 1, 73 own segments: the reduction's second trip; lanes 1..63 never veto"""
    cs = conjunct_cases()
    check_on_device(wide_group, cs[:6] + cs[10:16] + threshold_cases()[:3] + contraction_cases(1)[0])


@pytest.mark.gpu
def test_full_size_group(full_group):
    """64 nodes: every lane of the gate's wave has a node; the node off the common course is the last one"""
    cs = conjunct_cases()
    check_on_device(full_group, [cs[0]], at=0)
    check_on_device(full_group, [c for c in cs if len(c["false"]) == 1][:4] + [cs[0]], at=63)


@pytest.mark.gpu
def test_any_node_vetoes_and_every_lane_beyond_the_group_is_silent(ladder_group):
    c = conjunct_cases()[3]
    for k in range(6):
        check_on_device(ladder_group, [c], at=k)
    check_on_device(ladder_group, [conjunct_cases()[0]] * 2)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["ladder", "wide"])
def test_reduction_of_random_sums(ladder_group, wide_group, which):
    """random normal partials: the pinned scalars, the device copy and launch_reduce's agree bit for bit and lie within
    (ceil(nseg_own / 64) + 6) u sum |p_k| of math.fsum -- one add per trip of the lane loop, six levels of wave_sum"""
    grp, layout = ladder_group if which == "ladder" else wide_group
    nseg_all, own, _ = layout
    L = len(own) - 1
    rng = np.random.default_rng(11)
    T = rng.standard_normal((MAX_SLOTS, nseg_all)) * np.exp2(rng.integers(-20, 20, (MAX_SLOTS, 1)))
    nodes = [node() for _ in range(L)]
    sc = launches_of(layout, nodes, BASE_OPT)
    for nslots in (MAX_SLOTS, 7):
        gate = dict(sc[3]["gate"], nslots=nslots)
        dev = grp.debug_cg_scalars(sc[:2] + [dict(kind="reduce", partials=T, gate=dict(nslots=MAX_SLOTS)),
                                             dict(kind="reduce", partials=T, gate=dict(nslots=nslots)),
                                             dict(kind="reduce_gate", partials=T, gate=gate)])
        full, red, gt = dev[2:]
        assert np.array_equal(_bits(gt["host_scalars"]), _bits(red["host_scalars"]))
        assert np.array_equal(_bits(gt["host_scalars"][:, :nslots]), _bits(gt["dev_sums"][:, :nslots]))
        assert np.array_equal(_bits(gt["dev_sums"][:, nslots:]), _bits(red["dev_sums"][:, nslots:]))
        assert np.array_equal(_bits(gt["host_scalars"][:, nslots:]), _bits(full["host_scalars"][:, nslots:]))   # not written
        for a in range(L):
            n = own[a + 1] - own[a]
            for s in range(nslots):
                p = T[s, own[a]:own[a + 1]]
                bound = (math.ceil(n / 64) + 6) * 2.0 ** -53 * float(np.sum(np.abs(p)))
                assert abs(gt["host_scalars"][a, s] - math.fsum(p)) <= bound, (a, s)
        assert gt["arrived"] == 0 and gt["flag"] == gt["seq"] == red["seq"] + 1


@pytest.mark.gpu
def test_two_gates_in_one_script_each_deliver_their_own_verdict(ladder_group):
    grp, layout = ladder_group
    cs = conjunct_cases()
    off, common = cs[3], cs[0]
    script = []
    for c in (off, common, off):
        nodes = [c["node"] if a == 2 else node() for a in range(6)]
        script += launches_of(layout, nodes, c["opt"], twice=True)
    dev = grp.debug_cg_scalars(script)
    gates = [o for q, o in zip(script, dev) if q["kind"] == "reduce_gate"]
    assert [o["go"] for o in gates] == [0, 0, ALL_ONES, ALL_ONES, 0, 0]
    assert [o["h_gate"] for o in gates] == [0.0, 0.0, 1.0, 1.0, 0.0, 0.0]
    for i in range(0, 6, 2):
        assert gates[i + 1]["seq"] == gates[i]["seq"] + 1
    assert all(o["arrived"] == 0 and o["flag"] == o["seq"] for o in gates)


@pytest.mark.gpu
def test_the_hooks_refuse_arguments_outside_the_group(ladder_group):
    grp, layout = ladder_group
    good = launches_of(layout, [node() for _ in range(6)], BASE_OPT)
    for bad in (dict(good[3], gate=dict(good[3]["gate"], nslots=0)), dict(good[3], gate=dict(good[3]["gate"], nslots=MAX_SLOTS + 1)),
                dict(good[3], gate=None), dict(good[1], bits=1 << 6)):
        with pytest.raises(RuntimeError):
            grp.debug_cg_scalars(good[:2] + [bad])
    P = np.zeros((MAX_SLOTS, layout[0]))
    with pytest.raises(RuntimeError):
        grp.debug_star_sums(P, 1 << 6)
    with pytest.raises(RuntimeError):
        grp.debug_gated_update(1)          # neither 0 nor all ones
    with pytest.raises(RuntimeError):
        grp.debug_gated_update(0)          # the trivial loss, no step taken: not the state the hook is for


# ---------------------------------------------------------------------------------------------------------------------
# host and device on real data, forced off the common course

FORCED = {"defaults": {}, "psi": dict(psi=1e12), "phi": dict(phi=1e3),
          "second iteration": dict(max_iterations=2, max_iterations_accepted=2, rel_func_decrease_tol=0.0, stepsize_tol=0.0)}
LATTICE = (8, 8, 8, 2048, 2, 12)   # synthetic.grid(nx, ny, nz, num_edges), nodes, steps


FORCED_CODE = """
import sys, json, numpy as np
sys.path.insert(0, %r)
import dpgo_amd
from dpgo_amd import synthetic
nx, ny, nz, num_edges, nn, steps = json.loads(sys.argv[3])
g = synthetic.grid(nx, ny, nz, num_edges)
G = dpgo_amd.graph_from_edges(3, g["num_poses"], g["I"], g["J"], g["R"], g["t"], g["kappa"], g["tau"], nn)
drv = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(1, True, **json.loads(sys.argv[2])), X0=G.chordal_initialization())
for it in range(steps):
    assert drv.step() == 0
np.save(sys.argv[1], drv.X())
del drv
""" % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def forced_run(tmp_path, lattice, tag, kw, **env):
    """one run in a child process -> (X, speculations enqueued, of which stood)"""
    import json
    path = os.path.join(str(tmp_path), tag.replace(" ", "_") + ".npy")
    p = subprocess.run([sys.executable, "-c", FORCED_CODE, path, json.dumps(kw), json.dumps(lattice)], capture_output=True, text=True,
                       timeout=120, env=dict(dict(os.environ, DPGO_HOST_TIMING="1", DPGO_ITER_GRAPH="0"), **env))
    assert p.returncode == 0, p.stderr[-2000:]
    assert "disagree" not in p.stderr, p.stderr[-2000:]
    line = [l for l in p.stderr.splitlines() if "updates enqueued ahead" in l]
    assert line, p.stderr[-2000:]
    nums = [int(x) for x in line[-1].replace(",", " ").replace(":", " ").split() if x.isdigit()]
    return np.load(path), nums[-2], nums[-1]


@pytest.mark.gpu
def test_host_and_gate_agree_where_the_iteration_is_forced_off_course(tmp_path):
    """A lattice (LATTICE) with the Huber loss and Static rescale through step(), eager launches, under the driver's options
    and three sets that force one branch each -- psi = 1e12: every half step is redone; phi = 1e3: every refined step falls
    back; two trust-region iterations with zero tolerances: a second iteration always follows (the oracle's run of smallGrid3D
    under the same sets, tests/test_gate_restatement_host.py, shows each forcing its branch in every iteration).  Every run
    enqueues speculations, none stands under a forcing set, at least five stand under the defaults, host and gate never
    disagree (a disagreement fails the group: step() returns -1) and X is bit for bit the X of the run with
    DPGO_SPEC_UPDATE=0.

    Measured on synthetic.grid(8, 8, 8, 2048) in 2 nodes, 12 steps (enqueued / stood): defaults 6 / 5, psi 6 / 0, phi 11 / 0, second
    iteration 4 / 0.  The smallest that has five standing: grid(6, 6, 6, 864) stays at 5 / 4 up to 90 steps, and lattices
    without loop closures (num_edges left out) at 2 .. 4 / 1 .. 3 up to 20 x 20 x 16 in 8 nodes."""
    for tag, kw in FORCED.items():
        X, enq, stood = forced_run(tmp_path, LATTICE, tag, kw)
        X0, enq0, stood0 = forced_run(tmp_path, LATTICE, tag + " host", kw, DPGO_SPEC_UPDATE="0")
        print("%s: enqueued %d, stood %d" % (tag, enq, stood))
        assert enq0 == 0 and stood0 == 0
        assert enq > 0, (tag, enq, stood)
        if kw:
            assert stood == 0, (tag, enq, stood)
        else:
            assert stood >= 5, (tag, enq, stood)
        assert np.array_equal(X, X0), tag
