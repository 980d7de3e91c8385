"""tests/stpcg_restatement.py -- the restatement the device's CG control is held to (tests/test_gpu_cg_scalars.py) -- pinned on
the host: driven with sums formed in numpy from the vectors of every known-answer STPCG case of the reference
(tests/golden/tnt_ref.jsonl), with the vector updates s += c1 p, r += cr H p, p = -v + be p replayed from its coefficients,
it must reproduce the recorded step, step norm and iteration count, through the exit the case is about.  The kernel branch,
which no recorded case takes, is checked against oracle.tnt.stpcg on a diagonal H with a zero eigen-direction.  No GPU."""
import json
import math
import os

import numpy as np
import pytest

import stpcg_restatement as R
from oracle import tnt as T


def _cases(golden_dir):
    with open(os.path.join(golden_dir, "tnt_ref.jsonl")) as fh:
        return [c for c in map(json.loads, fh) if c["kind"] == "stpcg"]


def replay(g, Hd, Md, Delta, max_it, kappa, theta):
    """One STPCG of a one-node group the way tnt.cpp strings it together (host start): the restatement decides, numpy does
    the vector work.  Returns (s, h_M_norm, cg_it, the exits taken, the smallest margin, the Control -- its `final`: what the last deciding launch left)."""
    P = (lambda v: v) if Md is None else (lambda v: v / Md)
    r = g.copy()
    v = P(r)
    p = -v
    rv = float(r @ v)
    r0 = R.c_sqrt(rv)
    target = r0 * min(kappa, math.pow(r0, theta)) if rv >= 0 else float("nan")
    C = R.Control(1)
    C.begin_host(1, [rv], [Delta], [target], max_it)
    exits, margin, C.final = [C.last[0].exit], C.min_margin()[0], C.last[0]
    s = np.zeros_like(g)
    while C.dmask[0] & 1:
        Hp = Hd * p
        C.phase0([[float(p @ Hp), float(Hp @ Hp), float(p @ p), float(p @ r)]])
        exits.append(C.last[0].exit)
        margin = min(margin, C.min_margin()[0])
        c, C.final = C.rec[0], C.last[0]
        s = s + c["c1"] * p
        if c["cr"] != 0.0:
            r = r + c["cr"] * Hp
        if not C.dmask[1] & 1:
            C.phase1([[float("nan")]])   # (the surplus launch: nobody is in dmask[1], nothing is read)
            assert C.dmask[0] == 0
            break
        v = P(r)
        C.phase1([[float(r @ v)]])
        exits.append(C.last[0].exit)
        margin = min(margin, C.min_margin()[0])
        C.final = C.last[0]
        p = -v + C.rec[0]["be"] * p
    return s, C.rec[0]["h_M_norm"], C.rec[0]["cg_it"], exits, margin, C


# the exit every recorded case is about (the last decision of the run)
EXITS = {
    "ExactSTPCG": R.EXIT_LIMIT,
    "ExactSTPCGwithNegativeCurvature": R.EXIT_CURVATURE,
    "ExactSTPCGwithPreconditioning": R.EXIT_TARGET,
    "ExactSTPCGwithNegativeCurvatureAndPreconditioning": R.EXIT_CURVATURE,
    "RadiusLimited": R.EXIT_BOUNDARY,
    "RadiusLimitedPrecon": R.EXIT_BOUNDARY,
    "Truncated": R.EXIT_TARGET,
    "TruncatedPrecon": R.EXIT_TARGET,
    "Large40": R.EXIT_TARGET,
    "Large40Precon": R.EXIT_TARGET,
    "Large40PreconRadius": R.EXIT_BOUNDARY,
}


def test_restatement_reproduces_the_recorded_stpcg_cases(golden_dir):
    cases = _cases(golden_dir)
    assert sorted(c["case"] for c in cases) == sorted(EXITS)
    for c in cases:
        g, Hd = np.array(c["g"]), np.array(c["Hdiag"])
        Md = np.array(c["Mdiag"]) if "Mdiag" in c else None
        s, nrm, nit, exits, margin, C = replay(g, Hd, Md, c["Delta"], c["max_it"], c["kappa"], c["theta"])
        assert nit == c["num_iterations"], c["case"]
        if nrm == c["Delta"]:
            assert nrm == c["step_norm"], c["case"]
        else:
            assert abs(nrm - c["step_norm"]) <= 1e-14 * abs(c["step_norm"]), (c["case"], nrm, c["step_norm"])
        sref = np.array(c["s"])
        assert np.linalg.norm(s - sref) <= 1e-12 * np.linalg.norm(sref), (c["case"], s, sref)
        assert exits[-1] == EXITS[c["case"]], (c["case"], exits)
        assert exits[0] == R.EXIT_LIVE and all(e == R.EXIT_STEP for e in exits[1:-1:2]) and all(e == R.EXIT_GO_ON for e in exits[2:-1:2])
        # a stop at phase 0 is ordinal 2 cg_it + 1 with h_M_norm = Delta, one at phase 1 is 2 cg_it
        rec = C.rec[0]
        if exits[-1] in (R.EXIT_BOUNDARY, R.EXIT_CURVATURE, R.EXIT_KERNEL):
            assert rec["stop_ord"] == 2 * nit + 1 and rec["cr"] == 0.0 and rec["h_M_norm"] == c["Delta"]
        else:
            assert rec["stop_ord"] == 2 * nit
        assert C.dmask == [0, 0, 1] and C.cg_summary[0] == [float(rec["stop_ord"]), rec["h_M_norm"], float(nit)]
        assert margin >= 1e-6, (c["case"], margin)


def test_every_stored_double_is_within_its_bound_of_the_exact_value(golden_dir):
    """The running bound covers the restatement's own rounding: |double - mpmath| <= bound for every computed field."""
    for c in _cases(golden_dir):
        g, Hd = np.array(c["g"]), np.array(c["Hdiag"])
        Md = np.array(c["Mdiag"]) if "Mdiag" in c else None
        C = replay(g, Hd, Md, c["Delta"], c["max_it"], c["kappa"], c["theta"])[5]
        nd = C.final
        for f, b in nd.bound.items():
            assert abs(C.rec[0][f] - float(nd.exact[f])) <= b, (c["case"], f)


def _oracle(g, Hd, Md, Delta, max_it=50, kappa=1e-3, theta=0.9):
    P = None if Md is None else (lambda v: v / Md)
    with np.errstate(all="ignore"):
        return T.stpcg(g, lambda v: Hd * v, lambda a, b: float(a @ b), Delta, max_it, kappa, theta, P)


# H = diag(h, 0): the second CG direction lies in the kernel of H (conjugacy), with sk_M_pk != 0 by then; H = 0: the first one
# does, with sk_M_pk = 0.  <p, r> = -<r, P r> + ... is negative for a positive definite preconditioner; an indefinite one
# (Mdiag of both signs, <g, P g> > 0) makes it positive at the second step.  At the first step <p, r> = -<g, P g> > 0 means
# pk_M_2 < 0 and a negative discriminant: the reference returns NaN there, and so must the restatement.  (At the second step
# pk_M_2 < 0 as well: the radius sits just outside the first step, where the discriminant is still positive.)
KERNEL_CASES = [
    ("first step, <p,r> < 0", [3.0, -4.0], [0.0, 0.0], None, 2.0, 0, -1, True),
    ("first step, <p,r> > 0", [3.0, -4.0], [0.0, 0.0], [-1.0, -1.0], 2.0, 0, +1, True),
    ("second step, <p,r> < 0", [3.0, 0.5], [2.0, 0.0], None, 50.0, 1, -1, False),
    ("second step, <p,r> < 0, preconditioned", [3.0, 0.5], [2.0, 0.0], [4.0, 0.5], 50.0, 1, -1, False),
    ("second step, <p,r> > 0", [3.0, 0.5], [2.0, 0.0], [1.0, -8.0], 1.4935, 1, +1, False),
]


@pytest.mark.parametrize("name,g,Hd,Md,Delta,nit,sign,zero_skpk", KERNEL_CASES, ids=[k[0] for k in KERNEL_CASES])
def test_kernel_branch_against_the_oracle(name, g, Hd, Md, Delta, nit, sign, zero_skpk):
    g, Hd = np.array(g), np.array(Hd)
    Md = None if Md is None else np.array(Md)
    s, nrm, it, exits, margin, C = replay(g, Hd, Md, Delta, 50, 1e-3, 0.9)
    so, no, ito = _oracle(g, Hd, Md, Delta)
    assert exits[-1] == R.EXIT_KERNEL and it == ito == nit and nrm == no == Delta
    rec = C.rec[0]
    assert rec["stop_ord"] == 2 * nit + 1 and rec["cr"] == 0.0 and not rec["live"]
    took = dict(C.final.margins)
    assert "<p, r> < 0" in took and "kappa_k <= 0" not in took
    if np.all(np.isnan(so)):
        assert name == "first step, <p,r> > 0" and math.isnan(rec["c1"]) and np.all(np.isnan(s))
        return
    # which way the direction was turned: c1 = sgn sigma, and sigma > 0 where pk_M_2 > 0 (the match with the oracle's step
    # pins it in either case)
    if rec["pk_M_2"] > 0:
        assert math.copysign(1.0, rec["c1"]) == sign
    assert (rec["sk_M_pk"] == 0.0) == zero_skpk
    assert np.linalg.norm(s - so) <= 1e-12 * np.linalg.norm(so), (s, so)
    assert margin >= 1e-6


def _record(sk_M_pk, sk_M_2, pk_M_2, Delta):
    c = R.new_record()
    c.update(sk_M_pk=sk_M_pk, sk_M_2=sk_M_2, pk_M_2=pk_M_2, rv=1.0, Delta=Delta, Delta_2=Delta * Delta, target=1e-3, live=1,
             cg_it=2, max_it=10)
    return c


@pytest.mark.parametrize("pr", [-3.0, 3.0])
@pytest.mark.parametrize("sk_M_pk", [0.0, 0.75, -0.75])
def test_kernel_branch_on_hand_made_records(pr, sk_M_pk):
    """<Hp, Hp> = 0: the stored sk_M_pk changes sign with <p, r> < 0, and c1 = sgn sigma with sigma the positive root of
    |s + sigma (sgn p)|_M = Delta -- checked in rational arithmetic on dyadic inputs."""
    from fractions import Fraction as F
    c = _record(sk_M_pk, 2.25, 4.0, 8.0)
    C = R.Control(1, [c], (1, 1, 0))
    C.phase0([[5.0, 0.0, 4.0, pr]])
    rec, nd = C.rec[0], C.last[0]
    sgn = -1 if pr < 0 else 1
    assert nd.exit == R.EXIT_KERNEL and rec["sk_M_pk"] == sgn * sk_M_pk
    assert rec["stop_ord"] == 5 and rec["cr"] == 0.0 and rec["h_M_norm"] == 8.0 and not rec["live"]
    assert C.dmask == [1, 0, 1] and C.cg_summary[0] == [5.0, 8.0, 2.0]
    # |s|^2 + 2 c <s, p>_M + c^2 |p|^2_M = Delta^2 at c = c1, with the ORIGINAL <s, p>_M
    c1 = F(rec["c1"])
    res = F(2.25) + 2 * c1 * F(sk_M_pk) + c1 * c1 * 4 - 64
    assert abs(res) <= 64 * 8 * 2.0 ** -53
    assert math.copysign(1.0, rec["c1"]) == sgn
    assert abs(rec["c1"] - float(nd.exact["c1"])) <= nd.bound["c1"]
    # the other fields are untouched
    for f in ("sk_M_2", "pk_M_2", "rv", "Delta", "Delta_2", "target", "al", "kap", "be"):
        assert rec[f] == c[f]


def test_a_stopped_node_is_left_alone_and_the_masks_hand_over():
    """Two nodes: node 0 stops at phase 0 (curvature), node 1 goes on; phase 1 then hands dmask[1] to dmask[0], and a further
    pair of launches changes neither node 0's record nor its summary."""
    C = R.Control(2)
    C.begin_host(3, [4.0, 9.0], [10.0, 10.0], [1e-3, 1e-3], 5)
    assert C.dmask == [3, 3, 0]
    C.phase0([[-2.0, 4.0, 4.0, -4.0], [18.0, 36.0, 9.0, -9.0]])
    assert [nd.exit for nd in C.last] == [R.EXIT_CURVATURE, R.EXIT_STEP] and C.dmask == [3, 2, 1]
    C.phase1([[float("nan")], [1.0]])
    assert C.dmask == [2, 2, 1] and C.last[0].exit == R.EXIT_NONE and C.last[1].exit == R.EXIT_GO_ON
    kept, summary = dict(C.rec[0]), list(C.cg_summary[0])
    C.phase0([[float("nan")] * 4, [3.0, 9.0, 1.5, -1.0]])
    C.phase1([[float("nan")], [0.25]])
    assert C.rec[0] == kept and C.cg_summary[0] == summary == [1.0, 10.0, 0.0]
