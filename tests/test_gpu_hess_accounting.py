"""What the consumers of the anchored tangent-space Hessian's factor (dpgo_amd/csrc/hess.h) report and in which order they may be
called: covariance, pair_covariance, sensitivity, robust_sensitivity, edge_reliability, polish, robust_polish,
robust_covariance and gnc on the smallest case of tests/test_gpu_covariance.py in d = 2 and in d = 3.

  accounting   every entry point with max_bytes = 1 (SKIPPED) and unlimited, one group per case; the integer and byte fields of
               every result struct -- the analysis' sizes, the predicted device bytes, the column plans: all computed on the
               host, none of them a floating-point result -- equal tests/golden/hess_accounting.json, recorded by
               tests/golden/make_hess_accounting.py with the build BEFORE the setup, the refusal and the verdict of these
               entry points were stated once.  (gnc's `levels` counts continuation levels, not the factor's: not recorded.)
  order        pair_covariance, covariance, edge_reliability(SELINV), sensitivity, polish on one group, and in the reverse
               order on a fresh one: what a call computes does not depend on what an earlier call left on the device (the
               numeric context, the blocks of the selected inversion, polish's vectors) -- every output array, the pivots and
               the stationarity are bitwise equal.
"""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_cert_proof as tp  # noqa: E402  (the instances; none of its tests is imported)
import test_gpu_covariance as tcov  # noqa: E402  (its cases and converged points; likewise)

import dpgo_amd  # noqa: E402
from oracle.problem import LOSS_HUBER  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hess_accounting.json")
CASES = [("ladder2", 6), ("tinyGrid3D", 1)]   # the smallest of tests/test_gpu_covariance.py's CASES in d = 2 and in d = 3
assert all(c in tcov.CASES for c in CASES)
FIELDS = ("outcome", "unknowns", "fronts", "levels", "max_front", "device_bytes", "device_bytes_selinv", "device_bytes_solve",
          "method_used", "columns", "batches", "edges", "unweighted")
SENS_BATCH = 64   # dpgo_amd/csrc/sens.h


def fields_of(r):
    skip = ("levels",) if isinstance(r, dpgo_amd.GncResult) else ()
    return {f: int(getattr(r, f)) for f in FIELDS if f in dict(r._fields_) and f not in skip}


def upstream(n, k):
    return np.asfortranarray(np.cos(1.0 + np.arange(n * k, dtype=np.float64)).reshape(n, k))


def entry_points(grp, X, N, d):
    """label -> call(max_bytes) -> the call's result struct, in the order they are run."""
    dof = d + d * (d - 1) // 2
    G = grp.graph
    pairs = np.array([[0, 1], [2, N - 1], [1, 5]], np.int32)   # (0, 1) names the anchor
    rset = (np.arange(G.num_edges) % 3 == 0).astype(np.int32)
    E = {
        "covariance": lambda mb: grp.covariance(X, max_bytes=mb)[2],
        "pair_covariance": lambda mb: grp.pair_covariance(X, pairs, max_bytes=mb)["result"],
        "sensitivity_1": lambda mb: grp.sensitivity(X, upstream(dof * N, 1), max_bytes=mb)[0],
        "sensitivity_batch_plus_1": lambda mb: grp.sensitivity(X, upstream(dof * N, SENS_BATCH + 1), max_bytes=mb)[0],
        "robust_sensitivity_huber": lambda mb: grp.robust_sensitivity(X, upstream(dof * N, 2), LOSS_HUBER, max_bytes=mb)[0],
    }
    for m, name in sorted(dpgo_amd.RELY_METHOD_NAMES.items()):
        E["edge_reliability_" + name] = lambda mb, m=m: grp.edge_reliability(X, method=m, max_bytes=mb)["result"]
    E["polish"] = lambda mb: grp.polish(X, max_bytes=mb)[1]
    E["robust_polish"] = lambda mb: grp.robust_polish(X, LOSS_HUBER, max_bytes=mb)[1]
    E["robust_covariance"] = lambda mb: grp.robust_covariance(X, LOSS_HUBER, max_bytes=mb)[2]
    E["gnc"] = lambda mb: grp.gnc(G, X, dpgo_amd.GncOptions(max_levels=3), robust_set=rset, max_bytes=mb)[2]
    return E


def record(fixtures_dir, name, nn):
    """One group: every entry point refused (nothing of the factor on the device yet), then every entry point unlimited."""
    N, mm = tp.instance(fixtures_dir, name)[:2]
    X = tcov.converged(fixtures_dir, name)
    E = entry_points(tcov.make_group(fixtures_dir, name, nn), X, N, mm.d)
    out = {label: {"skipped": fields_of(call(1))} for label, call in E.items()}
    for label, call in E.items():
        out[label]["unlimited"] = fields_of(call(0))
    return out


@pytest.mark.parametrize("name,nn", CASES)
def test_accounting_equals_the_recorded(fixtures_dir, name, nn):
    with open(GOLDEN) as f:
        want = json.load(f)["%s/%d" % (name, nn)]
    got = record(fixtures_dir, name, nn)
    assert sorted(got) == sorted(want)
    for label in want:
        for mode in ("skipped", "unlimited"):
            for field, v in want[label][mode].items():
                assert got[label][mode][field] == v, (label, mode, field, got[label][mode][field], v)
            assert sorted(got[label][mode]) == sorted(want[label][mode]), (label, mode)


def ordered_calls(fixtures_dir):
    name, nn = CASES[1]
    N, mm = tp.instance(fixtures_dir, name)[:2]
    d = mm.d
    dof = d + d * (d - 1) // 2
    X = tcov.converged(fixtures_dir, name)
    edges = np.unique(np.stack([np.asarray(mm.ipose), np.asarray(mm.jpose)], axis=1), axis=0).astype(np.int32)[:3]
    pairs = np.array([[0, 1], [2, N - 1], [1, 5]], np.int32)
    U = upstream(dof * N, 3)

    def scalars(r):
        return [np.array([r.pivot_min, r.pivot_max] + ([r.stationarity] if "stationarity" in dict(r._fields_) else []))]

    def pair_covariance(grp):
        o = grp.pair_covariance(X, pairs)
        return [o["joint"], o["rel"]] + scalars(o["result"])

    def covariance(grp):
        marg, cross, r = grp.covariance(X, pairs=edges)
        return [marg, cross] + scalars(r)

    def edge_reliability(grp):
        o = grp.edge_reliability(X, method=dpgo_amd.RELY_SELINV)
        return [o["records"], o["rel"], o["joint"]] + scalars(o["result"])

    def sensitivity(grp):
        r, sens, adj = grp.sensitivity(X, U, want_adjoint=True)
        return [sens, adj] + scalars(r)

    def polish(grp):
        Xout, r, log = grp.polish(X)
        return [Xout, np.asarray(log, np.float64)] + scalars(r)

    return (name, nn), [pair_covariance, covariance, edge_reliability, sensitivity, polish]


def test_outputs_do_not_depend_on_the_order_of_the_calls(fixtures_dir):
    (name, nn), calls = ordered_calls(fixtures_dir)
    fwd_grp, rev_grp = tcov.make_group(fixtures_dir, name, nn), tcov.make_group(fixtures_dir, name, nn)
    fwd = {c.__name__: c(fwd_grp) for c in calls}
    rev = {c.__name__: c(rev_grp) for c in reversed(calls)}
    for c in calls:
        for i, (a, b) in enumerate(zip(fwd[c.__name__], rev[c.__name__])):
            a, b = np.asarray(a), np.asarray(b)
            assert a.shape == b.shape and np.isfinite(a).all()
            diff = float(np.max(np.abs(a - b))) if a.size else 0.0
            print("%-18s output %d: max |forward - reverse| = %.3g" % (c.__name__, i, diff))
            assert a.tobytes() == b.tobytes(), (c.__name__, i, diff)
