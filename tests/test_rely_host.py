"""Host side of the per-edge reliability (dpgo_amd/csrc/rely.h): the restatement (tests/rely_restatement.py) against what it
claims to predict -- the redundancies of a noise-free graph, and graphs re-solved without one edge -- the record arithmetic
through its debug hook against the long-double restatement, injected faults against the margins, and the C ABI.  No GPU.

The points are POLISHED on the host (tests/newton_restatement.py, anchor 0) from the converged points of
tests/test_certify_host.py and, for the d = 2 ladder, tests/test_polish_host.py; Sigma is numpy's inverse of the restated
anchored Hessian.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_restatement as cr  # noqa: E402
import newton_restatement as nr  # noqa: E402
import pairs_restatement as pr  # noqa: E402
import rely_restatement as rr  # noqa: E402
import test_certify_host as tch  # noqa: E402  (its converged points; none of its tests is imported)
import test_gpu_cert_proof as tp  # noqa: E402  (the d = 2 graph; none of its tests is imported)
import test_polish_host as tpol  # noqa: E402  (its points of the d = 2 graph; none of its tests is imported)

import dpgo_amd  # noqa: E402
from oracle import g2o as og  # noqa: E402
from oracle.hash import Options as OOptions  # noqa: E402
from oracle.problem import LOSS_NONE  # noqa: E402
from oracle.star import GlobalProblem  # noqa: E402

LD, U = pr.LD, pr.U
FIXTURES = ["tinyGrid3D", "smallGrid3D", "ladder2"]
_pt = {}


def problem_of(N, mm):
    return GlobalProblem(N, mm, 1, OOptions.driver(LOSS_NONE, True))


def covariance(M, X, d, anchor=0):
    """(Sigma in fp64, the factorisation's part of the bound of its entries) of the restated anchored Hessian at X."""
    A = nr.anchored_hessian(M, X, d, anchor)
    A = (A + A.T) / 2
    lam = np.linalg.eigvalsh(A)
    assert lam[0] > 0
    return np.linalg.inv(A), cr.C * U * float(lam[-1] / lam[0]) / float(lam[0])


def point(fixtures_dir, name):
    """dict(d, N, mm, M, X, Sigma, bS): a fixture at its polished point, anchor 0, computed once."""
    if name not in _pt:
        if name == "ladder2":
            _, N, mm, gp, _, _ = tp.ladder2()
            X = tpol.start_point(fixtures_dir, name, 300)[1]
        else:
            gp, _, X = tch.points(fixtures_dir, name)
            N, mm = og.read_g2o_file(os.path.join(fixtures_dir, name + ".g2o"))
        d = gp.d
        X, outcome = nr.polish(gp.M, X, d)[:2]
        assert outcome == nr.CONVERGED
        Sigma, bS = covariance(gp.M, X, d)
        _pt[name] = dict(d=d, N=N, mm=mm, M=gp.M, X=X, Sigma=Sigma, bS=bS)
    return _pt[name]


def edge_inputs(P, mm=None, Sigma=None, X=None, dtype=np.float64, fault=None):
    """Per edge of mm: (p, q, cand, rel, r) in dtype from Sigma's blocks at X (anchor 0)."""
    mm = P["mm"] if mm is None else mm
    Sigma = P["Sigma"] if Sigma is None else Sigma
    X = P["X"] if X is None else X
    d = P["d"]
    dof = cr.dof_of(d)
    out = []
    for e in range(len(mm.ipose)):
        p, q = int(mm.ipose[e]), int(mm.jpose[e])
        cand = rr.candidate_of(mm, e)
        rel, r = rr.rel_and_r(X, d, p, q, cand, pr.joint_of(Sigma, dof, p, q, 0), dtype, fault)
        out.append((p, q, cand, rel, r))
    return out


def restated_records(P, **kw):
    """The long-double records of every edge from fp64 Sigma: (list of rely_restatement.record dicts, the edge inputs)."""
    E = edge_inputs(P, dtype=LD, **kw)
    return [rr.record(rel, r, P["d"], c[2], c[3]) for _, _, c, rel, r in E], E


def noise_free(P, extra=None):
    """(mm, X, N) of the graph whose every measurement is the estimate's own relative pose at P's point; extra = (p, R, t): one
    more pose N, placed at T_p (R, t) and tied to p by that one (noise-free) edge -- a pendant edge."""
    d, N, mm, X = P["d"], P["N"], P["mm"], P["X"]
    I, J = [int(v) for v in mm.ipose], [int(v) for v in mm.jpose]
    kappa, tau = list(mm.kappa), list(mm.tau)
    if extra is not None:
        p, Rn, tn = extra
        tp_, Yp = pr.record(X, d, p)
        Yn = (Yp.T @ Rn).T
        X = np.concatenate([X[:N], (tp_ + Yp.T @ tn)[None, :], X[N:], Yn])
        I.append(p), J.append(N), kappa.append(20.0), tau.append(10.0)
        N = N + 1
    rel = [pr.relative(X, d, p, q, LD) for p, q in zip(I, J)]
    z = np.zeros(len(I), np.int64)
    mm0 = og.Measurements(z, I, z, J, np.stack([np.asarray(r[0], np.float64) for r in rel]),
                          np.stack([np.asarray(r[1], np.float64) for r in rel]), kappa, tau)
    return mm0, X, N


# ---------------------------------------------------------------------------------------------------------------
# (a) a graph without noise: the redundancies sum to dof (m - N + 1), nothing disagrees, a pendant edge is not checked
# ---------------------------------------------------------------------------------------------------------------
def test_noise_free_graph_and_a_pendant_edge(fixtures_dir):
    P = point(fixtures_dir, "smallGrid3D")
    d, dof = P["d"], cr.dof_of(P["d"])
    for extra in (None, (P["N"] - 1, np.asarray(pr.exp_so([0.1, -0.2, 0.3], 3), np.float64), np.array([1.0, 0.0, 0.5]))):
        mm0, X, N = noise_free(P, extra)
        M = problem_of(N, mm0).M
        assert nr.objective(M, X) <= 1e-20 * len(mm0.ipose)   # (the same reading of (R~, t~) as the objective's)
        Sigma, bS = covariance(M, X, d)
        Q = dict(P, mm=mm0, X=X, N=N, Sigma=Sigma)
        recs, E = restated_records(Q)
        m = len(recs)
        total = float(sum(r["redundancy"] for r in recs))
        print("noise-free smallGrid3D%s: sum of redundancies %.12f, dof (m - N + 1) = %d"
              % (" with a pendant edge" if extra else "", total, dof * (m - N + 1)))
        assert abs(total - dof * (m - N + 1)) <= 1e-9
        for rec, (p, q, c, rel, r) in zip(recs, E):
            if rec["flag"] != 0:
                continue
            Sj = pr.joint_of(Sigma, dof, p, q, 0)
            mg = rr.margins(rec, rel, d, c[2], c[3], pr.margin_rel(X, d, p, q, Sj, bS), pr.margin_residual(X, d, p, q, c))
            assert float(rec["d2_loo"]) <= mg[0]
        if extra:
            print("  the pendant edge: redundancy %.3g, lambda_min(C) Omega_min %.3g"
                  % (float(recs[-1]["redundancy"]), recs[-1]["lam_min"] * recs[-1]["omega_min"]))
            assert abs(float(recs[-1]["redundancy"])) <= 1e-12 and abs(float(recs[-1]["redundancy_trans"])) <= 1e-12


# ---------------------------------------------------------------------------------------------------------------
# (b) the graph re-solved without one edge
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", [208, 155, 233])
def test_leave_one_out_against_the_resolved_graph(fixtures_dir, e):
    """smallGrid3D without edge e, polished again from the full graph's point: twice the drop of the optimum against d2_loo,
    and the edge's residual at the new point against r_loo.  Both are first-order statements (a Gauss-Newton step of the
    reduced problem), so the bound is the model's error, not rounding.  Measured:
        edge   2 (F* - F*_-e)   d2_loo    |d2_loo - 2 dF| / 2 dF   |r_loo - r2| / |r2|   |r - r2| / |r2|   |r| / |r2|
        208    0.5851           0.5865    0.0023                   0.0067                0.361             0.708
        155    5.4683           5.4031    0.0119                   0.0424                0.429             0.644
        233    21.8799          22.6666   0.0360                   0.0554                0.776             0.367
    0.10 is about twice the worst of either; |r - r2| / |r2| >= 0.25 says the plain residual would not pass."""
    P = point(fixtures_dir, "smallGrid3D")
    d, mm, X = P["d"], P["mm"], P["X"]
    recs, E = restated_records(P)
    p, q, cand, _, r = E[e]
    keep = np.arange(len(mm.ipose)) != e
    mm_e = og.Measurements(mm.inode[keep], mm.ipose[keep], mm.jnode[keep], mm.jpose[keep], mm.R[keep], mm.t[keep], mm.kappa[keep],
                           mm.tau[keep])
    M_e = problem_of(P["N"], mm_e).M
    X_e, outcome = nr.polish(M_e, X, d)[:2]
    assert outcome == nr.CONVERGED
    dF2 = 2 * (nr.objective(P["M"], X) - nr.objective(M_e, X_e))
    r2 = np.asarray(pr.residual(X_e, d, p, q, cand, LD), np.float64)
    r_loo, r = np.asarray(recs[e]["r_loo"], np.float64), np.asarray(r, np.float64)
    got = (abs(float(recs[e]["d2_loo"]) - dF2) / dF2, np.linalg.norm(r_loo - r2) / np.linalg.norm(r2),
           np.linalg.norm(r - r2) / np.linalg.norm(r2))
    print("edge %d: 2 dF %.4f, d2_loo %.4f (%.4f of it apart); |r_loo - r2| / |r2| %.4f, |r - r2| / |r2| %.3f, |r| / |r2| %.3f"
          % (e, dF2, float(recs[e]["d2_loo"]), got[0], got[1], got[2], np.linalg.norm(r) / np.linalg.norm(r2)))
    assert recs[e]["flag"] == 0 and got[0] <= 0.10 and got[1] <= 0.10 and got[2] >= 0.25


# ---------------------------------------------------------------------------------------------------------------
# (c) the record arithmetic of the library on the host against the long-double restatement
# ---------------------------------------------------------------------------------------------------------------
def compare(d, lib, rel, r, kappa, tau, m_rel=None, m_r=None):
    """(worst error / margin over the entries of one record, the restated record, flags agree) -- where the restated flag is one
    rounding decides and the library's differs, only the entries that do not depend on it are compared."""
    dof = cr.dof_of(d)
    ref = rr.record(rel, r, d, kappa, tau)
    want, m = rr.vector(ref, d), rr.margins(ref, rel, d, kappa, tau, m_rel, m_r)
    same = int(lib[1]) == ref["flag"]
    idx = np.arange(rr.width(d)) if same else np.array([2, 3, 4] + list(range(6, 6 + dof)))
    idx = idx[idx != 1]
    err = np.abs(np.asarray(lib, LD) - want)[idx]
    return float(np.max(np.where(err == 0, 0.0, np.asarray(err, np.float64) / (m[idx] + 1e-300)))), ref, same


@pytest.mark.parametrize("name", FIXTURES)
def test_record_arithmetic_against_the_restatement(fixtures_dir, name):
    P = point(fixtures_dir, name)
    d = P["d"]
    E = edge_inputs(P)
    lib = dpgo_amd.rely_edge_debug(d, [x[3] for x in E], [x[4] for x in E], [x[2][2] for x in E], [x[2][3] for x in E])
    worst, flagged, undecided = 0.0, [], 0
    for e, (p, q, c, rel, r) in enumerate(E):
        w, ref, same = compare(d, lib[e], rel, r, c[2], c[3])
        worst = max(worst, w)
        if rr.decided(ref):
            assert same, (e, lib[e][1], ref["flag"], ref["lam_min"] * ref["omega_min"])
        else:
            undecided += 1
        if lib[e][1] == 1:
            flagged.append(e)
            assert lib[e][0] == 0 and lib[e][5] == 0 and not lib[e][6 + cr.dof_of(d):].any()
    print("%s: %d edges, worst error / margin %.3g, flagged %s, %d left to rounding" % (name, len(E), worst, flagged if len(flagged) <= 12 else "%d edges" % len(flagged), undecided))
    assert worst <= 1.0
    if name == "smallGrid3D":
        assert undecided == 0 and flagged == []
    if name == "tinyGrid3D":
        assert flagged == [0, 1, 2, 7, 8]


@pytest.mark.parametrize("d", [2, 3])
def test_record_arithmetic_on_seeded_residual_covariances(d):
    """C = Q diag(lambda) Q^T with kappa_2(C) = 1, 1e2, 1e4, 1e6, 1e8 and seeded r; C with a negative eigenvalue; an edge without
    weight."""
    dof = cr.dof_of(d)
    rng = np.random.default_rng(1000 + d)
    rels, rs, ks, ts = [], [], [], []
    for k in (0, 2, 4, 6, 8):
        for _ in range(6):
            Q = np.linalg.qr(rng.standard_normal((dof, dof)))[0]
            kappa, tau = float(rng.uniform(5, 50)), float(rng.uniform(5, 50))
            Cm = (Q * (0.02 * np.logspace(0, -k, dof))) @ Q.T
            rels.append(np.diag(1 / np.diag(pr.omega(d, kappa, tau))) - (Cm + Cm.T) / 2)
            rs.append(rng.standard_normal(dof) * 0.1)
            ks.append(kappa), ts.append(tau)
    n_pd = len(rels)
    for _ in range(4):   # C indefinite, clear of zero
        Q = np.linalg.qr(rng.standard_normal((dof, dof)))[0]
        lam = 0.02 * np.ones(dof)
        lam[int(rng.integers(0, dof))] = -0.01
        rels.append(np.eye(dof) / 20.0 - (Q * lam) @ Q.T)
        rs.append(rng.standard_normal(dof) * 0.1)
        ks.append(10.0), ts.append(20.0)
    for kappa, tau in ((0.0, 3.0), (3.0, 0.0), (-1.0, 2.0), (float("nan"), 1.0)):
        rels.append(rels[0]), rs.append(rs[0]), ks.append(kappa), ts.append(tau)
    lib = dpgo_amd.rely_edge_debug(d, rels, rs, ks, ts)
    worst = 0.0
    for e in range(len(rels)):
        w, ref, same = compare(d, lib[e], rels[e], rs[e], ks[e], ts[e])
        assert same, e   # (lambda_min(C) is 2e-10 at the least here and the inputs are exact: the sign is not rounding's)
        assert ref["flag"] == (0 if e < n_pd else 1 if e < n_pd + 4 else 2)
        worst = max(worst, w)
    assert not lib[n_pd + 4:, 0].any() and not lib[n_pd + 4:, 2:].any()
    print("d = %d: %d seeded records, worst error / margin %.3g" % (d, len(rels), worst))
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------------------
# (d) injected faults
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fault", rr.FAULTS)
def test_an_injected_fault_is_caught_by_a_margin(fixtures_dir, fault):
    """The restated step with one mistake, on every edge of smallGrid3D, against the margins a device result is held to (bS: the
    factorisation's part): the entry the mistake touches leaves its margin on every edge that can show it."""
    P = point(fixtures_dir, "smallGrid3D")
    d, dof, X = P["d"], cr.dof_of(P["d"]), P["X"]
    field = dict(plus=0, kappa=0, no_omega=slice(6 + dof, 6 + 2 * dof), trace=2, transpose=0)[fault]
    caught = 0
    E = edge_inputs(P, dtype=LD)
    Ef = edge_inputs(P, dtype=LD, fault=fault) if fault == "transpose" else E
    for (p, q, c, rel, r), (_, _, _, relf, rf) in zip(E, Ef):
        ref = rr.record(rel, r, d, c[2], c[3])
        bad = rr.record(relf, rf, d, c[2], c[3], fault=None if fault == "transpose" else fault)
        Sj = pr.joint_of(P["Sigma"], dof, p, q, 0)
        m = rr.margins(ref, rel, d, c[2], c[3], pr.margin_rel(X, d, p, q, Sj, P["bS"]), pr.margin_residual(X, d, p, q, c))
        err = np.abs(rr.vector(bad, d) - rr.vector(ref, d))
        caught += bool(np.any(np.asarray(err, np.float64)[field] > m[field]))
    print("%s: caught on %d of %d edges" % (fault, caught, len(E)))
    # (S_pq is zero for the edges at the anchor: nothing to transpose there)
    at_anchor = sum(1 for x in E if 0 in x[:2])
    assert caught >= len(E) - (at_anchor if fault == "transpose" else 0)


# ---------------------------------------------------------------------------------------------------------------
# (e) C ABI
# ---------------------------------------------------------------------------------------------------------------
def test_rely_abi():
    assert (dpgo_amd.RELY_OK, dpgo_amd.RELY_NOT_PD, dpgo_amd.RELY_SKIPPED) == (0, 1, 2)
    assert (dpgo_amd.RELY_AUTO, dpgo_amd.RELY_SELINV, dpgo_amd.RELY_SOLVE) == (0, 1, 2)
    # twelve ints, three long longs, eight doubles
    assert C.sizeof(dpgo_amd.RelyResult) == 48 + 24 + 64
    assert [f[0] for f in dpgo_amd.RelyResult._fields_] == [
        "outcome", "method_used", "unknowns", "fronts", "levels", "max_front", "edges", "flagged", "unweighted", "columns", "batches",
        "reserved", "device_bytes", "device_bytes_selinv", "device_bytes_solve", "redundancy_sum", "pivot_min", "pivot_max",
        "stationarity", "symbolic_s", "factor_ms", "inverse_ms", "edge_ms"]
    L = dpgo_amd.lib()
    header = open(os.path.join(os.path.dirname(dpgo_amd.__file__), "..", "include", "dpgo_amd.h")).read()
    for sym in ("dpgo_group_edge_reliability", "dpgo_graph_edge_reliability_reweighted", "dpgo_debug_rely_edge_host",
                "dpgo_debug_rely_edge"):
        assert sym + "(" in header and sym in dpgo_amd.SYMBOLS and hasattr(L, sym)
    for name in ("DPGO_RELY_OK 0", "DPGO_RELY_NOT_PD 1", "DPGO_RELY_SKIPPED 2", "DPGO_RELY_AUTO 0", "DPGO_RELY_SELINV 1",
                 "DPGO_RELY_SOLVE 2"):
        assert "#define " + name in header
    for name in ("edge_reliability",):
        assert callable(getattr(dpgo_amd.NodeGroup, name))
    assert callable(dpgo_amd.edge_reliability_reweighted) and callable(dpgo_amd.rely_edge_debug)
    facade = open(os.path.join(os.path.dirname(dpgo_amd.__file__), "..", "include", "dpgo_amd.hpp")).read()
    assert "edge_reliability(" in facade
    X = np.zeros((8, 3), order="F")
    dp = X.ctypes.data_as(C.POINTER(C.c_double))
    r = dpgo_amd.RelyResult()
    # no group, no graph, no output
    assert L.dpgo_group_edge_reliability(None, None, dp, 8, 0, 0, 0, None, 0, dp, None, None, C.byref(r)) == -1
    assert L.dpgo_graph_edge_reliability_reweighted(None, 0, dp, 8, 0, 0.25, 0, 0, 0, None, 0, dp, None, None, C.byref(r), None) == -1
    G = dpgo_amd.graph_from_edges(2, 2, [0], [1], [np.eye(2)], [np.zeros(2)], [1.0], [1.0], 1)
    assert L.dpgo_graph_edge_reliability_reweighted(G._h, 0, None, 8, 0, 0.25, 0, 0, 0, None, 0, dp, None, None, C.byref(r), None) == -1
    assert L.dpgo_graph_edge_reliability_reweighted(G._h, 0, dp, 8, 0, 0.25, 0, 0, 0, None, 0, None, None, None, C.byref(r), None) == -1
    assert L.dpgo_graph_edge_reliability_reweighted(G._h, 0, dp, 8, 0, 0.25, 0, 0, 0, None, 0, dp, None, None, None, None) == -1
    # the host hook: null arrays, a dimension that is neither 2 nor 3
    rec = np.zeros(18)
    rp = rec.ctypes.data_as(C.POINTER(C.c_double))
    assert L.dpgo_debug_rely_edge_host(3, 1, None, dp, dp, dp, rp) == -1 and L.dpgo_debug_rely_edge_host(3, 1, dp, None, dp, dp, rp) == -1
    assert L.dpgo_debug_rely_edge_host(3, 1, dp, dp, None, dp, rp) == -1 and L.dpgo_debug_rely_edge_host(3, 1, dp, dp, dp, None, rp) == -1
    assert L.dpgo_debug_rely_edge_host(3, 1, dp, dp, dp, dp, None) == -1 and L.dpgo_debug_rely_edge_host(4, 1, dp, dp, dp, dp, rp) == -1
    assert L.dpgo_debug_rely_edge_host(3, -1, dp, dp, dp, dp, rp) == -1
    with pytest.raises(ValueError):
        dpgo_amd.rely_edge_debug(3, np.zeros((2, 6, 6)), np.zeros((1, 6)), 1.0, 1.0)
