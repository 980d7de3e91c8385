"""Per-edge reliability on the device (dpgo_amd/csrc/rely.h): NodeGroup.edge_reliability on tinyGrid3D x {1, 2} nodes,
smallGrid3D x {1, 5} and the d = 2 ladder x 6 (tests/test_gpu_pairs.py's cases, polished points and references, imported, not
edited), anchors 0 and N - 1, under RELY_SELINV and RELY_SOLVE.

The reference is the long-double restatement (tests/rely_restatement.py) on the long-double inverse of the restated anchored H;
the bounds are its margins with bS = bSigma (tests/test_gpu_pairs.py): nothing in them comes from the device.  On the two grids
every edge is restated; on the ladder (1358 edges, 3 N unknowns) every 34th, the long-double inverse being solved for the
poses of those only.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_restatement as cr  # noqa: E402
import pairs_restatement as pr  # noqa: E402
import rely_restatement as rr  # noqa: E402
import test_gpu_certify as tc  # noqa: E402  (its inputs; none of its tests is imported)
import test_gpu_covariance as tgc  # noqa: E402  (its groups; none of its tests is imported)
import test_gpu_cert_proof as tp  # noqa: E402
import test_gpu_pairs as tgp  # noqa: E402  (its cases, polished points and references; none of its tests is imported)

import dpgo_amd  # noqa: E402
from dpgo_amd import RELY_AUTO, RELY_SELINV, RELY_SOLVE  # noqa: E402
from oracle.problem import LOSS_NONE  # noqa: E402

pytestmark = pytest.mark.gpu

LD, U = pr.LD, pr.U
CASES = tgp.CASES
FLAGGED = {"tinyGrid3D": [0, 1, 2, 7, 8], "smallGrid3D": []}
_restated = {}


def restated(fixtures_dir, name, anchor, graph):
    """Computed once per (fixture, anchor): the edges of the graph, which of them are restated, and per restated edge the
    long-double record (rely_restatement.record), its vector, its margins and the long-double joint blocks."""
    key = (name, anchor)
    I, J, Rm, t, kappa, tau = graph.edges()
    if key not in _restated:
        R = tgp.reference(fixtures_dir, name, anchor)
        d, dof, X = R["d"], R["dof"], R["X"]
        m = len(I)
        sel = np.arange(m) if name != "ladder2" else np.arange(0, m, 34)
        pairs = [(int(I[e]), int(J[e])) for e in sel]
        tgp.need(R, pairs)
        recs, vecs, margs, joints = [], [], [], []
        for e, (p, q) in zip(sel, pairs):
            cand = (Rm[e], t[e], float(kappa[e]), float(tau[e]))
            Sj = pr.joint_of(R["Sigma"], dof, p, q, anchor)
            rel, r = rr.rel_and_r(X, d, p, q, cand, Sj, LD)
            ref = rr.record(rel, r, d, cand[2], cand[3])
            m_rel = pr.margin_rel(X, d, p, q, np.asarray(Sj, np.float64), R["bSigma"])
            recs.append(ref)
            vecs.append(rr.vector(ref, d))
            margs.append(rr.margins(ref, rel, d, cand[2], cand[3], m_rel, pr.margin_residual(X, d, p, q, cand)))
            joints.append(pr.blocks_of(Sj, dof))
        _restated[key] = dict(I=I, J=J, sel=sel, recs=recs, vecs=np.stack(vecs), margins=np.stack(margs), joints=np.stack(joints))
    Q = _restated[key]
    assert np.array_equal(Q["I"], I) and np.array_equal(Q["J"], J)   # (every partition: the same edges in the same order)
    return Q


def worst_ratio(Q, out, d):
    """(worst error / margin of the records over the restated edges, the edges whose flag differs from a DECIDED restated flag)."""
    dof = cr.dof_of(d)
    worst, wrong = 0.0, []
    for k, e in enumerate(Q["sel"]):
        ref, lib = Q["recs"][k], out["records"][e]
        same = int(lib[1]) == ref["flag"]
        if not same and rr.decided(ref):
            wrong.append(int(e))
        idx = np.arange(rr.width(d)) if same else np.array([2, 3, 4] + list(range(6, 6 + dof)))
        idx = idx[idx != 1]
        err = np.asarray(np.abs(np.asarray(lib, LD) - Q["vecs"][k]), np.float64)[idx]
        worst = max(worst, float(np.max(np.where(err == 0, 0.0, err / (Q["margins"][k][idx] + 1e-300)))))
    return worst, wrong


_first = {}


@pytest.mark.parametrize("name,nn", CASES)
def test_records_against_the_restatement(fixtures_dir, name, nn):
    grp = tgc.make_group(fixtures_dir, name, nn)
    N = tp.instance(fixtures_dir, name)[0]
    outs = {}
    for a in (0, N - 1):
        R = tgp.reference(fixtures_dir, name, a)
        d, dof = R["d"], R["dof"]
        Q = restated(fixtures_dir, name, a, grp.graph)
        m = len(Q["I"])
        for method in (RELY_SELINV, RELY_SOLVE):
            out = outs[(a, method)] = grp.edge_reliability(R["X"], anchor=a, method=method)
            res = out["result"]
            assert res.outcome == dpgo_amd.RELY_OK and res.method_used == method and res.edges == m and res.unweighted == 0
            assert res.unknowns == dof * N and res.fronts >= 1 and res.pivot_min > 0 and res.stationarity >= 0
            assert res.device_bytes == (res.device_bytes_selinv if method == RELY_SELINV else res.device_bytes_solve) > 0
            assert out["records"].shape == (m, 6 + 2 * dof) and np.all(np.isin(out["flag"], (0, 1)))
            worst, wrong = worst_ratio(Q, out, d)
            jw = float(np.abs(np.asarray(out["joint"][Q["sel"]], LD) - Q["joints"]).max()) / R["bSigma"]
            print("%s x %d, anchor %d, %s: records %.3g of their margins, joint %.3g of bSigma, %d flagged, sum of redundancies %.6f"
                  % (name, nn, a, dpgo_amd.RELY_METHOD_NAMES[method], worst, jw, res.flagged, res.redundancy_sum))
            assert worst < 1.0 and jw < 1.0 and wrong == []
            # flags and their zeros; the count; the host's sum, bit for bit
            fl = out["flag"] == 1
            assert res.flagged == int(fl.sum())
            assert not out["d2_loo"][fl].any() and not out["influence"][fl].any() and not out["r_loo"][fl].any()
            assert np.all(out["d2_loo"][~fl] > 0) and out["residual"].any(axis=1).all()
            if name in FLAGGED:
                assert np.flatnonzero(fl).tolist() == FLAGGED[name]
            total = 0.0
            for v in out["redundancy"]:
                total += float(v)
            assert res.redundancy_sum == total
            # rel is what the records were computed from
            again = dpgo_amd.rely_edge_debug(d, out["rel"], out["residual"], grp.graph.edges()[4], grp.graph.edges()[5], device=0)
            assert np.array_equal(again, out["records"])
        # the two methods: each within its margins of the same restatement
        s, v = outs[(a, RELY_SELINV)], outs[(a, RELY_SOLVE)]
        same = s["flag"][Q["sel"]] == v["flag"][Q["sel"]]
        assert np.all(np.abs(s["records"][Q["sel"]] - v["records"][Q["sel"]])[same] <= 2 * Q["margins"][same])
        assert np.abs(s["joint"] - v["joint"]).max() <= 2 * R["bSigma"]
        # every partition: other orderings, other fronts, the same records
        first = _first.setdefault((name, a), s)
        same = first["flag"][Q["sel"]] == s["flag"][Q["sel"]]
        assert np.all(np.abs(first["records"][Q["sel"]] - s["records"][Q["sel"]])[same] <= 2 * Q["margins"][same])
    # the two anchors: the relative pose of an edge does not know the gauge
    Q0, Q1 = restated(fixtures_dir, name, 0, grp.graph), restated(fixtures_dir, name, N - 1, grp.graph)
    for method in (RELY_SELINV, RELY_SOLVE):
        a0, a1 = outs[(0, method)], outs[(N - 1, method)]
        same = a0["flag"][Q0["sel"]] == a1["flag"][Q0["sel"]]
        assert np.all(np.abs(a0["records"][Q0["sel"]] - a1["records"][Q0["sel"]])[same] <= (Q0["margins"] + Q1["margins"])[same])


@pytest.mark.parametrize("name,nn", CASES)
def test_joint_is_the_selected_inversions_blocks_bit_for_bit(fixtures_dir, name, nn):
    """Under SELINV joint is gathered from the array NodeGroup.covariance reads on the host: the same bits, the edges at the
    anchor (zero blocks) included."""
    grp = tgc.make_group(fixtures_dir, name, nn)
    N = tp.instance(fixtures_dir, name)[0]
    for a in (0, N - 1):
        R = tgp.reference(fixtures_dir, name, a)
        I, J = grp.graph.edges()[:2]
        pairs = np.stack([I, J], axis=1).astype(np.int32)
        out = grp.edge_reliability(R["X"], anchor=a, method=RELY_SELINV)
        marg, cross, res = grp.covariance(R["X"], anchor=a, pairs=pairs)
        assert res.outcome == dpgo_amd.COV_OK and out["result"].outcome == dpgo_amd.RELY_OK
        assert np.array_equal(out["joint"][:, 1], cross)
        assert np.array_equal(out["joint"][:, 0], marg[I]) and np.array_equal(out["joint"][:, 2], marg[J])
        at = (I == a) | (J == a)
        assert at.any() and not out["joint"][at, 1].any() and not out["joint"][I == a, 0].any() and not out["joint"][J == a, 2].any()
        assert np.abs(cross).max() > 100 * R["bSigma"]   # (an orientation that is wrong would show)
        assert not np.array_equal(cross[~at], np.swapaxes(cross[~at], 1, 2))


def noise_free_graph(fixtures_dir, name, nn):
    """The device graph whose every measurement is the polished estimate's own relative pose (fp64 of the long-double one)."""
    R = tgp.reference(fixtures_dir, name, 0)
    d, X = R["d"], R["X"]
    G = tgc.make_group(fixtures_dir, name, nn).graph
    I, J, _, _, kappa, tau = G.edges()
    rel = [pr.relative(X, d, int(p), int(q), LD) for p, q in zip(I, J)]
    return dpgo_amd.graph_from_edges(d, R["N"], I, J, np.stack([np.asarray(r[0], np.float64) for r in rel]),
                                     np.stack([np.asarray(r[1], np.float64) for r in rel]), kappa, tau, nn)


@pytest.mark.parametrize("method", [RELY_SELINV, RELY_SOLVE])
def test_redundancies_of_a_noise_free_graph_sum_to_the_cycle_count(fixtures_dir, method):
    """smallGrid3D with every measurement replaced by the estimate's own relative pose: sum rho_e = dof (m - N + 1) exactly, and
    every edge agrees with the others.  The margin of one redundancy is rely_restatement's with bSigma of the original graph
    scaled by what its formula changes by -- the two anchored Hessians have the same pattern and the same weights, and differ
    in the Lambda blocks only -- i.e. by max(1, ratio of kappa_2 / lambda_min, ratio of 1 / lambda_min^2)."""
    import cert_restatement as cert
    name, nn = "smallGrid3D", 5
    R = tgp.reference(fixtures_dir, name, 0)
    d, dof, X, N = R["d"], R["dof"], R["X"], R["N"]
    G0 = noise_free_graph(fixtures_dir, name, nn)
    grp = dpgo_amd.NodeGroup(G0, range(nn), dpgo_amd.Options.driver(LOSS_NONE, True, max_iterations=0))
    out = grp.edge_reliability(X, method=method)
    res = out["result"]
    assert res.outcome == dpgo_amd.RELY_OK and res.stationarity <= 1e-10
    I, J, Rm, t, kappa, tau = G0.edges()
    m = len(I)
    ptr, col, val = grp.cov_hessian(X)
    import scipy.sparse as sp
    A0 = sp.csr_matrix((val, col, ptr)).toarray()
    lam0, lam = np.linalg.eigvalsh((A0 + A0.T) / 2), np.linalg.eigvalsh(R["A"])
    scale = max(1.0, (lam0[-1] / lam0[0] ** 2) / (lam[-1] / lam[0] ** 2), (lam[0] / lam0[0]) ** 2)
    S0 = np.linalg.inv((A0 + A0.T) / 2)
    bound = 0.0
    for e in range(m):
        p, q = int(I[e]), int(J[e])
        Sj = pr.joint_of(S0, dof, p, q, 0)
        m_rel = pr.margin_rel(X, d, p, q, Sj, scale * R["bSigma"])
        om = np.diag(pr.omega(d, kappa[e], tau[e]))
        rel = np.abs(pr.rel_cov(pr.jacobian(X, d, p, q), Sj))
        bound += np.sum(om * np.diag(m_rel)) + (dof + 2) * U * np.sum(om * np.diag(rel)) + U * dof
    print("noise-free smallGrid3D x %d, %s: sum of redundancies %.12f against %d, bound %.3g; largest d2_loo %.3g"
          % (nn, dpgo_amd.RELY_METHOD_NAMES[method], res.redundancy_sum, dof * (m - N + 1), bound, out["d2_loo"].max()))
    assert abs(res.redundancy_sum - dof * (m - N + 1)) <= bound + m * U * dof * (m - N + 1)   # (and the m additions of the sum)
    assert out["d2_loo"].max() <= 1e-20 and out["d2_own"].max() <= 1e-20


def test_a_shuffled_subset_with_repeats_has_the_bits_of_the_full_call(fixtures_dir):
    R = tgp.reference(fixtures_dir, "smallGrid3D", 0)
    grp = tgc.make_group(fixtures_dir, "smallGrid3D", 5)
    full = grp.edge_reliability(R["X"], method=RELY_SELINV)
    m = full["result"].edges
    rng = np.random.default_rng(5)
    edges = np.concatenate([rng.permutation(m)[:70], [3, 3, m - 1, 0, 3]])
    part = grp.edge_reliability(R["X"], edges=edges, method=RELY_SELINV)
    assert part["result"].edges == len(edges) and part["result"].outcome == dpgo_amd.RELY_OK
    for key in ("records", "rel", "joint"):
        assert np.array_equal(part[key], full[key][edges]), key
    total = 0.0
    for v in part["redundancy"]:
        total += float(v)
    assert part["result"].redundancy_sum == total
    none = grp.edge_reliability(R["X"], edges=[], method=RELY_SELINV)
    assert none["result"].outcome == dpgo_amd.RELY_OK and none["result"].edges == 0 and none["records"].shape[0] == 0
    # under SOLVE an edge's bits do not depend on its companions either (pairs.h)
    one = grp.edge_reliability(R["X"], edges=[17], method=RELY_SOLVE)
    many = grp.edge_reliability(R["X"], edges=edges[:40].tolist() + [17], method=RELY_SOLVE)
    assert one["result"].batches == 1 and many["result"].batches > 1 and np.array_equal(one["records"][0], many["records"][-1])


def test_auto_the_refusals_and_skipped_allocates_nothing(fixtures_dir):
    R = tgp.reference(fixtures_dir, "smallGrid3D", 0)
    grp = tgc.make_group(fixtures_dir, "smallGrid3D", 2)
    edges = [5, 200]
    grp.edge_reliability(R["X"], edges=edges, max_bytes=1)   # (the certificate's buffers and M's values come here)
    free0 = tgp.device_free_bytes()
    out = grp.edge_reliability(R["X"], edges=edges, max_bytes=1)
    assert tgp.device_free_bytes() == free0
    res = out["result"]
    assert res.outcome == dpgo_amd.RELY_SKIPPED and res.method_used == RELY_AUTO and not out["records"].any() and not out["joint"].any()
    assert res.unknowns == 6 * R["N"] and res.fronts >= 4 and res.stationarity > 0 and res.edges == 2
    assert 1 < res.device_bytes_solve < res.device_bytes_selinv and res.device_bytes == res.device_bytes_solve
    print("smallGrid3D, 2 edges: SELINV predicts %d bytes, SOLVE %d" % (res.device_bytes_selinv, res.device_bytes_solve))
    for method, field in ((RELY_SELINV, "device_bytes_selinv"), (RELY_SOLVE, "device_bytes_solve")):
        sk = grp.edge_reliability(R["X"], edges=edges, method=method, max_bytes=getattr(res, field) - 1)["result"]
        assert sk.outcome == dpgo_amd.RELY_SKIPPED and sk.method_used == method and sk.device_bytes == getattr(res, field)
        assert (sk.device_bytes_selinv, sk.device_bytes_solve) == (res.device_bytes_selinv, res.device_bytes_solve)
    assert tgp.device_free_bytes() == free0
    between = (res.device_bytes_solve + res.device_bytes_selinv) // 2
    auto = grp.edge_reliability(R["X"], edges=edges, max_bytes=between)
    assert auto["result"].outcome == dpgo_amd.RELY_OK and auto["result"].method_used == RELY_SOLVE
    assert grp.edge_reliability(R["X"], edges=edges, method=RELY_SELINV, max_bytes=between)["result"].outcome == dpgo_amd.RELY_SKIPPED
    roomy = grp.edge_reliability(R["X"], edges=edges)
    assert roomy["result"].outcome == dpgo_amd.RELY_OK and roomy["result"].method_used == RELY_SELINV
    solve = grp.edge_reliability(R["X"], edges=edges, method=RELY_SOLVE)
    assert np.array_equal(auto["records"], solve["records"])
    Q = restated(fixtures_dir, "smallGrid3D", 0, grp.graph)
    assert np.all(np.abs(np.asarray(roomy["records"], LD) - Q["vecs"][edges]) <= Q["margins"][edges])
    assert np.all(np.abs(np.asarray(auto["records"], LD) - Q["vecs"][edges]) <= Q["margins"][edges])


def test_a_point_that_is_no_minimum(fixtures_dir):
    R = tgp.reference(fixtures_dir, "smallGrid3D", 0)
    grp = tgc.make_group(fixtures_dir, "smallGrid3D", 2)
    before = grp.edge_reliability(R["X"])
    Z = cr.random_rotations_point(R["X"], R["d"], 5)
    for method in (RELY_AUTO, RELY_SELINV, RELY_SOLVE):
        bad = grp.edge_reliability(Z, method=method)
        assert bad["result"].outcome == dpgo_amd.RELY_NOT_PD and bad["result"].flagged == 0 and bad["result"].redundancy_sum == 0
        assert not bad["records"].any() and not bad["rel"].any() and not bad["joint"].any()
    after = grp.edge_reliability(R["X"])
    assert after["result"].outcome == dpgo_amd.RELY_OK
    for key in ("records", "rel", "joint"):
        assert np.array_equal(before[key], after[key])


def test_unweighted_edges_are_flag_two_and_not_uploaded(fixtures_dir):
    """scale_edges can leave kappa = tau = 0: such an edge is flag 2, all zeros, left out of the sum; the others have the
    records of the call that lists only them."""
    R = tgp.reference(fixtures_dir, "smallGrid3D", 0)
    G = dpgo_amd.read_g2o(tc.problem(fixtures_dir, "smallGrid3D")[0], 2)
    I, J, Rm, t, kappa, tau = G.edges()
    kappa, tau = kappa.copy(), tau.copy()
    dead = [7, 100]
    kappa[dead[0]] = tau[dead[0]] = 0.0
    tau[dead[1]] = 0.0
    kappa[dead[1]] = 0.0
    Gz = dpgo_amd.graph_from_edges(3, R["N"], I, J, Rm, t, kappa, tau, 2)
    grp = dpgo_amd.NodeGroup(Gz, range(2), dpgo_amd.Options.driver(LOSS_NONE, True, max_iterations=0))
    X = grp.polish(R["X"])[0]
    out = grp.edge_reliability(X, method=RELY_SELINV)
    res = out["result"]
    assert res.outcome == dpgo_amd.RELY_OK and res.unweighted == 2 and np.flatnonzero(out["flag"] == 2).tolist() == dead
    assert not out["records"][dead][:, [0, 2, 3, 4, 5]].any() and not out["records"][dead][:, 6:].any()
    assert not out["rel"][dead].any() and not out["joint"][dead].any()
    live = [e for e in range(len(I)) if e not in dead]
    only = grp.edge_reliability(X, edges=live, method=RELY_SELINV)
    assert np.array_equal(only["records"], out["records"][live]) and only["result"].redundancy_sum == res.redundancy_sum


def test_refusals(fixtures_dir):
    path, N, mm, gp, X0 = tc.problem(fixtures_dir, "smallGrid3D")
    X = tgp.reference(fixtures_dir, "smallGrid3D", 0)["X"]
    G = dpgo_amd.read_g2o(path, 2)
    hub = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(dpgo_amd.LOSS_HUBER, True), X0=X0)
    with pytest.raises(RuntimeError):
        hub.group.edge_reliability(X)                   # a robust loss
    part = dpgo_amd.NodeGroup(G, [0], dpgo_amd.Options.driver(LOSS_NONE, True))
    with pytest.raises(RuntimeError):
        part.edge_reliability(X)                        # a group that does not host every node
    grp = tgc.make_group(fixtures_dir, "smallGrid3D", 2)
    m = grp.graph.num_edges
    for bad in (dict(anchor=N), dict(anchor=-1), dict(method=3), dict(method=-1), dict(edges=[0, m]), dict(edges=[-1])):
        with pytest.raises(RuntimeError):
            grp.edge_reliability(X, **bad)
    with pytest.raises(RuntimeError):
        grp.edge_reliability(X[:-1])
    tiny = dpgo_amd.read_g2o(tc.problem(fixtures_dir, "tinyGrid3D")[0], 2)
    with pytest.raises(RuntimeError):
        grp.edge_reliability(X, graph=tiny)             # a graph that is not the group's
    # null arrays behind a valid group
    import ctypes as C
    L = dpgo_amd.lib()
    Xf = np.asfortranarray(X)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rec, res = np.zeros((m, 18)), dpgo_amd.RelyResult()
    call = lambda x, r, out, g=grp.graph._h: L.dpgo_group_edge_reliability(grp._h, g, x, Xf.shape[0], 0, 0, 0, None, 0, r, None, None, out)
    assert call(dp(Xf), dp(rec), C.byref(res)) == 0 and res.outcome == dpgo_amd.RELY_OK
    assert call(None, dp(rec), C.byref(res)) == -1 and call(dp(Xf), None, C.byref(res)) == -1 and call(dp(Xf), dp(rec), None) == -1
    assert call(dp(Xf), dp(rec), C.byref(res), None) == -1
    e = np.zeros(1, np.int32)
    assert L.dpgo_group_edge_reliability(grp._h, grp.graph._h, dp(Xf), Xf.shape[0], 0, 0, 0, e.ctypes.data_as(C.POINTER(C.c_int)), -1,
                                         dp(rec), None, None, C.byref(res)) == -1
    assert grp.edge_reliability(X)["result"].outcome == dpgo_amd.RELY_OK


def test_edge_reliability_does_not_disturb_the_optimiser(fixtures_dir):
    """30 AMM-PGO# iterations with a call on a sibling trivial-loss group after every fifth: bit for bit the run without."""
    path = tc.problem(fixtures_dir, "smallGrid3D")[0]
    runs = []
    for with_call in (False, True):
        drv = dpgo_amd.DistPGO(dpgo_amd.read_g2o(path, 2), dpgo_amd.Options.driver(LOSS_NONE, True))
        sib = tc.group(path, 2)[0] if with_call else None
        trace = []
        for it in range(30):
            assert drv.step() == 0
            if with_call and it % 5 == 4:
                method = (RELY_SELINV, RELY_SOLVE)[(it // 5) % 2]
                assert sib.edge_reliability(drv.X(), method=method)["result"].outcome in (dpgo_amd.RELY_OK, dpgo_amd.RELY_NOT_PD)
            trace.append([getattr(drv.group.results(a), f) for a in range(2) for f in ("fobj", "gamma", "gradFnorm", "Gk")])
        runs.append((np.array(drv.X()), [drv.group[a].Xk() for a in range(2)], np.array(trace)))
    assert np.array_equal(runs[0][0], runs[1][0])
    for a in range(2):
        assert np.array_equal(runs[0][1][a], runs[1][1][a])
    assert np.array_equal(runs[0][2], runs[1][2])


def test_reweighted_with_unit_weights_is_the_group_call(fixtures_dir):
    path = tc.problem(fixtures_dir, "smallGrid3D")[0]
    R = tgp.reference(fixtures_dir, "smallGrid3D", 0)
    G = dpgo_amd.read_g2o(path, 2)
    edges = [4, 250, 4, 33]
    for method in (RELY_SELINV, RELY_SOLVE):
        got = dpgo_amd.edge_reliability_reweighted(G, R["X"], LOSS_NONE, edges=edges, method=method)
        want = tgc.make_group(fixtures_dir, "smallGrid3D", 2).edge_reliability(R["X"], edges=edges, method=method)
        assert got["result"].outcome == dpgo_amd.RELY_OK and got["summary"].num_downweighted == 0
        for key in ("records", "rel", "joint"):
            assert np.array_equal(got[key], want[key])
    # a robust loss: the weights of the MM surrogate at X scale the edges
    hub = dpgo_amd.edge_reliability_reweighted(G, R["X"], dpgo_amd.LOSS_HUBER, loss_reg=0.25)
    assert hub["result"].outcome in (dpgo_amd.RELY_OK, dpgo_amd.RELY_NOT_PD) and hub["summary"].num_inter > 0


# ---------------------------------------------------------------------------------------------------------------
# the drivers
# ---------------------------------------------------------------------------------------------------------------
_py = {}


def python_run(fixtures_dir):
    """What the drivers do on tinyGrid3D x 2: 30 iterations, the polish, the records of every edge."""
    if not _py:
        drv = dpgo_amd.DistPGO(dpgo_amd.read_g2o(os.path.join(fixtures_dir, "tinyGrid3D.g2o"), 2), dpgo_amd.Options.driver(LOSS_NONE, True))
        for _ in range(30):
            assert drv.step() == 0
        Xp, pres, _ = drv.group.polish(drv.X())
        assert pres.outcome == dpgo_amd.POLISH_CONVERGED
        out = drv.group.edge_reliability(Xp)
        assert out["result"].outcome == dpgo_amd.RELY_OK
        _py["v"] = (out, drv.graph.edges()[0], drv.graph.edges()[1])
    return _py["v"]


def test_dist_pgo_edge_reliability_flag(fixtures_dir, tmp_path):
    """--polish --edge_reliability FILE adds the report and one line after the summary; the report holds
    NodeGroup.edge_reliability's numbers bit for bit."""
    exe = os.path.join(tc.ROOT, "dpgo_amd", "dist_pgo")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    path = os.path.join(fixtures_dir, "tinyGrid3D.g2o")
    base = [exe, "--dataset", path, "--num_nodes", "2", "--iters", "30", "--dist_init", "false", "--save", "false"]
    run = subprocess.run(base + ["--polish", "--edge_reliability", "rely.txt"], capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = [l for l in run.stdout.splitlines() if l.startswith("reliability: ")]
    assert len(lines) == 1 and run.stdout.rstrip().splitlines()[-1] == lines[0]
    out, I, J = python_run(fixtures_dir)
    res = out["result"]
    f = lines[0].split()
    assert f[1:3] == ["OK", dpgo_amd.RELY_METHOD_NAMES[res.method_used]]
    assert [int(v) for v in f[3:6]] == [res.edges, res.flagged, res.unweighted] and float(f[6]) == res.redundancy_sum
    assert int(f[7]) == res.device_bytes
    rows = np.loadtxt(tmp_path / "rely.txt")
    m = res.edges
    assert rows.shape == (m, 9) and np.array_equal(rows[:, 0], np.arange(m)) and np.array_equal(rows[:, 1], I) and np.array_equal(rows[:, 2], J)
    assert np.array_equal(rows[:, 3:], out["records"][:, [2, 3, 4, 0, 1, 5]])
    # without --polish, or with a robust loss: the line says why
    raw = subprocess.run(base + ["--edge_reliability", "r2.txt"], capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert raw.returncode == 0 and "reliability: not computed" in raw.stdout and not (tmp_path / "r2.txt").exists()
    hub = subprocess.run(base + ["--loss", "huber", "--polish", "--edge_reliability", "r3.txt"], capture_output=True, text=True, cwd=tmp_path,
                         timeout=300)
    assert hub.returncode == 0 and "reliability: not computed" in hub.stdout and not (tmp_path / "r3.txt").exists()


def test_cpp_facade_edge_reliability(fixtures_dir):
    """examples/facade_mm.cpp with `reliability`: DPGOHashGroup::newton_polish and ::edge_reliability after the loop, on stderr;
    stdout the same trace as without; the records those of NodeGroup.edge_reliability bit for bit; an edge index outside the
    graph refused."""
    exe = os.path.join(tc.ROOT, "dpgo_amd", "facade_mm")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    args = [exe, os.path.join(fixtures_dir, "tinyGrid3D.g2o"), "2", "30", "trivial", "1"]
    plain = subprocess.run(args, check=True, capture_output=True, text=True, timeout=300)
    out = subprocess.run(args + ["reliability"], check=True, capture_output=True, text=True, timeout=300)
    assert out.stdout == plain.stdout and "reliability" not in plain.stderr
    lines = [l.split() for l in out.stderr.splitlines() if l.startswith("reliability: ")]
    want, _, _ = python_run(fixtures_dir)
    res = want["result"]
    m = res.edges
    assert len(lines) == m + 2
    assert lines[-2][1:6] == ["OK", dpgo_amd.RELY_METHOD_NAMES[res.method_used], str(m), str(res.flagged), str(res.unweighted)]
    assert float(lines[-2][6]) == res.redundancy_sum
    assert [int(l[2]) for l in lines[:m]] == list(range(m))
    got = np.array([[float(v) for v in l[3:]] for l in lines[:m]])
    assert np.array_equal(got, want["records"])
    assert lines[-1][1:] == ["bad", "edge", "-1"]
