"""Edge reliability on the full information matrices on the device (dpgo_amd/csrc/ml_rely.h): NodeGroup.ml_edge_reliability on
tinyGrid3D x 1 node, smallGrid3D x 2 and the d = 2 grid x 3 with their seeded Omega_e (tests/ml_inputs.py) at the
maximum-likelihood refinement's final point (tests/test_gpu_ml_covariance.py's references, imported, not edited), anchor 0,
under RELY_SELINV and RELY_SOLVE.

What is held, link by link, each against the long-double restatement with a bound of its own -- nothing in a bound comes from
the device:
  * joint against the dense long-double inverse of the restated H within bSigma, and bit for bit ml_covariance's blocks;
  * the residuals bit for bit ml_eval's (held to the restatement in tests/test_gpu_ml_ops.py);
  * rel and every record entry against tests/ml_rely_restatement.py evaluated on those very fp64 arrays (the device's J, joint, r
    and the graph's Omega) within tests/test_ml_rely_host.py's constants, and rel bit for bit the host twin's;
  * the sum of the redundancies against dof (m - N + 1) within the edges' bounds plus what the rounding of the factorisation
    moves the sum by (ml_rely_restatement.sum_margin_sigma).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_restatement as cr  # noqa: E402
import ml_inputs as mi  # noqa: E402
import ml_rely_restatement as mrr  # noqa: E402
import ml_restatement as mr  # noqa: E402
import pairs_restatement as pr  # noqa: E402
import rely_restatement as rr  # noqa: E402
import test_gpu_ml_covariance as tgc  # noqa: E402  (its references; none of its tests is imported)
import test_gpu_ml_ops as ops  # noqa: E402  (its groups; none of its tests is imported)
import test_gpu_polish as tgp  # noqa: E402  (device_free_bytes; none of its tests is imported)
import test_ml_host as tmh  # noqa: E402
import test_ml_rely_host as tmr  # noqa: E402  (its comparison and constants; none of its tests is imported)

import dpgo_amd  # noqa: E402
from dpgo_amd import RELY_AUTO, RELY_SELINV, RELY_SOLVE  # noqa: E402
from oracle.problem import LOSS_NONE  # noqa: E402

pytestmark = pytest.mark.gpu
LD, U = mrr.LD, mrr.U
CASES = [("tinyGrid3D", 1), ("smallGrid3D", 2), ("grid2", 3)]
_sum = {}


def sum_bound_sigma(R):
    """What the rounding of the factorisation moves the sum of all redundancies by (anchor 0), once per reference."""
    key = id(R)
    if key not in _sum:
        H = np.asarray(mr.assemble(R["E"], R["X"], 0, LD)[2], np.float64)
        _sum[key] = mrr.sum_margin_sigma(R["Sigma"], np.sqrt(np.diag(H)), 0, R["dof"])
    return _sum[key]


def dense_joint(R, anchor=0):
    E, dof = R["E"], R["dof"]
    return np.stack([pr.blocks_of(pr.joint_of(R["Sigma"], dof, int(p), int(q), anchor), dof) for p, q in zip(E["I"], E["J"])])


def check_records(R, grp, out, edges=None):
    """rel and the records of a call against the restatement on the device's own J, joint and r: (worst ratio of rel, of the
    records, the per-edge bounds of the records, the flags left to rounding)."""
    E, d = R["E"], R["E"]["d"]
    full = grp.ml_eval(R["X"], full=True)
    r_dev, more = full[1], full[4]
    idx = np.arange(len(E["I"])) if edges is None else np.asarray(edges)
    J = np.stack([more["Ji"][idx], more["Jj"][idx]], axis=1)
    assert np.array_equal(out["residual"], r_dev[idx])   # bit for bit the edge pass's
    host_rel, host_rec = dpgo_amd.ml_rely_edge_debug(d, J, out["joint"], E["Om"][idx], r_dev[idx])
    assert np.array_equal(out["rel"], host_rel) and np.array_equal(out["rel"], np.transpose(out["rel"], (0, 2, 1)))
    worst_rel = worst = 0.0
    bounds, undecided = [], 0
    for k, e in enumerate(idx):
        wr, w, ref, dec, same = tmr.compare(d, -1, out["rel"][k], out["records"][k], J[k], out["joint"][k], E["Om"][e], r_dev[e])
        worst_rel, worst = max(worst_rel, wr), max(worst, w)
        assert same or not dec, (e, out["records"][k][1], ref["flag"], ref["pivots"])
        undecided += not dec
        assert host_rec[k][1] == out["records"][k][1] or not dec
        bounds.append(mrr.bound(ref, d, tmr.CONSTANTS, tmr.CONSTANTS["rel"] *
                                mrr.rel_margin(J[k][0], J[k][1], mrr.joint_matrix(out["joint"][k])))[0])
    return worst_rel, worst, np.stack(bounds) if bounds else np.zeros((0, mrr.width(d))), undecided, J


@pytest.mark.parametrize("name,nn", CASES)
def test_records_rel_and_joint_against_the_restatement(fixtures_dir, name, nn):
    R = tgc.reference(fixtures_dir, name, 0)
    E, X, N, dof, d = R["E"], R["X"], R["N"], R["dof"], R["E"]["d"]
    m = len(E["I"])
    grp = ops.group_of(E, nn)
    pairs = np.stack([E["I"], E["J"]], axis=1).astype(np.int32)
    marg, cross, cres = grp.ml_covariance(X, pairs=pairs)
    assert cres.outcome == dpgo_amd.COV_OK
    want_joint = dense_joint(R)
    outs, bnds, Js = {}, {}, {}
    for method in (RELY_SELINV, RELY_SOLVE):
        out = outs[method] = grp.ml_edge_reliability(X, method=method)
        res = out["result"]
        assert res.outcome == dpgo_amd.RELY_OK and res.method_used == method and res.edges == m and res.unweighted == 0
        assert res.unknowns == dof * N and res.fronts >= 1 and res.pivot_min > 0 and res.stationarity == cres.stationarity
        assert res.device_bytes == (res.device_bytes_selinv if method == RELY_SELINV else res.device_bytes_solve) > 0
        assert out["records"].shape == (m, 6 + 2 * dof) and np.all(np.isin(out["flag"], (0, 1)))
        jw = float(np.abs(np.asarray(out["joint"], LD) - want_joint).max()) / R["bSigma"]
        worst_rel, worst, bnds[method], undecided, Js[method] = check_records(R, grp, out)
        fl = out["flag"] == 1
        assert res.flagged == int(fl.sum())
        assert not out["d2_loo"][fl].any() and not out["influence"][fl].any() and not out["r_loo"][fl].any()
        assert np.all(out["d2_loo"][~fl] > 0) and np.all(out["d2_own"] > 0)
        total = 0.0
        for v in out["redundancy"]:
            total += float(v)
        assert res.redundancy_sum == total
        # the identity of the Gauss-Newton Hessian: the edges' own bounds, the factorisation's part, the m additions
        want = dof * (m - N + 1)
        sb = float(bnds[method][:, 2].sum()) + sum_bound_sigma(R) + m * U * float(np.abs(out["redundancy"]).sum())
        print("%s x %d, %s: joint %.3g of bSigma, rel %.3g and records %.3g of their bounds, %d flagged, %d flags left to rounding; sum "
              "of redundancies %.12f against %d, apart %.3g, bound %.3g" % (name, nn, dpgo_amd.RELY_METHOD_NAMES[method], jw, worst_rel,
                                                                             worst, res.flagged, undecided, total, want, abs(total - want), sb))
        assert jw < 1.0 and worst_rel <= 1.0 and worst <= 1.0
        assert abs(total - want) <= sb
        # again: the same bits
        again = grp.ml_edge_reliability(X, method=method)
        for key in ("records", "rel", "joint"):
            assert np.array_equal(again[key], out[key])
    # under SELINV joint is bit for bit the selected inversion's blocks as ml_covariance hands them out
    s, v = outs[RELY_SELINV], outs[RELY_SOLVE]
    I, J = E["I"], E["J"]
    assert np.array_equal(s["joint"][:, 1], cross) and np.array_equal(s["joint"][:, 0], marg[I]) and np.array_equal(s["joint"][:, 2], marg[J])
    at = (I == 0) | (J == 0)
    assert at.any() and not s["joint"][at, 1].any() and not s["joint"][I == 0, 0].any() and not s["joint"][J == 0, 2].any()
    assert not v["joint"][at, 1].any() and not v["joint"][I == 0, 0].any() and not v["joint"][J == 0, 2].any()
    # the two methods: joint within the sum of its bounds; the records within the sum of theirs, with what the difference of
    # the two joints moves rel by (first order, entrywise) counted in
    assert np.abs(s["joint"] - v["joint"]).max() <= 2 * R["bSigma"]
    for e in range(m):
        if s["flag"][e] != v["flag"][e]:
            continue
        Ja = np.abs(np.concatenate([Js[RELY_SELINV][e][0], Js[RELY_SELINV][e][1]], axis=1))
        dS = np.abs(np.asarray(mrr.joint_matrix(s["joint"][e]) - mrr.joint_matrix(v["joint"][e]), np.float64))
        ref = mrr.record(s["rel"][e], E["Om"][e], s["residual"][e], d)
        moved = mrr.margins(ref, d, m_rel=Ja @ dS @ Ja.T)[0] - mrr.margins(ref, d)[0]
        assert np.all(np.abs(s["records"][e] - v["records"][e]) <= bnds[RELY_SELINV][e] + bnds[RELY_SOLVE][e] + moved), e


def test_a_shuffled_subset_with_repeats_has_the_bits_of_the_full_call(fixtures_dir):
    R = tgc.reference(fixtures_dir, "smallGrid3D", 0)
    grp = ops.group_of(R["E"], 2)
    full = grp.ml_edge_reliability(R["X"], method=RELY_SELINV)
    m = full["result"].edges
    rng = np.random.default_rng(5)
    edges = np.concatenate([rng.permutation(m)[:70], [3, 3, m - 1, 0, 3]])
    part = grp.ml_edge_reliability(R["X"], edges=edges, method=RELY_SELINV)
    assert part["result"].edges == len(edges) and part["result"].outcome == dpgo_amd.RELY_OK
    for key in ("records", "rel", "joint"):
        assert np.array_equal(part[key], full[key][edges]), key
    total = 0.0
    for v in part["redundancy"]:
        total += float(v)
    assert part["result"].redundancy_sum == total
    none = grp.ml_edge_reliability(R["X"], edges=[], method=RELY_SELINV)
    assert none["result"].outcome == dpgo_amd.RELY_OK and none["result"].edges == 0 and none["records"].shape[0] == 0
    # under SOLVE an edge's bits do not depend on its companions either (pairs.h)
    one = grp.ml_edge_reliability(R["X"], edges=[17], method=RELY_SOLVE)
    many = grp.ml_edge_reliability(R["X"], edges=edges[:40].tolist() + [17], method=RELY_SOLVE)
    assert one["result"].batches == 1 and many["result"].batches > 1 and np.array_equal(one["records"][0], many["records"][-1])
    assert check_records(R, grp, many, edges[:40].tolist() + [17])[1] <= 1.0


def test_auto_and_skipped_allocates_nothing(fixtures_dir):
    R = tgc.reference(fixtures_dir, "smallGrid3D", 0)
    grp = ops.group_of(R["E"], 2)
    X, edges = R["X"], [5, 200]
    grp.ml_edge_reliability(X, edges=edges, max_bytes=1)   # (the certificate's buffers come here)
    free0 = tgp.device_free_bytes()
    out = grp.ml_edge_reliability(X, edges=edges, max_bytes=1)
    assert tgp.device_free_bytes() == free0
    res = out["result"]
    assert res.outcome == dpgo_amd.RELY_SKIPPED and res.method_used == RELY_AUTO and not out["records"].any() and not out["joint"].any()
    assert res.unknowns == 6 * R["N"] and res.fronts >= 4 and res.stationarity == 0 and res.edges == 2
    assert 1 < res.device_bytes_solve < res.device_bytes_selinv and res.device_bytes == res.device_bytes_solve
    print("smallGrid3D, 2 edges: SELINV predicts %d bytes, SOLVE %d" % (res.device_bytes_selinv, res.device_bytes_solve))
    for method, field in ((RELY_SELINV, "device_bytes_selinv"), (RELY_SOLVE, "device_bytes_solve")):
        sk = grp.ml_edge_reliability(X, edges=edges, method=method, max_bytes=getattr(res, field) - 1)["result"]
        assert sk.outcome == dpgo_amd.RELY_SKIPPED and sk.method_used == method and sk.device_bytes == getattr(res, field)
        assert (sk.device_bytes_selinv, sk.device_bytes_solve) == (res.device_bytes_selinv, res.device_bytes_solve)
    assert tgp.device_free_bytes() == free0
    between = (res.device_bytes_solve + res.device_bytes_selinv) // 2
    auto = grp.ml_edge_reliability(X, edges=edges, max_bytes=between)
    assert auto["result"].outcome == dpgo_amd.RELY_OK and auto["result"].method_used == RELY_SOLVE
    assert grp.ml_edge_reliability(X, edges=edges, method=RELY_SELINV, max_bytes=between)["result"].outcome == dpgo_amd.RELY_SKIPPED
    roomy = grp.ml_edge_reliability(X, edges=edges)
    assert roomy["result"].outcome == dpgo_amd.RELY_OK and roomy["result"].method_used == RELY_SELINV
    solve = grp.ml_edge_reliability(X, edges=edges, method=RELY_SOLVE)
    assert np.array_equal(auto["records"], solve["records"])
    assert check_records(R, grp, roomy, edges)[1] <= 1.0 and check_records(R, grp, auto, edges)[1] <= 1.0


def cut_graph(E, pose, nn):
    """E's graph without the edges of one pose: every edge still a block of the group's pattern, H of rank dof (N - 1) - dof."""
    keep = (E["I"] != pose) & (E["J"] != pose)
    assert 0 < keep.sum() < len(keep)
    return tmh.graph_of(dict(E, **{k: E[k][keep] for k in ("I", "J", "R", "t", "kappa", "tau", "Om")}), nn)


def test_a_rank_deficient_graph_is_not_pd(fixtures_dir):
    R = tgc.reference(fixtures_dir, "smallGrid3D", 0)
    E, X = R["E"], R["X"]
    grp = ops.group_of(E, 2)
    before = grp.ml_edge_reliability(X)
    cut = cut_graph(E, 7, 2)
    for method in (RELY_AUTO, RELY_SELINV, RELY_SOLVE):
        bad = grp.ml_edge_reliability(X, method=method, graph=cut)
        assert bad["result"].outcome == dpgo_amd.RELY_NOT_PD and bad["result"].flagged == 0 and bad["result"].redundancy_sum == 0
        assert not bad["records"].any() and not bad["rel"].any() and not bad["joint"].any()
    after = grp.ml_edge_reliability(X)
    assert after["result"].outcome == dpgo_amd.RELY_OK
    for key in ("records", "rel", "joint"):
        assert np.array_equal(before[key], after[key])


def test_refusals(fixtures_dir):
    R = tgc.reference(fixtures_dir, "smallGrid3D", 0)
    E, X, N = R["E"], R["X"], R["N"]
    G = tmh.graph_of(E, 2)
    hub = dpgo_amd.NodeGroup(G, range(2), dpgo_amd.Options.driver(dpgo_amd.LOSS_HUBER, True, max_iterations=0))
    part = dpgo_amd.NodeGroup(G, [0], dpgo_amd.Options.driver(LOSS_NONE, True, max_iterations=0))
    grp = ops.group_of(E, 2)
    m = grp.graph.num_edges
    other = tmh.graph_of(mi.fixture(fixtures_dir, "tinyGrid3D"), 2)
    bad = E["Om"].copy()
    bad[11, 2, 2] = -1.0
    notspd = tmh.graph_of(dict(E, Om=bad), 2)
    for g, kw in ((hub, {}), (part, {}), (grp, dict(graph=other)), (grp, dict(graph=notspd)), (grp, dict(anchor=N)), (grp, dict(anchor=-1)),
                  (grp, dict(method=3)), (grp, dict(method=-1)), (grp, dict(edges=[0, m])), (grp, dict(edges=[-1]))):
        with pytest.raises(RuntimeError):
            g.ml_edge_reliability(X, **kw)
    with pytest.raises(RuntimeError):
        grp.ml_edge_reliability(X[:-1])
    # null arrays behind a valid group
    L = dpgo_amd.lib()
    Xf = np.asfortranarray(X)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    rec, res = np.zeros((m, 18)), dpgo_amd.RelyResult()
    call = lambda x, r, out, g=grp.graph._h: L.dpgo_group_ml_edge_reliability(grp._h, g, x, Xf.shape[0], 0, 0, 0, None, 0, r, None,  # noqa: E731
                                                                              None, out)
    assert call(dp(Xf), dp(rec), C.byref(res)) == 0 and res.outcome == dpgo_amd.RELY_OK
    assert call(None, dp(rec), C.byref(res)) == -1 and call(dp(Xf), None, C.byref(res)) == -1 and call(dp(Xf), dp(rec), None) == -1
    assert call(dp(Xf), dp(rec), C.byref(res), None) == -1
    e = np.zeros(1, np.int32)
    assert L.dpgo_group_ml_edge_reliability(grp._h, grp.graph._h, dp(Xf), Xf.shape[0], 0, 0, 0, e.ctypes.data_as(C.POINTER(C.c_int)), -1,
                                            dp(rec), None, None, C.byref(res)) == -1
    assert grp.ml_edge_reliability(X)["result"].outcome == dpgo_amd.RELY_OK


def test_ml_edge_reliability_does_not_disturb_the_optimiser(fixtures_dir):
    """30 AMM-PGO# iterations with a call on a sibling trivial-loss group after every fifth: bit for bit the run without."""
    path = os.path.join(fixtures_dir, "smallGrid3D.g2o")
    E = mi.fixture(fixtures_dir, "smallGrid3D")
    runs = []
    for with_call in (False, True):
        drv = dpgo_amd.DistPGO(dpgo_amd.read_g2o(path, 2), dpgo_amd.Options.driver(LOSS_NONE, True))
        sib = ops.group_of(E, 2) if with_call else None
        trace = []
        for it in range(30):
            assert drv.step() == 0
            if with_call and it % 5 == 4:
                method = (RELY_SELINV, RELY_SOLVE)[(it // 5) % 2]
                assert sib.ml_edge_reliability(drv.X(), method=method)["result"].outcome in (dpgo_amd.RELY_OK, dpgo_amd.RELY_NOT_PD)
            trace.append([getattr(drv.group.results(a), f) for a in range(2) for f in ("fobj", "gamma", "gradFnorm", "Gk")])
        runs.append((np.array(drv.X()), [drv.group[a].Xk() for a in range(2)], np.array(trace)))
    assert np.array_equal(runs[0][0], runs[1][0])
    for a in range(2):
        assert np.array_equal(runs[0][1][a], runs[1][1][a])
    assert np.array_equal(runs[0][2], runs[1][2])


@pytest.mark.parametrize("d", [2, 3])
def test_isotropic_redundancies_on_a_noise_free_graph_are_edge_reliabilitys(d):
    """A graph without Omega whose every residual is exactly zero: Omega_iso, the Gauss-Newton Hessian is the Riemannian one and
    J differs from the chordal relative-pose Jacobian by rotations inside the translation and the rotation block, which
    tr(Omega_iso rel) does not see -- redundancy and redundancy_trans equal edge_reliability's within the sum of both bounds.
    ML: ml_rely_restatement's with m_rel from bS (entrywise, both Hessians' rounding in it: test_gpu_ml_ops'
    isotropic-consistency bound) and the bound of J; chordal: rely_restatement's margins with pairs_restatement's m_rel for the
    same bS."""
    E, X = mi.noise_free(d)
    N, dof, m = E["N"], cr.dof_of(d), len(E["I"])
    grp = ops.group_of(E, 2, info=False)
    ref = mr.edges_all(E, X, LD)
    eb = mr.edge_bounds(E, X, ref)
    absH = mr.assemble(dict(E), X, None, np.float64, per_edge={k: (np.abs(np.asarray(v, np.float64)) if k != "near_pi" else v)
                                                              for k, v in ref.items()})[2]
    bH = tmh.CONSTANTS["H"] * mr.sum_bounds(E, N, ref, eb)[2] + 2 * (4 * d + 2) * U * absH
    H = np.asarray(mr.assemble(E, X, 0, LD, per_edge=ref)[2], np.float64)
    lam = np.linalg.eigvalsh(0.5 * (H + H.T))
    bS = cr.C * U * float(lam[-1] / lam[0]) / float(lam[0]) + float(np.linalg.norm(bH, 2)) / float(lam[0]) ** 2
    Sigma = mrr.inverse(H)
    for method in (RELY_SELINV, RELY_SOLVE):
        ml = grp.ml_edge_reliability(X, method=method)
        ch = grp.edge_reliability(X, method=method)
        assert ml["result"].outcome == dpgo_amd.RELY_OK and ch["result"].outcome == dpgo_amd.RELY_OK
        worst = 0.0
        for e in range(m):
            p, q = int(E["I"][e]), int(E["J"][e])
            Sj = pr.joint_of(np.asarray(Sigma), dof, p, q, 0)
            Ja = np.abs(np.concatenate([np.asarray(ref["Ji"][e], np.float64), np.asarray(ref["Jj"][e], np.float64)], axis=1))
            bJ = np.concatenate([tmh.CONSTANTS["Ji"] * eb["Ji"][e], tmh.CONSTANTS["Jj"] * eb["Jj"][e]], axis=1)
            Sa = np.abs(np.asarray(Sj, np.float64))
            m_rel = (Ja @ np.full((2 * dof, 2 * dof), bS) @ Ja.T + bJ @ Sa @ Ja.T + Ja @ Sa @ bJ.T +
                     tmr.CONSTANTS["rel"] * mrr.rel_margin(ref["Ji"][e], ref["Jj"][e], Sj))
            rec = mrr.record(mrr.rel_of(ref["Ji"][e], ref["Jj"][e], Sj), E["Om"][e], ref["r"][e], d)
            b_ml = mrr.bound(rec, d, tmr.CONSTANTS, m_rel, tmh.CONSTANTS["r"] * eb["r"][e])[0]
            cand = (E["R"][e], E["t"][e], float(E["kappa"][e]), float(E["tau"][e]))
            rel_c, r_c = rr.rel_and_r(X, d, p, q, cand, Sj, LD)
            rec_c = rr.record(rel_c, r_c, d, cand[2], cand[3])
            b_ch = rr.margins(rec_c, rel_c, d, cand[2], cand[3], pr.margin_rel(X, d, p, q, np.asarray(Sj, np.float64), bS),
                              pr.margin_residual(X, d, p, q, cand))
            for f in (2, 3):
                worst = max(worst, abs(ml["records"][e][f] - ch["records"][e][f]) / (b_ml[f] + b_ch[f]))
        print("d = %d, %s: redundancies against edge_reliability's at %.3g of the sum of both bounds; sums %.12f and %.12f against %d"
              % (d, dpgo_amd.RELY_METHOD_NAMES[method], worst, ml["result"].redundancy_sum, ch["result"].redundancy_sum,
                 dof * (m - N + 1)))
        assert worst <= 1.0
        assert not ml["d2_own"].any() and not ml["residual"].any()
