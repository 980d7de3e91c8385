"""The candidate gate on the full information matrices on the device (dpgo_amd/csrc/ml_rely.h): NodeGroup.ml_pair_gate on
tinyGrid3D x 1 node, smallGrid3D x 2 and the d = 2 grid x 3 with their seeded Omega_e at the maximum-likelihood refinement's final
point (tests/test_gpu_ml_covariance.py's references), anchor 0; and the C++ facade and the driver's two flags against the Python
calls.

The candidates of a case: copies of graph edges (measurement and Omega), pairs that are no edge with the estimate's own relative
pose perturbed and a seeded anisotropic Omega (tests/ml_inputs.py: information), a pair p == p, pairs with the anchor on either
side and the anchor with itself.  What is held, link by link, each with a bound of its own and nothing of it from the device:
joint against the dense long-double inverse within bSigma; the residual against the long-double restatement within
tests/test_ml_host.py's constant; rel, d2 and not_pd against tests/ml_rely_restatement.py on the restated J and r (their bounds
carried as the inputs' margins) and the device's joint, within tests/test_ml_rely_host.py's constants.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_restatement as cr  # noqa: E402
import ml_inputs as mi  # noqa: E402
import ml_rely_restatement as mrr  # noqa: E402
import ml_restatement as mr  # noqa: E402
import pairs_restatement as pr  # noqa: E402
import test_gpu_ml_covariance as tgc  # noqa: E402  (its references; none of its tests is imported)
import test_gpu_ml_ops as ops  # noqa: E402  (its groups; none of its tests is imported)
import test_gpu_ml_reliability as tgr  # noqa: E402  (cut_graph; none of its tests is imported)
import test_gpu_polish as tgp  # noqa: E402  (device_free_bytes, ROOT; none of its tests is imported)
import test_ml_host as tmh  # noqa: E402
import test_ml_rely_host as tmr  # noqa: E402  (its constants; none of its tests is imported)

import dpgo_amd  # noqa: E402
from oracle.problem import LOSS_NONE  # noqa: E402

pytestmark = pytest.mark.gpu
LD, U = mrr.LD, mrr.U
CASES = [("tinyGrid3D", 1), ("smallGrid3D", 2), ("grid2", 3)]
_cand = {}


def candidates(R, name):
    """dict(d, I, J, R, t, Om, copies): the candidates of a case as an edge dict of tests/ml_restatement.py; copies[k]: the
    graph edge candidate k copies, -1: none."""
    if name not in _cand:
        E, X = R["E"], R["X"]
        d, N, m = E["d"], R["N"], len(E["I"])
        rng = np.random.default_rng(mi.SEED + 31 + N)
        P = mr.poses_of(np.asarray(X, np.float64), d)
        copies = [0, m // 2, m - 1, 1, m // 3]   # (m // 2: the edge whose Omega is scaled by 1e4)
        is_edge = {(int(a), int(b)) for a, b in zip(E["I"], E["J"])} | {(int(b), int(a)) for a, b in zip(E["I"], E["J"])}
        far = []
        while len(far) < 4:
            p, q = (int(v) for v in rng.integers(1, N, 2))
            if p != q and (p, q) not in is_edge:
                far.append((p, q))
        other = far + [(N // 2, N // 2), (0, N - 1), (N - 2, 0), (0, 0)]
        I = [int(E["I"][e]) for e in copies] + [p for p, _ in other]
        J = [int(E["J"][e]) for e in copies] + [q for _, q in other]
        Rm, t = [E["R"][e] for e in copies], [E["t"][e] for e in copies]
        dr = cr.dof_of(d) - d
        for p, q in other:
            Rm.append(P[p][1] @ P[q][1].T @ mi.rotation(0.05 * rng.standard_normal(dr), d))
            t.append(P[p][1] @ (P[q][0] - P[p][0]) + 0.05 * rng.standard_normal(d))
        Om_new = mi.information(d, rng.uniform(5, 50, len(other)), rng.uniform(5, 50, len(other)), mi.SEED + 32 + N)
        Om = np.concatenate([E["Om"][copies], Om_new])
        _cand[name] = dict(d=d, I=np.array(I, np.int32), J=np.array(J, np.int32), R=np.array(Rm), t=np.array(t), Om=Om,
                           copies=np.array(copies + [-1] * len(other)))
    return _cand[name]


def check_gate(R, Cd, out, anchor=0):
    """joint, the residual, rel, d2 and not_pd of a call against the restatement: (joint / bSigma, the worst ratio of the
    residual, of rel, of d2)."""
    d, dof, X = Cd["d"], R["dof"], R["X"]
    n = len(Cd["I"])
    ref = mr.edges_all(Cd, X, LD)
    eb = mr.edge_bounds(Cd, X, ref)
    want_joint = np.stack([pr.blocks_of(pr.joint_of(R["Sigma"], dof, int(p), int(q), anchor), dof) for p, q in zip(Cd["I"], Cd["J"])])
    jw = float(np.abs(np.asarray(out["joint"], LD) - want_joint).max()) / R["bSigma"]
    w_r = w_rel = w_d2 = 0.0
    for k in range(n):
        m_r = tmh.CONSTANTS["r"] * eb["r"][k]
        err = np.abs(np.asarray(out["residual"][k], LD) - ref["r"][k]).astype(np.float64)
        assert np.all(err[m_r == 0] == 0)
        w_r = max(w_r, float((err[m_r > 0] / m_r[m_r > 0]).max()) if np.any(m_r > 0) else 0.0)
        Sj = mrr.joint_matrix(out["joint"][k])
        Ja = np.abs(np.concatenate([np.asarray(ref["Ji"][k], np.float64), np.asarray(ref["Jj"][k], np.float64)], axis=1))
        bJ = np.concatenate([tmh.CONSTANTS["Ji"] * eb["Ji"][k], tmh.CONSTANTS["Jj"] * eb["Jj"][k]], axis=1)
        Sa = np.abs(np.asarray(Sj, np.float64))
        m_rel = mrr.mirrored(bJ @ Sa @ Ja.T + Ja @ Sa @ bJ.T + tmr.CONSTANTS["rel"] * mrr.rel_margin(ref["Ji"][k], ref["Jj"][k], Sj))
        rel = mrr.mirrored(mrr.rel_of(ref["Ji"][k], ref["Jj"][k], Sj))   # (the lower triangle, written to both places)
        err = np.abs(np.asarray(out["rel"][k], LD) - rel).astype(np.float64)
        assert np.all(err[m_rel == 0] == 0) and np.array_equal(out["rel"][k], out["rel"][k].T)
        w_rel = max(w_rel, float((err[m_rel > 0] / m_rel[m_rel > 0]).max()) if np.any(m_rel > 0) else 0.0)
        rec = mrr.record(rel, Cd["Om"][k], ref["r"][k], d, 1)
        b = mrr.bound(rec, d, tmr.CONSTANTS, m_rel, m_r)[0]
        assert rec["flag"] == 0 and not out["not_pd"][k]     # I + A is positive definite
        w_d2 = max(w_d2, abs(float(LD(out["d2"][k]) - rec["d2"])) / b[0])
    return jw, w_r, w_rel, w_d2


@pytest.mark.parametrize("name,nn", CASES)
def test_gate_against_the_restatement(fixtures_dir, name, nn):
    R = tgc.reference(fixtures_dir, name, 0)
    E, X = R["E"], R["X"]
    Cd = candidates(R, name)
    n = len(Cd["I"])
    pairs = np.stack([Cd["I"], Cd["J"]], axis=1)
    grp = ops.group_of(E, nn)
    out = grp.ml_pair_gate(X, pairs, (Cd["R"], Cd["t"], Cd["Om"]))
    res = out["result"]
    cres = grp.ml_covariance(X)[2]
    assert res.outcome == dpgo_amd.PAIRS_OK and res.stationarity == cres.stationarity and res.pivot_min > 0 and res.device_bytes > 0
    assert res.columns == R["dof"] * len(set(pairs.reshape(-1).tolist()) - {0}) and res.batches >= 1
    jw, w_r, w_rel, w_d2 = check_gate(R, Cd, out)
    print("%s x %d: %d candidates, joint %.3g of bSigma, residual %.3g, rel %.3g and d2 %.3g of their bounds; d2 from %.3g to %.3g"
          % (name, nn, n, jw, w_r, w_rel, w_d2, out["d2"].min(), out["d2"].max()))
    assert jw < 1.0 and w_r <= 1.0 and w_rel <= 1.0 and w_d2 <= 1.0
    # a candidate that copies an edge of the graph has that edge's residual bit for bit
    r_dev = grp.ml_eval(X)[1]
    cp = Cd["copies"] >= 0
    assert cp.sum() == 5 and np.array_equal(out["residual"][cp], r_dev[Cd["copies"][cp]])
    # the anchor's blocks are exact zeros; p == p has one block three times; the anchor with itself: d2 = r' Omega r
    k_pp, k_0q, k_p0, k_00 = n - 4, n - 3, n - 2, n - 1
    assert not out["joint"][k_0q][:2].any() and out["joint"][k_0q][2].any()
    assert not out["joint"][k_p0][1:].any() and out["joint"][k_p0][0].any()
    assert not out["joint"][k_00].any() and not out["rel"][k_00].any()
    assert np.array_equal(out["joint"][k_pp][0], out["joint"][k_pp][1]) and np.array_equal(out["joint"][k_pp][0], out["joint"][k_pp][2])
    r0 = np.asarray(out["residual"][k_00], LD)
    own = float(r0 @ np.asarray(Cd["Om"][k_00], LD) @ r0)
    assert abs(out["d2"][k_00] - own) <= 8 * R["dof"] * U * float(np.abs(out["residual"][k_00]) @ np.abs(Cd["Om"][k_00]) @ np.abs(out["residual"][k_00]))
    # accept follows the threshold
    thr = float(np.median(out["d2"]))
    acc = grp.ml_pair_gate(X, pairs, (Cd["R"], Cd["t"], Cd["Om"]), threshold=thr)
    assert np.array_equal(acc["d2"], out["d2"]) and np.array_equal(acc["accept"], out["d2"] <= thr) and 0 < acc["accept"].sum() < n
    assert "accept" not in out
    # a candidate's bits do not depend on its companions
    one = grp.ml_pair_gate(X, pairs[2:3], (Cd["R"][2:3], Cd["t"][2:3], Cd["Om"][2:3]))
    for key in ("d2", "residual", "rel", "joint"):
        assert np.array_equal(one[key][0], out[key][2]), key
    none = grp.ml_pair_gate(X, np.zeros((0, 2), np.int32), (np.zeros((0, E["d"], E["d"])), np.zeros((0, E["d"])), np.zeros((0, R["dof"], R["dof"]))))
    assert none["result"].outcome == dpgo_amd.PAIRS_OK and none["d2"].shape == (0,)


def test_skipped_not_pd_and_refusals(fixtures_dir, capfd):
    R = tgc.reference(fixtures_dir, "smallGrid3D", 0)
    E, X, N = R["E"], R["X"], R["N"]
    Cd = candidates(R, "smallGrid3D")
    pairs, cand = np.stack([Cd["I"], Cd["J"]], axis=1), (Cd["R"], Cd["t"], Cd["Om"])
    grp = ops.group_of(E, 2)
    grp.ml_pair_gate(X, pairs, cand, max_bytes=1)   # (the certificate's buffers come here)
    free0 = tgp.device_free_bytes()
    sk = grp.ml_pair_gate(X, pairs, cand, max_bytes=1)
    assert tgp.device_free_bytes() == free0
    assert sk["result"].outcome == dpgo_amd.PAIRS_SKIPPED and sk["result"].device_bytes > 1 and sk["result"].columns > 0
    assert not sk["d2"].any() and not sk["joint"].any() and sk["result"].stationarity == 0
    ok = grp.ml_pair_gate(X, pairs, cand, max_bytes=sk["result"].device_bytes)
    assert ok["result"].outcome == dpgo_amd.PAIRS_OK
    assert grp.ml_pair_gate(X, pairs, cand, max_bytes=sk["result"].device_bytes - 1)["result"].outcome == dpgo_amd.PAIRS_SKIPPED
    bad = grp.ml_pair_gate(X, pairs, cand, graph=tgr.cut_graph(E, 7, 2))
    assert bad["result"].outcome == dpgo_amd.PAIRS_NOT_PD and not bad["d2"].any() and not bad["rel"].any()
    again = grp.ml_pair_gate(X, pairs, cand)
    for key in ("d2", "residual", "rel", "joint"):
        assert np.array_equal(again[key], ok[key])
    # a candidate whose information matrix is not symmetric positive definite is refused by name
    capfd.readouterr()
    for change in ("negative", "asymmetric", "nan"):
        Om = Cd["Om"].copy()
        if change == "negative":
            Om[3, 1, 1] = -1.0
        elif change == "asymmetric":
            Om[3, 0, 1] += 1.0
        else:
            Om[3, 2, 2] = np.nan
        with pytest.raises(RuntimeError):
            grp.ml_pair_gate(X, pairs, (Cd["R"], Cd["t"], Om))
        assert "candidate 3" in capfd.readouterr().err
    # the other refusals
    G = tmh.graph_of(E, 2)
    hub = dpgo_amd.NodeGroup(G, range(2), dpgo_amd.Options.driver(dpgo_amd.LOSS_HUBER, True, max_iterations=0))
    part = dpgo_amd.NodeGroup(G, [0], dpgo_amd.Options.driver(LOSS_NONE, True, max_iterations=0))
    other = tmh.graph_of(mi.fixture(fixtures_dir, "tinyGrid3D"), 2)
    notspd = E["Om"].copy()
    notspd[11, 2, 2] = -1.0
    for g, kw in ((hub, {}), (part, {}), (grp, dict(graph=other)), (grp, dict(graph=tmh.graph_of(dict(E, Om=notspd), 2))),
                  (grp, dict(anchor=N)), (grp, dict(anchor=-1))):
        with pytest.raises(RuntimeError):
            g.ml_pair_gate(X, pairs, cand, **kw)
    for p in ([[0, N]], [[-1, 2]]):
        with pytest.raises(RuntimeError):
            grp.ml_pair_gate(X, p, (Cd["R"][:1], Cd["t"][:1], Cd["Om"][:1]))
    with pytest.raises(RuntimeError):
        grp.ml_pair_gate(X[:-1], pairs, cand)
    assert grp.ml_pair_gate(X, pairs, cand)["result"].outcome == dpgo_amd.PAIRS_OK


# ---------------------------------------------------------------------------------------------------------------
# the facade and the driver
# ---------------------------------------------------------------------------------------------------------------
_py = {}
BARC2 = 5.0   # (tests/test_gpu_ml_gnc.py: the threshold at which smallGrid3D loses edges and stays connected)


def python_run(fixtures_dir):
    """What the driver and the facade example do, through Python: chordal point, 20 AMM-PGO# iterations on 2 nodes, the polish,
    the refinement on the file's own information matrices and at its point the records of every edge and the gate of every edge
    of the file as a candidate of its own; then GNC-TLS on chi2 and the same two calls on the graph without the rejected edges."""
    if not _py:
        path = os.path.join(fixtures_dir, "smallGrid3D.g2o")
        G = dpgo_amd.read_g2o(path, 2)
        drv = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(LOSS_NONE, True))
        for _ in range(20):
            assert drv.step() == 0
        Xm, res, _ = drv.group.ml_polish(drv.group.polish(drv.X())[0])
        assert res.outcome == dpgo_amd.POLISH_CONVERGED
        I, J, Rm, t = G.edges()[:4]
        own = (np.stack([I, J], axis=1), (Rm, t, G.edge_information()[0]))
        G1 = dpgo_amd.read_g2o(path, 1)   # (the file as the driver reads a candidate file: one node)
        I1, J1, R1, t1 = G1.edges()[:4]
        cand = (np.stack([I1, J1], axis=1), (R1, t1, G1.edge_information()[0]))
        _py["own"] = (drv.group.ml_edge_reliability(Xm), drv.group.ml_pair_gate(Xm, *own))
        _py["driver"] = (G, drv.group.ml_edge_reliability(Xm), drv.group.ml_pair_gate(Xm, *cand), cand[0])
        Xg, w, gres, _ = drv.group.ml_gnc(G, Xm, dpgo_amd.GncOptions(barc2=BARC2))
        assert gres.outcome == dpgo_amd.GNC_CONVERGED and 0 < np.sum(w > 0) < G.num_edges
        kept = G.filter_edges(w > 0)
        _py["gnc"] = (np.flatnonzero(w > 0), drv.group.ml_edge_reliability(Xg, graph=kept), drv.group.ml_pair_gate(Xg, *cand, graph=kept))
        for v in (_py["own"], _py["driver"][1:3], _py["gnc"][1:]):
            assert v[0]["result"].outcome == dpgo_amd.RELY_OK and v[1]["result"].outcome == dpgo_amd.PAIRS_OK
    return _py


def test_cpp_facade_ml_reliability(fixtures_dir):
    """examples/facade_mm.cpp with `ml_reliability`: DPGOHashGroup::ml_edge_reliability and ::ml_pair_gate at ::ml_polish's point,
    on stderr; stdout the same trace as without; the records and the gate those of the Python calls bit for bit."""
    exe = os.path.join(tgp.ROOT, "dpgo_amd", "facade_mm")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    args = [exe, os.path.join(fixtures_dir, "smallGrid3D.g2o"), "2", "20", "trivial", "1"]
    plain = subprocess.run(args, check=True, capture_output=True, text=True, timeout=300)
    out = subprocess.run(args + ["ml_reliability"], check=True, capture_output=True, text=True, timeout=300)
    assert out.stdout == plain.stdout and "ml reliability" not in plain.stderr and "ml gate" not in plain.stderr
    rely, gate = python_run(fixtures_dir)["own"]
    res = rely["result"]
    m = res.edges
    lines = [l.split() for l in out.stderr.splitlines() if l.startswith("ml reliability: ")]
    assert len(lines) == m + 1
    assert lines[-1][2:6] == ["OK", dpgo_amd.RELY_METHOD_NAMES[res.method_used], str(m), str(res.flagged)]
    assert float(lines[-1][6]) == res.redundancy_sum
    assert [int(l[3]) for l in lines[:m]] == list(range(m))
    assert np.array_equal(np.array([[float(v) for v in l[4:]] for l in lines[:m]]), rely["records"])
    glines = [l.split() for l in out.stderr.splitlines() if l.startswith("ml gate: ")]
    assert len(glines) == m + 1 and glines[-1][2:] == ["OK", str(gate["result"].columns), str(gate["result"].batches)]
    got = np.array([[float(v) for v in l[4:]] for l in glines[:m]])
    assert np.array_equal(got[:, 0], gate["d2"]) and np.array_equal(got[:, 1] != 0, gate["not_pd"]) and np.array_equal(got[:, 2:], gate["residual"])
    # every edge as its own candidate: its residual is the record's, bit for bit
    assert np.array_equal(gate["residual"], rely["residual"])


def driver_run(fixtures_dir, tmp_path, more):
    exe = os.path.join(tgp.ROOT, "dpgo_amd", "dist_pgo")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    path = os.path.join(fixtures_dir, "smallGrid3D.g2o")
    base = [exe, "--dataset", path, "--num_nodes", "2", "--iters", "20", "--dist_init", "false", "--save", "false", "--polish", "--ml_polish"] + more
    plain = subprocess.run(base, capture_output=True, text=True, cwd=tmp_path, timeout=300)
    run = subprocess.run(base + ["--ml_edge_reliability", "mlrely.txt", "--ml_gate_candidates", path, "--ml_gate_report", "mlgate.txt"],
                         capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert plain.returncode == 0 and run.returncode == 0, run.stderr[-2000:]
    steady = lambda text: [l for l in text.splitlines() if not l.startswith(("time: ", "ml reliability: ", "ml gate: "))]   # noqa: E731
    assert steady(plain.stdout) == steady(run.stdout) and "ml reliability" not in plain.stdout and "ml gate" not in plain.stdout
    return run


def check_driver(run, tmp_path, edge_ids, I, J, rely, gate, pairs):
    res, gres = rely["result"], gate["result"]
    f = [l for l in run.stdout.splitlines() if l.startswith("ml reliability: ")][0].split()
    assert f[2:4] == ["OK", dpgo_amd.RELY_METHOD_NAMES[res.method_used]] and [int(v) for v in f[4:6]] == [res.edges, res.flagged]
    assert float(f[6]) == res.redundancy_sum and int(f[7]) == res.device_bytes and float(f[9]) == float("%.16g" % res.stationarity)
    rows = np.loadtxt(tmp_path / "mlrely.txt")
    assert rows.shape == (res.edges, 9) and np.array_equal(rows[:, 0], edge_ids)
    assert np.array_equal(rows[:, 1], I[edge_ids]) and np.array_equal(rows[:, 2], J[edge_ids])
    assert np.array_equal(rows[:, 3:], rely["records"][:, [2, 3, 4, 0, 1, 5]])
    g = [l for l in run.stdout.splitlines() if l.startswith("ml gate: ")][0].split()
    assert g[2] == "OK" and [int(v) for v in g[3:7]] == [len(pairs), gres.columns, gres.batches, gres.device_bytes]
    got = np.loadtxt(tmp_path / "mlgate.txt")
    dof = gate["rel"].shape[-1]
    iu = np.triu_indices(dof)
    assert got.shape == (len(pairs), 5 + len(iu[0])) and np.array_equal(got[:, :2], pairs) and np.array_equal(got[:, 2], gate["d2"])
    assert np.all(got[:, 3] == dof) and np.array_equal(got[:, 4] != 0, gate["not_pd"])
    assert np.array_equal(got[:, 5:], np.array([r[iu] for r in gate["rel"]]))


def test_dist_pgo_ml_reliability_and_gate_flags(fixtures_dir, tmp_path):
    """--ml_edge_reliability and --ml_gate_candidates / --ml_gate_report behind --polish --ml_polish add one line each and their
    two files, which hold the Python calls' numbers bit for bit; without them stdout is what it was."""
    run = driver_run(fixtures_dir, tmp_path, [])
    G, rely, gate, pairs = python_run(fixtures_dir)["driver"]
    I, J = G.edges()[:2]
    check_driver(run, tmp_path, np.arange(G.num_edges), I, J, rely, gate, pairs)


def test_dist_pgo_ml_flags_behind_ml_gnc_act_on_the_kept_edges(fixtures_dir, tmp_path):
    run = driver_run(fixtures_dir, tmp_path, ["--ml_gnc", "tls", "--ml_gnc_barc2", "%.17g" % BARC2])
    G = python_run(fixtures_dir)["driver"][0]
    kept, rely, gate = python_run(fixtures_dir)["gnc"]
    I, J = G.edges()[:2]
    assert 0 < len(kept) < G.num_edges and rely["result"].edges == len(kept)
    check_driver(run, tmp_path, kept, I, J, rely, gate, python_run(fixtures_dir)["driver"][3])
