"""Joint compatibility and budgeted selection of loop-closure candidates on the device (dpgo_amd/csrc/cand.h):
NodeGroup.candidate_set on tinyGrid3D x {1, 2} nodes, smallGrid3D x {1, 5} and the d = 2 ladder x 6, anchors 0 and N - 1, at the
POLISHED points and with the references and groups of tests/test_gpu_pairs.py.  The measurements are the estimate's own relative
poses perturbed on the CPU (tests/test_pairs_host.py: seeded_candidate).

Bounds (tests/cand_restatement.py); nothing in them comes from the device.
  cov, S, r        margin_cov with bSigma, bound_S, pairs_restatement.margin_residual
  S^-1, logdet     marg_restatement.info_bound / logdet_bound from bound_S; rho <= 0.1 is asserted on every input
  d2_joint         d2_joint_bound; gain_all: half the logdet bound plus the weights' logarithms
  own d2           of candidate i, from the delivered S_ii and r_i in long double, against pair_covariance's d2: the sum of the two
                   margin_d2's
  selection        the order is the long-double greedy's, whose every decision is checked on the CPU to sit GAP_FACTOR times its
                   bounds (with the inputs' own error in them) away from the alternative; the records within step_bounds
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cand_restatement as cd  # noqa: E402
import cov_restatement as cr  # noqa: E402
import marg_restatement as mr  # noqa: E402
import pairs_restatement as pr  # noqa: E402
import test_cand_host as tch  # noqa: E402  (its comparisons; none of its tests is imported)
import test_gpu_certify as tc  # noqa: E402  (its inputs; none of its tests is imported)
import test_gpu_covariance as tgc  # noqa: E402  (its groups; none of its tests is imported)
import test_gpu_cert_proof as tp  # noqa: E402
import test_gpu_pairs as tgp  # noqa: E402  (its polished points and references; none of its tests is imported)
import test_pairs_host as tph  # noqa: E402

import dpgo_amd  # noqa: E402
from oracle.problem import LOSS_NONE  # noqa: E402

pytestmark = pytest.mark.gpu

LD, U = cd.LD, cd.U
# (fixture, nodes, candidates, budget): d = 3, 9 candidates have 10 end poses, 54 columns in one batch; 22 have 33, 198 columns in
# four batches; d = 2: 22 candidates, 34 end poses, 102 columns in two batches
CASES = [("tinyGrid3D", 1, 4, 4), ("tinyGrid3D", 2, 6, 6), ("smallGrid3D", 1, 9, 4), ("smallGrid3D", 5, 22, 4), ("ladder2", 6, 22, 4)]

WEIGHT_MAX, WEIGHT_STEP, WEIGHT_WEAK = 10.0, 5.0, 0.02

_want = {}


def wanted(fixtures_dir, name, anchor, m, budget, seed=63):
    """The long-double answers and the bounds of a seeded candidate set at the polished point, once.  The seed is one under which
    every case below meets the selection's conditions with room to spare at the unpolished points of tests/test_pairs_host.py: it
    was picked there, on the CPU."""
    key = (name, anchor, m, budget, seed)
    if key not in _want:
        R = tgp.reference(fixtures_dir, name, anchor)
        d, dof, X, N = R["d"], R["dof"], R["X"], R["N"]
        pairs = tch.seeded_set(N, anchor, seed + m, m)
        if m >= 2:
            pairs[1] = (1, N - 1) if anchor == 0 else (0, N - 2)   # (the two ends of the range: different nodes of every partition)
        rng = np.random.default_rng(seed + m + 1)
        # The weights: `budget` strong candidates, in seeded places, a factor WEIGHT_STEP apart from WEIGHT_MAX down, and the
        # others weak (WEIGHT_WEAK).  The gains of the strong ones then lie further apart than the selection's bounds -- which
        # carry bSigma, the Hessian's own error, into every conditional covariance -- the weak ones lie below them all, and
        # |C_i^-1|_2 <= max(tau_i, 2 kappa_i) keeps rho_i' <= 0.1: the conditions are asserted below on the CPU
        # (select_reference), before the device is asked.  The budget ends the selection where the weak ones would have to be
        # told apart.
        scale = WEIGHT_WEAK * rng.uniform(1.0, 2.0, m)
        scale[rng.permutation(m)[:budget]] = WEIGHT_MAX * WEIGHT_STEP ** (-np.arange(budget, dtype=float))
        cands = [tph.seeded_candidate(X, d, p, q, rng)[:2] + (float(scale[i] / 2), float(scale[i] * rng.uniform(0.7, 1.0)))
                 for i, (p, q) in enumerate(pairs)]
        kappa, tau = np.array([c[2] for c in cands]), np.array([c[3] for c in cands])
        K, kpos = cd.pose_list(pairs)
        sig = mr.sigma_kk(R["A"], dof, K, anchor, R["L"])
        cov = cd.cov_of(cd.jacobian_cand(X, d, pairs, K, LD), sig)
        S = cd.innovation(cov, d, kappa, tau, LD)
        r = cd.residuals(X, d, pairs, cands, LD)
        m_cov = cd.margin_cov(X, d, pairs, K, anchor, np.asarray(sig, np.float64), R["bSigma"])
        b_S = cd.bound_S(m_cov, np.asarray(S, np.float64), d, kappa, tau)
        m_r = cd.margin_residuals(X, d, pairs, cands)
        rho = mr.rho_of(S, b_S)
        assert rho <= 0.1, "the candidate set does not satisfy the condition rho <= 0.1: %g" % rho
        Sinv, logdet, d2j, gain_all, sal = cd.joint(S, r, d, kappa, tau)
        b_info = mr.info_bound(S, b_S)
        b_logdet = mr.logdet_bound(S, b_S, sal)
        ref = tch.select_reference(d, np.asarray(S, np.float64), np.asarray(r, np.float64), kappa, tau, budget,
                                   E_in=float(np.linalg.norm(b_S, 2)), er_in=float(np.linalg.norm(m_r)))
        packed = dpgo_amd.pack_candidates(d, m, [c[0] for c in cands], [c[1] for c in cands], kappa, tau)
        _want[key] = dict(pairs=pairs, cands=cands, kappa=kappa, tau=tau, K=K, packed=packed, cov=cov, S=S, r=r, Sinv=Sinv, logdet=logdet,
                          d2j=d2j, gain_all=gain_all, m_cov=m_cov, b_S=b_S, m_r=m_r, b_info=b_info, b_logdet=b_logdet, rho=rho,
                          b_d2j=cd.d2_joint_bound(Sinv, r, m_r, b_info), b_gain=b_logdet / 2 + float(cd.omega_log_bound(d, kappa, tau).sum()),
                          ref=ref)
    return _want[key]


def ratios(out, W):
    return np.array([tch.worst(out["cov"], W["cov"], W["m_cov"]), tch.worst(out["S"], W["S"], W["b_S"]),
                     tch.worst(out["residual"], W["r"], W["m_r"]), float(np.abs(np.asarray(out["info"], LD) - W["Sinv"]).max() / W["b_info"]),
                     float(abs(LD(out["logdet"]) - W["logdet"]) / W["b_logdet"]), float(abs(LD(out["d2_joint"]) - W["d2j"]) / W["b_d2j"]),
                     float(abs(LD(out["gain_all"]) - W["gain_all"]) / W["b_gain"])])


def as_compare(out, budget):
    """candidate_set's dict in the shape tch.select_compare reads (whole arrays, -1 and zeros past n_selected)."""
    k = out["result"].n_selected
    sel, steps = np.full(budget, -1, np.int32), np.zeros((budget, 4))
    sel[:k], steps[:k] = out["selected"], out["steps"]
    return {"selected": sel, "steps": steps, "n_selected": k, "gain_selected": out["gain_selected"], "d2_selected": out["d2_selected"]}


_first = {}


@pytest.mark.parametrize("name,nn,m,budget", CASES)
def test_candidate_set_against_the_restatement(fixtures_dir, name, nn, m, budget):
    grp = tgc.make_group(fixtures_dir, name, nn)
    N = tp.instance(fixtures_dir, name)[0]
    for a in (0, N - 1):
        R = tgp.reference(fixtures_dir, name, a)
        d, dof = R["d"], R["dof"]
        W = wanted(fixtures_dir, name, a, m, budget)
        if nn > 1 and m >= 2:
            assert len({tgp.node_of(grp, g) for g in W["K"]}) > 1
        out = grp.candidate_set(R["X"], W["pairs"], W["packed"], anchor=a, budget=budget)
        res = out["result"]
        ncol = dof * (len(W["K"]) - (1 if a in W["K"] else 0))
        assert res.outcome == dpgo_amd.CAND_OK and not res.joint_not_pd and res.unknowns == dof * N and res.pivot_min > 0
        assert res.n == dof * m and res.poses == len(W["K"]) and res.columns == ncol and res.batches == (ncol + 63) // 64
        assert out["poses"].tolist() == W["K"] and res.dense_pivot_min > 0 and res.device_bytes > 0 and res.n_selected == budget
        w = ratios(out, W)
        print("%s x %d, anchor %d, m = %d: n = %d, %d poses, %d batches, rho %.3g; cov %.3g, S %.3g, r %.3g, info %.3g, logdet %.3g, "
              "d2_joint %.3g, gain_all %.3g of their bounds" % ((name, nn, a, m, res.n, res.poses, res.batches, W["rho"]) + tuple(w)))
        assert w.max() < 1.0, w
        assert all(np.array_equal(out[k], out[k].T) for k in ("cov", "S", "info"))
        tch.select_compare(as_compare(out, budget), W["ref"], budget)
        # every candidate's own d2, from the delivered S_ii and r_i, against pair_covariance's
        pc = grp.pair_covariance(R["X"], W["pairs"], anchor=a, candidates=tuple(np.stack([np.asarray(c[i]) for c in W["cands"]]) for i in range(4)))
        tgp.need(R, W["pairs"])
        for i, (p, q) in enumerate(W["pairs"]):
            sl = slice(dof * i, dof * i + dof)
            ck = W["cands"][i]
            own = cd.block_stats(np.asarray(out["S"][sl, sl], LD), np.asarray(out["residual"][sl], LD))[2]
            Sj = pr.joint_of(R["Sigma"], dof, p, q, a)
            rel_ld = pr.rel_cov(pr.jacobian(R["X"], d, p, q, LD), Sj)
            m_d2 = pr.margin_d2(rel_ld, W["r"][sl], d, ck[2], ck[3], pr.margin_rel(R["X"], d, p, q, np.asarray(Sj, np.float64), R["bSigma"]), W["m_r"][sl])
            assert abs(own - LD(pc["d2"][i])) <= 2 * m_d2, (i, float(own), pc["d2"][i], m_d2)
        # the same bits on a second call; a smaller budget is a prefix; without the joint test the same cov and selection
        again = grp.candidate_set(R["X"], W["pairs"], W["packed"], anchor=a, budget=budget)
        assert all(np.array_equal(again[k], out[k]) for k in ("cov", "S", "info", "residual", "selected", "steps"))
        assert (again["logdet"], again["d2_joint"], again["gain_selected"]) == (out["logdet"], out["d2_joint"], out["gain_selected"])
        bare = grp.candidate_set(R["X"], W["pairs"], W["packed"], anchor=a, budget=2, want_joint=False)
        assert all(bare[k] is None for k in ("info", "logdet", "d2_joint", "gain_all")) and np.array_equal(bare["S"], out["S"])
        assert np.array_equal(bare["selected"], out["selected"][:2]) and np.array_equal(bare["steps"], out["steps"][:2])
        none = grp.candidate_set(R["X"], W["pairs"], W["packed"], anchor=a, want_cov=False)
        assert none["cov"] is None and none["S"] is None and len(none["selected"]) == 0 and none["d2_joint"] == out["d2_joint"]
        # every partition: other orderings, other fronts, the same answer
        first = _first.setdefault((name, a, m, budget), out)
        assert np.all(np.abs(out["cov"] - first["cov"]) <= 2 * W["m_cov"]) and np.abs(out["info"] - first["info"]).max() <= 2 * W["b_info"]
        assert np.array_equal(out["selected"], first["selected"])


def test_a_point_that_is_no_minimum_and_the_calls_around_it(fixtures_dir):
    R = tgp.reference(fixtures_dir, "smallGrid3D", 0)
    grp = tgc.make_group(fixtures_dir, "smallGrid3D", 2)
    W = wanted(fixtures_dir, "smallGrid3D", 0, 9, 4)
    before = grp.candidate_set(R["X"], W["pairs"], W["packed"], budget=4)
    bad = grp.candidate_set(cr.random_rotations_point(R["X"], R["d"], 5), W["pairs"], W["packed"], budget=4)
    assert bad["result"].outcome == dpgo_amd.CAND_NOT_PD and not bad["cov"].any() and not bad["S"].any() and not bad["info"].any()
    assert bad["logdet"] == 0.0 and bad["d2_joint"] == 0.0 and len(bad["selected"]) == 0 and not bad["residual"].any()
    after = grp.candidate_set(R["X"], W["pairs"], W["packed"], budget=4)
    assert after["result"].outcome == dpgo_amd.CAND_OK
    assert all(np.array_equal(before[k], after[k]) for k in ("cov", "S", "info", "selected", "steps")) and before["logdet"] == after["logdet"]


def test_skipped_allocates_nothing_and_predicts_what_a_run_reports(fixtures_dir):
    R = tgp.reference(fixtures_dir, "smallGrid3D", 0)
    grp = tgc.make_group(fixtures_dir, "smallGrid3D", 2)
    W = wanted(fixtures_dir, "smallGrid3D", 0, 9, 4)
    kw = dict(budget=4)
    grp.candidate_set(R["X"], W["pairs"], W["packed"], max_bytes=1, **kw)   # (the certificate's buffers and M's values come here)
    free0 = tgp.device_free_bytes()
    out = grp.candidate_set(R["X"], W["pairs"], W["packed"], max_bytes=1, **kw)
    assert tgp.device_free_bytes() == free0
    res = out["result"]
    assert res.outcome == dpgo_amd.CAND_SKIPPED and not out["cov"].any() and not out["info"].any() and len(out["selected"]) == 0
    assert res.unknowns == 6 * R["N"] and res.n == 54 and res.poses == len(W["K"]) and res.columns == 6 * (len(W["K"]) - 1) and res.batches == 1
    assert res.stationarity > 0 and out["poses"].tolist() == W["K"]
    assert grp.candidate_set(R["X"], W["pairs"], W["packed"], max_bytes=res.device_bytes - 1, **kw)["result"].outcome == dpgo_amd.CAND_SKIPPED
    ok = grp.candidate_set(R["X"], W["pairs"], W["packed"], max_bytes=res.device_bytes, **kw)
    assert ok["result"].outcome == dpgo_amd.CAND_OK and ok["result"].device_bytes == res.device_bytes
    assert ratios(ok, W).max() < 1.0 and ok["selected"].tolist() == W["ref"][0]
    # without the joint test no dense factor is counted: the prediction falls by exactly the dense factor of order 54 (what
    # dpgo_debug_marg_dense reports for that order) and the buffer of S^-1 with its two scalars -- the call never asks
    # MargCache for it
    bare = grp.candidate_set(R["X"], W["pairs"], W["packed"], want_joint=False, max_bytes=1, **kw)["result"]
    dense = dpgo_amd.marg_dense_debug(ok["S"])["result"].device_bytes
    assert bare.outcome == dpgo_amd.CAND_SKIPPED and res.device_bytes - bare.device_bytes == dense + 8 * (54 * 54 + 2)
    got = grp.candidate_set(R["X"], W["pairs"], W["packed"], want_joint=False, max_bytes=bare.device_bytes, **kw)
    assert got["result"].outcome == dpgo_amd.CAND_OK and got["result"].device_bytes == bare.device_bytes and got["info"] is None
    assert got["selected"].tolist() == W["ref"][0] and got["result"].dense_pivot_max == 0.0


def test_refusals(fixtures_dir):
    path, N, mm, gp, X0 = tc.problem(fixtures_dir, "smallGrid3D")
    X = tgp.reference(fixtures_dir, "smallGrid3D", 0)["X"]
    W = wanted(fixtures_dir, "smallGrid3D", 0, 9, 4)
    two = W["packed"][:2]
    G = dpgo_amd.read_g2o(path, 2)
    hub = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(dpgo_amd.LOSS_HUBER, True), X0=X0)
    with pytest.raises(RuntimeError):
        hub.group.candidate_set(X, [(1, 5), (3, 9)], two)              # a robust loss
    part = dpgo_amd.NodeGroup(G, [0], dpgo_amd.Options.driver(LOSS_NONE, True))
    with pytest.raises(RuntimeError):
        part.candidate_set(X, [(1, 5), (3, 9)], two)                   # a group that does not host every node
    grp = tgc.make_group(fixtures_dir, "smallGrid3D", 2)
    zero_kappa, neg_tau = two.copy(), two.copy()
    zero_kappa[1, -2], neg_tau[0, -1] = 0.0, -1.0
    bad = [dict(pairs=[(1, 5), (3, 9)], candidates=two, anchor=N), dict(pairs=[(1, 5), (3, 9)], candidates=two, anchor=-1),
           dict(pairs=[(1, N), (3, 9)], candidates=two), dict(pairs=[(-1, 3), (3, 9)], candidates=two),
           dict(pairs=[(1, 5), (4, 4)], candidates=two),                # p == q
           dict(pairs=[(1, 5), (3, 9)], candidates=zero_kappa), dict(pairs=[(1, 5), (3, 9)], candidates=neg_tau)]
    for kw in bad:
        with pytest.raises(RuntimeError):
            grp.candidate_set(X, **kw)
    with pytest.raises(RuntimeError):
        grp.candidate_set(X[:-1], [(1, 5), (3, 9)], two)
    with pytest.raises(ValueError):
        grp.candidate_set(X, [(1, 5), (3, 9)], two, budget=-1)
    with pytest.raises(ValueError):
        grp.candidate_set(X, np.zeros((0, 2), int), two[:0])
    assert grp.candidate_set(X, [(1, 5), (3, 9)], two, budget=1)["result"].outcome == dpgo_amd.CAND_OK


def test_candidate_set_does_not_disturb_the_optimiser(fixtures_dir):
    """30 AMM-PGO# iterations with a call on a sibling trivial-loss group after every fifth: bit for bit the run without."""
    path = tc.problem(fixtures_dir, "smallGrid3D")[0]
    W = wanted(fixtures_dir, "smallGrid3D", 0, 9, 4)
    runs = []
    for with_call in (False, True):
        drv = dpgo_amd.DistPGO(dpgo_amd.read_g2o(path, 2), dpgo_amd.Options.driver(LOSS_NONE, True))
        sib = tc.group(path, 2)[0] if with_call else None
        trace = []
        for it in range(30):
            assert drv.step() == 0
            if with_call and it % 5 == 4:
                assert sib.candidate_set(drv.X(), W["pairs"], W["packed"], budget=3)["result"].outcome in (dpgo_amd.CAND_OK, dpgo_amd.CAND_NOT_PD)
            trace.append([getattr(drv.group.results(a), f) for a in range(2) for f in ("fobj", "gamma", "gradFnorm", "Gk")])
        runs.append((np.array(drv.X()), [drv.group[a].Xk() for a in range(2)], np.array(trace)))
    assert np.array_equal(runs[0][0], runs[1][0])
    for a in range(2):
        assert np.array_equal(runs[0][1][a], runs[1][1][a])
    assert np.array_equal(runs[0][2], runs[1][2])


def test_reweighted_with_unit_weights_is_the_group_call(fixtures_dir):
    path = tc.problem(fixtures_dir, "smallGrid3D")[0]
    R = tgp.reference(fixtures_dir, "smallGrid3D", 0)
    W = wanted(fixtures_dir, "smallGrid3D", 0, 9, 4)
    G = dpgo_amd.read_g2o(path, 2)
    got = dpgo_amd.candidate_set_reweighted(G, R["X"], LOSS_NONE, W["pairs"], W["packed"], budget=4)
    want = tgc.make_group(fixtures_dir, "smallGrid3D", 2).candidate_set(R["X"], W["pairs"], W["packed"], budget=4)
    assert got["result"].outcome == dpgo_amd.CAND_OK and got["summary"].num_downweighted == 0
    assert all(np.array_equal(got[k], want[k]) for k in ("cov", "S", "info", "residual", "selected", "steps", "poses"))
    assert (got["logdet"], got["d2_joint"], got["gain_all"], got["gain_selected"]) == (want["logdet"], want["d2_joint"], want["gain_all"], want["gain_selected"])


# ---------------------------------------------------------------------------------------------------------------
# the drivers
# ---------------------------------------------------------------------------------------------------------------
INFO = "100 0 0 0 0 0   100 0 0 0 0   100 0 0 0   25 0 0   25 0   25"
# tinyGrid3D (nine poses): measurements a little off the grid's own relative poses; two share pose 1, one is reversed
CAND_EDGES = [(1, 7, "1.05 1.98 0.02   0 0 0 1"), (1, 5, "1.9 1.1 -0.05   0.01 -0.02 0.03 0.9993"),
              (6, 2, "-0.1 -1.0 0.0   0 0 0 1"), (3, 8, "2.0 1.02 0.1   0.02 0.0 0.0 0.9998"), (2, 4, "0.5 0.5 0.0   0 0 0 1")]
_py = {}


def python_run(fixtures_dir, cand_path, budget):
    """What the drivers do on tinyGrid3D x 2: 30 iterations, the polish, the candidate set read by the same loader."""
    if budget not in _py:
        drv = dpgo_amd.DistPGO(dpgo_amd.read_g2o(os.path.join(fixtures_dir, "tinyGrid3D.g2o"), 2), dpgo_amd.Options.driver(LOSS_NONE, True))
        for _ in range(30):
            assert drv.step() == 0
        Xp, pres, _ = drv.group.polish(drv.X())
        assert pres.outcome == dpgo_amd.POLISH_CONVERGED
        I, J, R, t, kappa, tau = dpgo_amd.read_g2o(str(cand_path), 1).edges()
        assert I.tolist() == [c[0] for c in CAND_EDGES] and J.tolist() == [c[1] for c in CAND_EDGES]
        out = drv.group.candidate_set(Xp, np.stack([I, J], axis=1), (R, t, kappa, tau), budget=budget)
        assert out["result"].outcome == dpgo_amd.CAND_OK and not out["result"].joint_not_pd
        _py[budget] = (out, I, J)
    return _py[budget]


def write_candidates(tmp_path):
    cand = tmp_path / "cand.g2o"
    cand.write_text("".join("EDGE_SE3:QUAT %d %d   %s   %s\n" % (p, q, pose, INFO) for p, q, pose in CAND_EDGES))
    return cand


def test_dist_pgo_select_flags(fixtures_dir, tmp_path):
    """--polish --select_candidates FILE --select_report FILE [--select_budget K] adds the report and one line after the summary;
    the report holds NodeGroup.candidate_set's numbers bit for bit; a robust loss says why not; one flag alone is an error."""
    import subprocess
    exe = os.path.join(tc.ROOT, "dpgo_amd", "dist_pgo")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    cand = write_candidates(tmp_path)
    path = os.path.join(fixtures_dir, "tinyGrid3D.g2o")
    common = [exe, "--dataset", path, "--num_nodes", "2", "--iters", "30", "--dist_init", "false", "--save", "false"]
    for budget, extra in ((5, []), (2, ["--select_budget", "2"])):
        run = subprocess.run(common + ["--polish", "--select_candidates", str(cand), "--select_report", "sel.txt"] + extra, capture_output=True,
                             text=True, cwd=tmp_path, timeout=300)
        assert run.returncode == 0, run.stderr[-2000:]
        lines = [l for l in run.stdout.splitlines() if l.startswith("candidates: ")]
        assert len(lines) == 1 and run.stdout.rstrip().splitlines()[-1] == lines[0]
        want, I, J = python_run(fixtures_dir, cand, budget)
        res = want["result"]
        f = lines[0].split()
        assert f[1] == "OK" and [int(v) for v in f[2:10]] == [5, res.n, res.poses, res.columns, res.batches, res.device_bytes, 0, budget]
        assert float(f[10]) == want["d2_joint"] and float(f[11]) == want["gain_all"]
        text = (tmp_path / "sel.txt").read_text().splitlines()
        h = text[0].split()
        assert h[:2] == ["n", str(res.n)] and (float(h[3]), float(h[5]), float(h[7])) == (want["logdet"], want["d2_joint"], want["gain_all"])
        h = text[1].split()
        assert h[:2] == ["selected", str(budget)] and (float(h[3]), float(h[5])) == (want["gain_selected"], want["d2_selected"])
        for k in range(budget):
            row = text[2 + k].split()
            s = int(want["selected"][k])
            assert [int(row[0]), int(row[1]), int(row[2]), int(row[5])] == [s, I[s], J[s], int(want["steps"][k][3])]
            assert (float(row[3]), float(row[4])) == (want["steps"][k][1], want["steps"][k][2])
        rows = np.array([[float(v) for v in l.split()] for l in text[2 + budget:]])
        assert rows.shape == (2 * res.n, res.n)
        assert np.array_equal(rows[:res.n], want["S"]) and np.array_equal(rows[res.n:], want["info"])
    hub = subprocess.run(common + ["--loss", "huber", "--select_candidates", str(cand), "--select_report", "s2.txt"], capture_output=True,
                         text=True, cwd=tmp_path, timeout=300)
    assert hub.returncode == 0 and "candidates: not computed" in hub.stdout and not (tmp_path / "s2.txt").exists()
    one = subprocess.run(common[:-6] + ["--iters", "1", "--dist_init", "false", "--save", "false", "--select_candidates", str(cand)],
                         capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert one.returncode != 0


def test_cpp_facade_candidate_set(fixtures_dir, tmp_path):
    """examples/facade_mm.cpp with `candidates FILE BUDGET`: DPGOHashGroup::newton_polish and ::candidate_set after the loop, on
    stderr; stdout the same trace as without; S, info, the scalars and the steps those of NodeGroup.candidate_set bit for bit; a
    candidate that joins a pose to itself refused."""
    import subprocess
    exe = os.path.join(tc.ROOT, "dpgo_amd", "facade_mm")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    cand = write_candidates(tmp_path)
    args = [exe, os.path.join(fixtures_dir, "tinyGrid3D.g2o"), "2", "30", "trivial", "1"]
    plain = subprocess.run(args, check=True, capture_output=True, text=True, timeout=300)
    for budget in (5, 2):
        out = subprocess.run(args + ["candidates", str(cand), str(budget)], check=True, capture_output=True, text=True, timeout=300)
        assert out.stdout == plain.stdout and "candidates" not in plain.stderr
        lines = [l.split() for l in out.stderr.splitlines() if l.startswith("candidates: ")]
        want = python_run(fixtures_dir, cand, budget)[0]
        res = want["result"]
        n = res.n
        assert len(lines) == 2 * n + budget + 2 and lines[-2][1:5] == ["OK", str(n), str(res.poses), str(budget)]
        assert [float(v) for v in lines[-2][5:10]] == [want["logdet"], want["d2_joint"], want["gain_all"], want["gain_selected"], want["d2_selected"]]
        got = {w: np.array([[float(v) for v in l[3:]] for l in lines if l[1] == w]) for w in ("S", "info")}
        assert np.array_equal(got["S"], want["S"]) and np.array_equal(got["info"], want["info"])
        steps = [l for l in lines if l[1] == "step"]
        assert [int(l[3]) for l in steps] == want["selected"].tolist()
        assert np.array_equal(np.array([[float(l[4]), float(l[5]), float(l[6])] for l in steps]), want["steps"][:, 1:])
        assert lines[-1][1:] == ["self", "pair", "-1"]
