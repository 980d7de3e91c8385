"""Candidate-set benchmark: NodeGroup.candidate_set (the tangent-space Hessian written on the device and factored, the unit
columns of the candidates' end poses solved in batches of 64, the joint innovation covariance block by block, the dense
one-front factorisation of order n = dof m and its inverse, the greedy selection on the device; dpgo_amd/csrc/cand.cpp) on one
GPU.

  python tools/cand_bench.py [--inputs torus3D,sphere2500,M3500,city10000] [--reps 3] [--iters 300] [--max-candidates 280]
                             [--budget 32] [--d2-max 0]

Inputs: tools/cov_bench.py's -- torus3D x 8, sphere2500 x 4, M3500 x 4 and city10000 x 8 -- after --iters AMM-PGO# iterations
(LOSS_NONE, driver options) and NodeGroup.polish.  The candidates are seeded pairs of inter-node boundary poses that lie on
different nodes; a measurement is the estimate's own relative pose moved by a seeded 0.05 rad and 0.05 length, with seeded weights
in [5, 50].  --max-candidates thins them so that n stays inside the widest root front the dense factor has been measured at
(about 1.7 k: 280 candidates for d = 3).

Per input one JSON line: n, poses, columns, batches, the predicted device bytes, the dense pivots, d2_joint, gain_all, what was
selected, and -- medians of --reps calls after one warm-up call, on the library's host clock -- factor_ms, solve_ms, dense_ms,
select_ms.  Beside them the route that exists without candidate_set, as the reference time: NodeGroup.joint_marginal (absolute) on
the end poses and NodeGroup.pair_covariance for the residuals, then J Sigma J^T, the inverse and the greedy loop in numpy
(reference_ms, and whether the two routes select the same candidates).  The selection streams its panels: per step t it reads
8 n dof (t + 1) bytes of P and S and writes 8 n dof; that count over select_ms is reported against the HBM peak.  Nothing here is
part of bench.py."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import dpgo_amd  # noqa: E402
import cov_bench  # noqa: E402  (its inputs)
import marg_bench  # noqa: E402  (its boundary poses)

PEAK_HBM = 8.0e12


def record(X, d, N, p):
    return X[p], X[N + d * p:N + d * p + d]


def relative(X, d, N, p, q):
    tp, Yp = record(X, d, N, p)
    tq, Yq = record(X, d, N, q)
    return Yp @ Yq.T, Yp @ (tq - tp)


def exp_so(w, d):
    if d == 2:
        c, s = np.cos(w[0]), np.sin(w[0])
        return np.array([[c, -s], [s, c]])
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + (np.sin(th) / th) * K + ((1 - np.cos(th)) / (th * th)) * (K @ K)


def jacobian(X, d, N, p, q):
    """[J_p J_q] of the relative pose's perturbation (dpgo_amd/csrc/pairs_math.h)."""
    dof = d + d * (d - 1) // 2
    Yp = record(X, d, N, p)[1]
    Rpq, tpq = relative(X, d, N, p, q)
    J = np.zeros((dof, 2 * dof))
    J[:d, :d], J[:d, dof:dof + d] = -Yp, Yp
    if d == 3:
        J[:d, d:dof] = np.array([[0, -tpq[2], tpq[1]], [tpq[2], 0, -tpq[0]], [-tpq[1], tpq[0], 0]])
        J[d:, d:dof] = -Rpq.T
    else:
        J[:d, d] = (tpq[1], -tpq[0])
        J[d, d] = -1
    J[d:, dof + d:] = np.eye(dof - d)
    return J


def draw_candidates(G, X, count, seed=0):
    d, N = G.d, G.num_poses
    dof = d + d * (d - 1) // 2
    b = marg_bench.boundary_poses(G)
    b = b[b != 0]
    off = np.array([G.node_offset(a) for a in range(G.num_nodes)])
    node = lambda p: int(np.searchsorted(off, p, side="right")) - 1
    rng = np.random.default_rng(seed)
    pairs = []
    while len(pairs) < count:
        p, q = (int(v) for v in rng.choice(b, 2, replace=False))
        if node(p) != node(q):
            pairs.append((p, q))
    R, t = [], []
    for p, q in pairs:
        Rpq, tpq = relative(X, d, N, p, q)
        w = rng.standard_normal(dof - d)
        s = rng.standard_normal(d)
        R.append(Rpq @ exp_so(0.05 * w / np.linalg.norm(w), d))
        t.append(tpq + 0.05 * s / np.linalg.norm(s))
    return np.array(pairs, np.int32), (np.array(R), np.array(t), rng.uniform(5, 50, count), rng.uniform(5, 50, count)), len(b)


def reference_route(grp, G, X, pairs, cand, budget, d2_max):
    """joint_marginal on the end poses, pair_covariance for the residuals, the rest in numpy: (ms, d2_joint, gain_all, selected)."""
    d, N = G.d, G.num_poses
    dof = d + d * (d - 1) // 2
    m = len(pairs)
    t0 = time.perf_counter()
    K = [int(g) for g in dict.fromkeys(int(v) for v in pairs.reshape(-1)) if int(g) != 0]
    sig = grp.joint_marginal(X, K, want_info=False)["cov"]
    r = grp.pair_covariance(X, pairs, candidates=cand)["residual"].reshape(-1)
    pos = {g: i for i, g in enumerate(K)}
    J = np.zeros((dof * m, dof * len(K)))
    for i, (p, q) in enumerate(pairs):
        Jpq = jacobian(X, d, N, int(p), int(q))
        for g, blk in ((int(p), Jpq[:, :dof]), (int(q), Jpq[:, dof:])):
            if g in pos:
                J[dof * i:dof * i + dof, dof * pos[g]:dof * pos[g] + dof] = blk
    winv = np.concatenate([np.r_[np.repeat(1 / cand[3][i], d), np.repeat(1 / (2 * cand[2][i]), dof - d)] for i in range(m)])
    S = J @ sig @ J.T + np.diag(winv)
    Sinv = np.linalg.inv(S)
    d2j = float(r @ Sinv @ r)
    gain_all = 0.5 * (np.linalg.slogdet(S)[1] - np.log(winv).sum())
    W, rho, taken, sel = S.copy(), r.copy(), np.zeros(m, bool), []
    lw = np.log(winv).reshape(m, dof).sum(axis=1)
    for _ in range(min(budget, m)):
        best, bi = -np.inf, -1
        for i in range(m):
            if taken[i]:
                continue
            sl = slice(dof * i, dof * i + dof)
            try:
                L = np.linalg.cholesky(W[sl, sl])
            except np.linalg.LinAlgError:
                continue
            z = np.linalg.solve(L, rho[sl])
            if d2_max > 0 and not z @ z <= d2_max:
                continue
            g = np.log(np.diag(L)).sum() - 0.5 * lw[i]
            if g > best:
                best, bi = g, i
        if bi < 0:
            break
        sel.append(bi)
        taken[bi] = True
        sl = slice(dof * bi, dof * bi + dof)
        L = np.linalg.cholesky(W[sl, sl])
        Pn = np.linalg.solve(L, W[sl, :]).T
        rho = rho - Pn @ np.linalg.solve(L, rho[sl])
        W = W - Pn @ Pn.T
    return 1e3 * (time.perf_counter() - t0), d2j, float(gain_all), sel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="torus3D,sphere2500,M3500,city10000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--max-candidates", type=int, default=280)
    ap.add_argument("--budget", type=int, default=32)
    ap.add_argument("--d2-max", type=float, default=0.0)
    a = ap.parse_args()
    med = lambda v: float(np.median(v)) if v else None
    for name in a.inputs.split(","):
        G = cov_bench.graph(name)
        grp = dpgo_amd.NodeGroup(G, range(G.num_nodes), dpgo_amd.Options.driver(dpgo_amd.LOSS_NONE, True, max_iterations=0))
        drv = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(dpgo_amd.LOSS_NONE, True))
        for _ in range(a.iters):
            assert drv.step() == 0
        X0 = np.array(drv.X())
        del drv
        X, pres, _ = grp.polish(X0)
        point = "polished (%s)" % dpgo_amd.POLISH_NAMES[pres.outcome]
        dof = G.d + G.d * (G.d - 1) // 2
        pairs, cand, boundary = draw_candidates(G, np.asarray(X), a.max_candidates)
        kw = dict(budget=a.budget, d2_max=a.d2_max, want_cov=False)
        first = grp.candidate_set(X, pairs, cand, **kw)
        out, r, fac, sol, den, sel = first, first["result"], [], [], [], []
        if r.outcome == dpgo_amd.CAND_OK:
            for _ in range(a.reps):
                out = grp.candidate_set(X, pairs, cand, **kw)
                r = out["result"]
                fac.append(r.factor_ms); sol.append(r.solve_ms); den.append(r.dense_ms); sel.append(r.select_ms)
        line = dict(input=name, point=point, d=G.d, poses=G.num_poses, nodes=G.num_nodes, boundary_poses=boundary, candidates=len(pairs),
                    budget=a.budget, d2_max=a.d2_max, outcome=dpgo_amd.CAND_NAMES[r.outcome], joint_not_pd=r.joint_not_pd, n=r.n,
                    end_poses=r.poses, columns=r.columns, batches=r.batches, device_bytes=r.device_bytes, unknowns=r.unknowns,
                    max_front=r.max_front, n_selected=r.n_selected, factor_ms=med(fac), solve_ms=med(sol), dense_ms=med(den),
                    select_ms=med(sel), dense_pivot_min=r.dense_pivot_min, dense_pivot_max=r.dense_pivot_max, pivot_min=r.pivot_min,
                    stationarity=r.stationarity, d2_joint=out["d2_joint"], gain_all=out["gain_all"], gain_selected=out["gain_selected"],
                    d2_selected=out["d2_selected"])
        if line["select_ms"] and r.n_selected:
            k = r.n_selected
            moved = 8.0 * r.n * dof * sum(t + 2 for t in range(k))
            line["select_bytes"] = moved
            line["select_share_of_hbm_peak"] = moved / (line["select_ms"] * 1e-3) / PEAK_HBM
        if r.outcome == dpgo_amd.CAND_OK:
            refs = [reference_route(grp, G, np.asarray(X), pairs, cand, a.budget, a.d2_max) for _ in range(a.reps + 1)][1:]
            line.update(reference_ms=med([v[0] for v in refs]), reference_d2_joint=refs[-1][1], reference_gain_all=refs[-1][2],
                        same_selection=refs[-1][3] == out["selected"].tolist())
            total = sum(line[k] for k in ("factor_ms", "solve_ms", "dense_ms", "select_ms"))
            line["reference_ms_over_device_ms"] = line["reference_ms"] / total
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
