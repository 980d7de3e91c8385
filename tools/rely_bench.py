"""Edge-reliability benchmark: NodeGroup.edge_reliability (dpgo_amd/csrc/rely.cpp, rely.hip) of EVERY edge of a graph on one GPU,
under both methods, beside the only route there was before it.

  python tools/rely_bench.py [--inputs torus3D,sphere2500,M3500,city10000] [--reps 5] [--iters 300]

Inputs: tools/pair_bench.py's -- torus3D x 8, sphere2500 x 4, M3500 x 4 and city10000 x 8 -- each at its polished point: a run of
--iters AMM-PGO# iterations (LOSS_NONE, driver options), then NodeGroup.polish.  All nodes on one GPU.

Per input and method (SELINV, SOLVE) one JSON line: the sizes of the factorisation, the bytes either method predicts, and -- after
one warm-up call (analysis, allocations, code objects), over --reps calls on the library's host clock, each phase ending in a
synchronise -- the median, minimum and maximum of factor_ms (k_cov_hessian and the factorisation), inverse_ms (the selected
inversion and k_rely_gather, or the batches of block solves) and edge_ms (k_pairs_gate, k_rely_edge and the copies of the records
to the host), the median of the whole call on the caller's clock (call_ms), and what the records say: flagged edges, the sum of
the redundancies against dof (m - N + 1), the median d2_loo.  One more line per input for the route that exists without this
call: NodeGroup.covariance with every edge as a pair -- the whole inverse copied to the host, the marginals and cross blocks
handed out -- and the records computed from them in vectorised numpy (baseline_ms = covariance_ms + numpy_ms, same repetitions),
with the largest difference between its records and the device's.  Nothing here is part of bench.py."""
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


def numpy_records(d, N, X, marg, cross, I, J, R, t, kappa, tau):
    """The records of rely.h from covariance's blocks, all edges at once, in fp64: (m, 6 + 2 dof); flag 1 where C is not
    positive definite."""
    dof, m = d + d * (d - 1) // 2, len(I)
    rows = lambda P: X[N + d * P[:, None] + np.arange(d)[None, :]]   # (m, d, d): Y_p
    Yp, Yq, tp, tq = rows(I), rows(J), X[I], X[J]
    Rpq = Yp @ np.swapaxes(Yq, 1, 2)
    tpq = np.einsum("mij,mj->mi", Yp, tq - tp)
    Jm = np.zeros((m, dof, 2 * dof))
    Jm[:, :d, :d], Jm[:, :d, dof:dof + d] = -Yp, Yp
    if d == 3:
        Jm[:, 0, 4], Jm[:, 0, 5], Jm[:, 1, 3], Jm[:, 1, 5], Jm[:, 2, 3], Jm[:, 2, 4] = -tpq[:, 2], tpq[:, 1], tpq[:, 2], -tpq[:, 0], -tpq[:, 1], tpq[:, 0]
        Jm[:, d:, d:dof] = -np.swapaxes(Rpq, 1, 2)
    else:
        Jm[:, 0, 2], Jm[:, 1, 2], Jm[:, 2, 2] = tpq[:, 1], -tpq[:, 0], -1.0
    Jm[:, np.arange(d, dof), dof + np.arange(d, dof)] = 1.0
    Sj = np.block([[marg[I], cross], [np.swapaxes(cross, 1, 2), marg[J]]])
    rel = Jm @ Sj @ np.swapaxes(Jm, 1, 2)
    E = np.swapaxes(R, 1, 2) @ Rpq
    if d == 3:
        v = 0.5 * np.stack([E[:, 2, 1] - E[:, 1, 2], E[:, 0, 2] - E[:, 2, 0], E[:, 1, 0] - E[:, 0, 1]], axis=1)
        s = np.linalg.norm(v, axis=1)
        theta = np.arctan2(s, 0.5 * (np.trace(E, axis1=1, axis2=2) - 1.0))
        w = v * np.where(s > 1e-8, theta / np.maximum(s, 1e-300), 1.0)[:, None]
    else:
        w = np.arctan2(E[:, 1, 0], E[:, 0, 0])[:, None]
    r = np.concatenate([tpq - t, w], axis=1)
    om = np.concatenate([np.repeat(tau[:, None], d, 1), np.repeat(2 * kappa[:, None], dof - d, 1)], axis=1)
    C = -rel
    C[:, np.arange(dof), np.arange(dof)] += 1.0 / om
    C = 0.5 * (C + np.swapaxes(C, 1, 2))
    pd = np.linalg.eigvalsh(C)[:, 0] > 0
    z = np.zeros((m, dof))
    z[pd] = np.linalg.solve(C[pd], r[pd][:, :, None])[:, :, 0]
    diag = np.diagonal(rel, axis1=1, axis2=2)
    rec = np.zeros((m, 6 + 2 * dof))
    rec[:, 0] = np.einsum("mi,mi->m", r, z)
    rec[:, 1] = (~pd).astype(float)
    rec[:, 2] = dof - np.sum(om * diag, axis=1)
    rec[:, 3] = d - tau * np.sum(diag[:, :d], axis=1)
    rec[:, 4] = np.sum(om * r * r, axis=1)
    rec[:, 5] = np.einsum("mi,mij,mj->m", z, rel, z)
    rec[:, 6:6 + dof] = r
    rec[:, 6 + dof:] = z / om
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="torus3D,sphere2500,M3500,city10000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=300)
    a = ap.parse_args()
    stats = lambda v: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v))) if len(v) else None
    for name in a.inputs.split(","):
        G = cov_bench.graph(name)
        drv = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(dpgo_amd.LOSS_NONE, True))
        for _ in range(a.iters):
            assert drv.step() == 0
        X0 = np.array(drv.X())
        del drv
        grp = dpgo_amd.NodeGroup(G, range(G.num_nodes), dpgo_amd.Options.driver(dpgo_amd.LOSS_NONE, True, max_iterations=0))
        X, pres, _ = grp.polish(X0)
        d, N, m = G.d, G.num_poses, G.num_edges
        dof = d + d * (d - 1) // 2
        point = "polished: %s after %d steps" % (dpgo_amd.POLISH_NAMES[pres.outcome], pres.steps)
        records = None
        for method in (dpgo_amd.RELY_SELINV, dpgo_amd.RELY_SOLVE):
            out = grp.edge_reliability(X, method=method)   # (analysis, allocations, code objects)
            r, fac, inv, edg, call = out["result"], [], [], [], []
            if r.outcome == dpgo_amd.RELY_OK:
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    out = grp.edge_reliability(X, method=method)
                    call.append(1e3 * (time.perf_counter() - t0))
                    r = out["result"]
                    fac.append(r.factor_ms); inv.append(r.inverse_ms); edg.append(r.edge_ms)
                if records is None:
                    records = out["records"]
            line = dict(input=name, point=point, d=d, poses=N, nodes=G.num_nodes, edges=m, method=dpgo_amd.RELY_METHOD_NAMES[method],
                        outcome=dpgo_amd.RELY_NAMES[r.outcome], unknowns=r.unknowns, fronts=r.fronts, levels=r.levels,
                        max_front=r.max_front, device_bytes_selinv=r.device_bytes_selinv, device_bytes_solve=r.device_bytes_solve,
                        columns=r.columns, batches=r.batches, factor_ms=stats(fac), inverse_ms=stats(inv), edge_ms=stats(edg),
                        call_ms=stats(call), stationarity=r.stationarity, pivot_min=r.pivot_min)
            if r.outcome == dpgo_amd.RELY_OK:
                ok = out["flag"] == 0
                line.update(flagged=r.flagged, unweighted=r.unweighted, redundancy_sum=r.redundancy_sum, cycle_dof=dof * (m - N + 1),
                            redundancy_min=float(out["redundancy"].min()), redundancy_max=float(out["redundancy"].max()),
                            d2_loo_median=float(np.median(out["d2_loo"][ok])) if ok.any() else None,
                            edge_share_of_call=float(np.median(edg) / (np.median(fac) + np.median(inv) + np.median(edg))))
            print(json.dumps(line), flush=True)
        # the route without this call: covariance with every edge as a pair, then numpy
        I, J, R, t, kappa, tau = G.edges()
        pairs = np.stack([I, J], axis=1).astype(np.int32)
        cov_ms, np_ms, rec = [], [], None
        res = grp.covariance(X, pairs=pairs)[2]
        if res.outcome == dpgo_amd.COV_OK:
            for _ in range(a.reps):
                t0 = time.perf_counter()
                marg, cross, res = grp.covariance(X, pairs=pairs)
                t1 = time.perf_counter()
                rec = numpy_records(d, N, np.asarray(X), marg, cross, I, J, R, t, kappa, tau)
                cov_ms.append(1e3 * (t1 - t0)); np_ms.append(1e3 * (time.perf_counter() - t1))
        line = dict(input=name, point=point, method="covariance + numpy", outcome=dpgo_amd.COV_NAMES[res.outcome],
                    device_bytes=res.device_bytes, covariance_ms=stats(cov_ms), covariance_numeric_ms=res.numeric_ms, numpy_ms=stats(np_ms),
                    baseline_ms=stats(np.add(cov_ms, np_ms)) if cov_ms else None)
        if rec is not None and records is not None:
            same = rec[:, 1] == records[:, 1]
            scale = np.maximum(np.abs(records), 1e-12)
            line.update(flags_differ=int((~same).sum()), max_relative_difference=float((np.abs(rec - records) / scale)[same].max()))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
