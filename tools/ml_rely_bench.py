"""ML edge-reliability benchmark: NodeGroup.ml_edge_reliability (dpgo_amd/csrc/ml_rely.cpp, ml_rely.hip) of EVERY edge of a
graph on one GPU, under both methods, beside NodeGroup.edge_reliability of the same graph -- and NodeGroup.ml_pair_gate with
every edge as its own candidate beside NodeGroup.pair_covariance's gate.

  python tools/ml_rely_bench.py [--inputs torus3D,sphere2500,M3500,city10000] [--reps 5] [--iters 300] [--max-steps 50]

Inputs: tools/ml_bench.py's -- torus3D x 8, sphere2500 x 4, M3500 x 4 and city10000 x 8 with the files' own information
matrices.  The chordal calls run at the isotropic polished point (--iters AMM-PGO# iterations, then NodeGroup.polish), the ML
calls at the point NodeGroup.ml_polish reaches from it.  All nodes on one GPU.

Per input, call and method one JSON line: the sizes of the factorisation, the bytes either method predicts, and -- after one
warm-up call, over --reps calls on the library's host clock, each phase ending in a synchronise -- the medians of factor_ms,
inverse_ms (or solve_ms) and edge_ms (or gate_ms), the median of the whole call on the caller's clock, the flagged edges, the sum
of the redundancies against dof (m - N + 1), the median d2_loo (or d2).  The clocks are host clocks around launches and
read-backs, not kernel times.  A report, not a gate; no speed claim is made from it, and nothing here is part of bench.py.
No number taken yet."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dpgo_amd  # noqa: E402

NODES = {"torus3D": 8, "sphere2500": 4, "M3500": 4, "city10000": 8}


def timed(call, reps, clocks):
    """(the last output, the medians of the result's clocks and of the caller's clock) of `reps` calls after one warm-up call."""
    out = call()
    times = {c: [] for c in clocks + ("call_ms",)}
    if out["result"].outcome == 0:
        for _ in range(reps):
            t0 = time.perf_counter()
            out = call()
            times["call_ms"].append(1e3 * (time.perf_counter() - t0))
            for c in clocks:
                times[c].append(getattr(out["result"], c))
    return out, {c: float(np.median(v)) if v else None for c, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="torus3D,sphere2500,M3500,city10000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--max-steps", type=int, default=50)
    a = ap.parse_args()
    for name in a.inputs.split(","):
        nn = NODES[name]
        G = dpgo_amd.read_g2o(os.path.join(ROOT, "fixtures", "g2o", name + ".g2o"), nn)
        drv = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(dpgo_amd.LOSS_NONE, True))
        for _ in range(a.iters):
            assert drv.step() == 0
        X0 = np.array(drv.X())
        del drv
        grp = dpgo_amd.NodeGroup(G, range(nn), dpgo_amd.Options.driver(dpgo_amd.LOSS_NONE, True, max_iterations=0))
        Xp, pres, _ = grp.polish(X0)
        Xm, mres, _ = grp.ml_polish(Xp, max_steps=a.max_steps)
        d, N, m = G.d, G.num_poses, G.num_edges
        dof = d + d * (d - 1) // 2
        head = dict(input=name, d=d, poses=N, nodes=nn, edges=m, polish=dpgo_amd.POLISH_NAMES[pres.outcome],
                    ml_polish=dpgo_amd.POLISH_NAMES[mres.polish.outcome], cycle_dof=dof * (m - N + 1))
        for label, call, X in (("ml_edge_reliability", grp.ml_edge_reliability, Xm), ("edge_reliability", grp.edge_reliability, Xp)):
            for method in (dpgo_amd.RELY_SELINV, dpgo_amd.RELY_SOLVE):
                out, t = timed(lambda: call(X, method=method), a.reps, ("factor_ms", "inverse_ms", "edge_ms"))
                r = out["result"]
                line = dict(head, call=label, method=dpgo_amd.RELY_METHOD_NAMES[method], outcome=dpgo_amd.RELY_NAMES[r.outcome],
                            unknowns=r.unknowns, fronts=r.fronts, levels=r.levels, max_front=r.max_front,
                            device_bytes_selinv=r.device_bytes_selinv, device_bytes_solve=r.device_bytes_solve, columns=r.columns,
                            batches=r.batches, stationarity=r.stationarity, pivot_min=r.pivot_min, **t)
                if r.outcome == dpgo_amd.RELY_OK:
                    ok = out["flag"] == 0
                    line.update(flagged=r.flagged, unweighted=r.unweighted, redundancy_sum=r.redundancy_sum,
                                d2_loo_median=float(np.median(out["d2_loo"][ok])) if ok.any() else None)
                print(json.dumps(line), flush=True)
        I, J, R, t, kappa, tau = G.edges()
        pairs = np.stack([I, J], axis=1).astype(np.int32)
        info = G.edge_information()[0]
        for label, call in (("ml_pair_gate", lambda: grp.ml_pair_gate(Xm, pairs, (R, t, info))),
                            ("pair_covariance", lambda: grp.pair_covariance(Xp, pairs, candidates=(R, t, kappa, tau)))):
            out, tm = timed(call, a.reps, ("factor_ms", "solve_ms", "gate_ms"))
            r = out["result"]
            line = dict(head, call=label, outcome=dpgo_amd.PAIRS_NAMES[r.outcome] if hasattr(dpgo_amd, "PAIRS_NAMES") else r.outcome,
                        device_bytes=r.device_bytes, columns=r.columns, batches=r.batches, stationarity=r.stationarity, **tm)
            if r.outcome == dpgo_amd.PAIRS_OK:
                line.update(not_pd=int(out["not_pd"].sum()), d2_median=float(np.median(out["d2"])))
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
