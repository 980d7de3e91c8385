"""Measurement-sensitivity benchmark: NodeGroup.sensitivity (the tangent-space Hessian written on the device, its multifrontal
factorisation, the adjoints of k upstream gradients solved in batches of 64 on the fp64 matrix cores, the per-edge kernel;
dpgo_amd/csrc/sens.cpp + sens.hip) on one GPU.

  python tools/sens_bench.py [--inputs torus3D,sphere2500,M3500,city10000] [--columns 1,16,64] [--reps 5] [--iters 300]
                             [--baseline-reps 2]

Inputs: tools/cov_bench.py's -- torus3D x 8, sphere2500 x 4, M3500 x 4 and city10000 x 8 -- each at the POLISHED point: a run of
--iters AMM-PGO# iterations (LOSS_NONE, driver options), then NodeGroup.polish.  All nodes on one GPU.  Cases: k = 1, 16 and 64
seeded dense upstream columns.

Per input and case one JSON line: the sizes of the factorisation, the predicted device bytes, the edges, and -- medians of
--reps calls after one warm-up call, on the library's host clock, each phase ending in a synchronise -- factor_ms, solve_ms per
batch (upload, right-hand sides, block solve), edge_ms (k_sens_edge and the copy of its k x m x (2 + dof) doubles to the host)
and its share of a batch.  Beside them, once per input, what there was before for ONE parameter of ONE edge: the graph rebuilt
with that parameter perturbed, a new group of it, and NodeGroup.polish from X* (baseline_ms, the median of --baseline-reps runs
on the host's clock: graph_from_edges + NodeGroup + polish) -- a central difference needs two of those per parameter, and there
are m (2 + dof) parameters; one sensitivity call with k columns gives all of them for k scalars.  Nothing here is part of
bench.py."""
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


def baseline_once(G, X, e, step):
    """One perturbed re-solve: kappa_e (1 + step), a new graph, a new group, the polish from X.  Host milliseconds."""
    I, J, R, t, kappa, tau = G.edges()
    t0 = time.perf_counter()
    kappa = kappa.copy()
    kappa[e] *= 1.0 + step
    Gp = dpgo_amd.graph_from_edges(G.d, G.num_poses, I, J, R, t, kappa, tau, G.num_nodes)
    grp = dpgo_amd.NodeGroup(Gp, range(Gp.num_nodes), dpgo_amd.Options.driver(dpgo_amd.LOSS_NONE, True, max_iterations=0))
    _, res, _ = grp.polish(X)
    ms = 1e3 * (time.perf_counter() - t0)
    return ms, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="torus3D,sphere2500,M3500,city10000")
    ap.add_argument("--columns", default="1,16,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--baseline-reps", type=int, default=2)
    a = ap.parse_args()
    med = lambda v: float(np.median(v)) if len(v) else None
    for name in a.inputs.split(","):
        G = cov_bench.graph(name)
        drv = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(dpgo_amd.LOSS_NONE, True))
        for _ in range(a.iters):
            assert drv.step() == 0
        X0 = np.array(drv.X())
        del drv
        grp = dpgo_amd.NodeGroup(G, range(G.num_nodes), dpgo_amd.Options.driver(dpgo_amd.LOSS_NONE, True, max_iterations=0))
        X, pres, _ = grp.polish(X0)
        n = (G.d + G.d * (G.d - 1) // 2) * G.num_poses
        base = [baseline_once(G, X, G.num_edges // 2, 1e-3) for _ in range(a.baseline_reps + 1)][1:]
        for k in (int(v) for v in a.columns.split(",")):
            U = np.asfortranarray(np.random.default_rng(2000 + k).standard_normal((n, k)))
            first = grp.sensitivity(X, U)[0]   # (analysis, allocations, code objects)
            r, fac, sol, edg = first, [], [], []
            if first.outcome == dpgo_amd.SENS_OK:
                for _ in range(a.reps):
                    r = grp.sensitivity(X, U)[0]
                    fac.append(r.factor_ms); sol.append(r.solve_ms); edg.append(r.edge_ms)
            line = dict(input=name, point="polished: %s after %d steps" % (dpgo_amd.POLISH_NAMES[pres.outcome], pres.steps), d=G.d,
                        poses=G.num_poses, nodes=G.num_nodes, edges=r.edges, columns=k, batches=r.batches, unknowns=r.unknowns,
                        fronts=r.fronts, levels=r.levels, max_front=r.max_front, device_bytes=r.device_bytes,
                        outcome=dpgo_amd.SENS_NAMES[r.outcome], factor_ms=med(fac), solve_ms=med(sol), edge_ms=med(edg),
                        stationarity=r.stationarity, pivot_min=r.pivot_min)
            if sol:
                line.update(solve_ms_per_batch=med(sol) / r.batches, edge_ms_per_batch=med(edg) / r.batches,
                            edge_share_of_batch=med(edg) / (med(sol) + med(edg)),
                            parameters=r.edges * (2 + r.unknowns // G.num_poses),
                            baseline_ms_per_resolve=med([b[0] for b in base]), baseline_polish_steps=base[-1][1].steps,
                            baseline_outcome=dpgo_amd.POLISH_NAMES[base[-1][1].outcome])
                line["call_ms"] = line["factor_ms"] + line["solve_ms"] + line["edge_ms"]
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
