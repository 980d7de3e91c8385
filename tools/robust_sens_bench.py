"""Benchmark of the robust objective's sensitivities: NodeGroup.robust_sensitivity (the robust edge pass, the TRUE robust
Hessian written on the device, its factorisation, the adjoints in batches of 64, the per-edge preparation pass and the
per-edge kernel; dpgo_amd/csrc/rsens.cpp + rsens.hip) beside NodeGroup.sensitivity on the same group, graph and point, phase by
phase, on one GPU.

  python tools/robust_sens_bench.py [--inputs torus3D,sphere2500,M3500,city10000] [--columns 1,16,64] [--reps 5] [--iters 300]
                                    [--loss huber|gm|welsch]

Inputs: tools/sens_bench.py's -- torus3D x 8, sphere2500 x 4, M3500 x 4 and city10000 x 8 -- each at the ROBUST-POLISHED point:
a run of --iters AMM-PGO# iterations with the loss (driver options), then NodeGroup.robust_polish with the driver's loss_reg on a
trivial-loss group of the same graph.  All nodes on one GPU.

Per input and case one JSON line: the sizes, the predicted device bytes of both calls, and -- medians of --reps calls after one
warm-up call, on the library's host clock, each phase ending in a synchronise -- for the robust call factor_ms (M_w, k_cov_hessian,
the rank-one terms, the factorisation), solve_ms, edge_ms (k_rsens_prep once, k_rsens_edge and the copy of k x m x (3 + dof)
doubles per batch, the host's sum for dloss_reg) and call_ms on the host's clock around the whole call (which also holds the
robust edge pass, the gather and the stationarity in front of the factorisation); for NodeGroup.sensitivity at the same point
the same three phases (its H is that of the trivial loss: the numbers it returns there mean nothing, its cost is the parent's).
Nothing here is part of bench.py."""
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

LOSSES = {"huber": dpgo_amd.LOSS_HUBER, "gm": dpgo_amd.LOSS_GM, "welsch": dpgo_amd.LOSS_WELSCH}


def timed(call, reps):
    """Medians of the three phases and of the host's clock around the call, after one warm-up call."""
    first = call()[0]
    fac, sol, edg, wall, r = [], [], [], [], first
    if first.outcome == dpgo_amd.SENS_OK:
        for _ in range(reps):
            t0 = time.perf_counter()
            r = call()[0]
            wall.append(1e3 * (time.perf_counter() - t0))
            fac.append(r.factor_ms); sol.append(r.solve_ms); edg.append(r.edge_ms)
    med = lambda v: float(np.median(v)) if len(v) else None
    return r, dict(factor_ms=med(fac), solve_ms=med(sol), edge_ms=med(edg), call_ms=med(wall))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="torus3D,sphere2500,M3500,city10000")
    ap.add_argument("--columns", default="1,16,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--loss", default="huber", choices=sorted(LOSSES))
    a = ap.parse_args()
    loss = LOSSES[a.loss]
    for name in a.inputs.split(","):
        G = cov_bench.graph(name)
        opt = dpgo_amd.Options.driver(loss, True)
        drv = dpgo_amd.DistPGO(G, opt)
        for _ in range(a.iters):
            assert drv.step() == 0
        X0 = np.array(drv.X())
        del drv
        grp = dpgo_amd.NodeGroup(G, range(G.num_nodes), dpgo_amd.Options.driver(dpgo_amd.LOSS_NONE, True, max_iterations=0))
        X, pres, _, sm = grp.robust_polish(X0, loss, opt.loss_reg)
        n = (G.d + G.d * (G.d - 1) // 2) * G.num_poses
        for k in (int(v) for v in a.columns.split(",")):
            U = np.asfortranarray(np.random.default_rng(2000 + k).standard_normal((n, k)))
            r, rob = timed(lambda: grp.robust_sensitivity(X, U, loss, opt.loss_reg), a.reps)
            p, plain = timed(lambda: grp.sensitivity(X, U), a.reps)
            line = dict(input=name, loss=a.loss, loss_reg=opt.loss_reg,
                        point="robust-polished: %s after %d steps" % (dpgo_amd.POLISH_NAMES[pres.outcome], pres.steps), d=G.d,
                        poses=G.num_poses, nodes=G.num_nodes, edges=r.edges, inter=sm.num_inter, downweighted=sm.num_downweighted,
                        columns=k, batches=r.batches, unknowns=r.unknowns, fronts=r.fronts, device_bytes=r.device_bytes,
                        plain_device_bytes=p.device_bytes, outcome=dpgo_amd.SENS_NAMES[r.outcome], plain_outcome=dpgo_amd.SENS_NAMES[p.outcome],
                        stationarity=r.stationarity, pivot_min=r.pivot_min, robust=rob, plain=plain)
            if rob["edge_ms"] and plain["edge_ms"]:
                line.update(edge_ratio=rob["edge_ms"] / plain["edge_ms"], factor_ratio=rob["factor_ms"] / plain["factor_ms"],
                            solve_ratio=rob["solve_ms"] / plain["solve_ms"], call_ratio=rob["call_ms"] / plain["call_ms"],
                            in_front_ms=rob["call_ms"] - rob["factor_ms"] - rob["solve_ms"] - rob["edge_ms"])
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
