"""Certificate-proof benchmark: NodeGroup.cert_factor (fast_verification STEP 1, the device Cholesky of S + eta I,
dpgo_amd/csrc/cert.cpp + spd_dev.hip in factor-only mode) on one GPU.

  python tools/cert_factor_bench.py [--inputs torus3D,sphere2500,M3500,city10000,headline] [--eta 1e-3] [--reps 5]
                                    [--iters 300] [--max-factor-bytes 0]

Inputs: torus3D x 8, sphere2500 x 4, M3500 x 4 and city10000 x 8, each at its chordal point and after a run of --iters
AMM-PGO# iterations (LOSS_NONE, driver options), and the headline lattice of dpgo_amd/synthetic.py (100 k poses, seed
20240817, 8 nodes) at its chordal point.  All nodes on one GPU.

Per (input, point) one JSON line: unknowns, fronts, tree levels, the largest front, factor entries and the device bytes
of the numeric phase (all predicted by the symbolic analysis, so they are there for a SKIPPED outcome too), the host
seconds of the analysis (the first call of a group), the numeric seconds (the library's host clock from the launch of
k_cert_matrix to the verdict, which ends in a synchronise; median of --reps calls after one warm-up call), the outcome,
the pivot range and the stationarity |S X|_F.  Nothing here is part of bench.py."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dpgo_amd  # noqa: E402
from dpgo_amd import synthetic  # noqa: E402

NODES = {"torus3D": 8, "sphere2500": 4, "M3500": 4, "city10000": 8}


def graph(name):
    if name == "headline":
        h = synthetic.HEADLINE
        g = synthetic.grid(h["nx"], h["ny"], h["nz"], h["num_edges"], seed=h["seed"])
        return dpgo_amd.graph_from_edges(g["d"], g["num_poses"], g["I"], g["J"], g["R"], g["t"], g["kappa"], g["tau"], 8)
    return dpgo_amd.read_g2o(os.path.join(ROOT, "fixtures", "g2o", name + ".g2o"), NODES[name])


def measure(grp, X, eta, reps, cap):
    first = grp.cert_factor(X, eta=eta, max_factor_bytes=cap)   # (the analysis, the allocations, the code objects: the warm-up)
    ts, f = [], first
    if first.outcome != dpgo_amd.CERT_FACTOR_SKIPPED:
        for _ in range(reps):
            f = grp.cert_factor(X, eta=eta, max_factor_bytes=cap)
            ts.append(f.numeric_s)
    return first, f, (float(np.median(ts)) if ts else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="torus3D,sphere2500,M3500,city10000,headline")
    ap.add_argument("--eta", type=float, default=1e-3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--max-factor-bytes", type=int, default=0)
    a = ap.parse_args()
    for name in a.inputs.split(","):
        G = graph(name)
        grp = dpgo_amd.NodeGroup(G, range(G.num_nodes), dpgo_amd.Options.driver(dpgo_amd.LOSS_NONE, True, max_iterations=0))
        points = [("chordal", np.array(G.chordal_initialization()))]
        if name != "headline" and a.iters > 0:
            drv = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(dpgo_amd.LOSS_NONE, True))
            for _ in range(a.iters):
                assert drv.step() == 0
            points.append(("after %d iterations" % a.iters, np.array(drv.X())))
            del drv
        symbolic_s = None
        for what, X in points:
            first, f, numeric_s = measure(grp, X, a.eta, a.reps, a.max_factor_bytes)
            if symbolic_s is None:
                symbolic_s = first.symbolic_s
            print(json.dumps(dict(input=name, point=what, d=G.d, poses=G.num_poses, nodes=G.num_nodes, eta=a.eta,
                                  unknowns=(G.d + 1) * G.num_poses, fronts=f.fronts, levels=f.levels, max_front=f.max_front,
                                  factor_entries=f.factor_entries, factor_bytes=f.factor_bytes, symbolic_s=symbolic_s,
                                  numeric_s=numeric_s, first_call_numeric_s=first.numeric_s,
                                  outcome=dpgo_amd.CERT_FACTOR_NAMES[f.outcome], pivot_min=f.pivot_min, pivot_max=f.pivot_max,
                                  stationarity=f.stationarity)), flush=True)


if __name__ == "__main__":
    main()
