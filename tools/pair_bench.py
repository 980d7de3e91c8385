"""Pair-covariance benchmark: NodeGroup.pair_covariance (the tangent-space Hessian written on the device, its multifrontal
factorisation, the unit columns of the poses asked for solved in batches of 64 on the fp64 matrix cores; dpgo_amd/csrc/pairs.cpp
+ spd_dev.hip: spd_msolve_device) on one GPU.

  python tools/pair_bench.py [--inputs torus3D,sphere2500,M3500,city10000,headline] [--pairs 1,16,64] [--reps 5] [--iters 300]
                             [--max-bytes 0]

Inputs: tools/cov_bench.py's -- torus3D x 8, sphere2500 x 4, M3500 x 4 and city10000 x 8 after a run of --iters AMM-PGO#
iterations (LOSS_NONE, driver options), the headline lattice of dpgo_amd/synthetic.py at its chordal point.  All nodes on one
GPU.  Cases: 16 and 64 seeded random pairs of distinct poses (so up to 2 dof columns per pair), and one pair: 2 dof <= 16
columns, the narrowest batch.

Per input and case one JSON line: the sizes of the factorisation, the predicted device bytes of this path and of
NodeGroup.covariance (and whether that one is SKIPPED), the columns and batches, and -- medians of --reps calls after one
warm-up call, on the library's host clock, each ending in a synchronise -- factor_ms, solve_ms in total and per batch, gate_ms,
the useful flops of the solves sum 4 (w + u) w kb against the 78.6 TFLOP/s fp64 matrix peak, the factor bytes they stream
(16 sum (w + u) w per batch) against the 8 TB/s of HBM.  Beside them the only thing there was before: the same number of columns
solved one at a time with the single-vector device solve on the same factor (vsolve_ms, dpgo_debug_pairs_vsolve_baseline).
Nothing here is part of bench.py."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import dpgo_amd  # noqa: E402
import cov_bench  # noqa: E402  (its inputs)

PEAK_FP64_MATRIX = 78.6e12
PEAK_HBM = 8.0e12


def vsolve_baseline(grp, X, ncols):
    Xf = np.asfortranarray(X, np.float64)
    ms = C.c_double(0)
    rc = dpgo_amd.lib().dpgo_debug_pairs_vsolve_baseline(grp._h, Xf.ctypes.data_as(C.POINTER(C.c_double)), Xf.shape[0], 0, int(ncols),
                                                         C.byref(ms))
    return ms.value if rc == 0 else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="torus3D,sphere2500,M3500,city10000,headline")
    ap.add_argument("--pairs", default="1,16,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--max-bytes", type=int, default=0)
    a = ap.parse_args()
    for name in a.inputs.split(","):
        G = cov_bench.graph(name)
        grp = dpgo_amd.NodeGroup(G, range(G.num_nodes), dpgo_amd.Options.driver(dpgo_amd.LOSS_NONE, True, max_iterations=0))
        what, X = "chordal", np.array(G.chordal_initialization())
        if name != "headline" and a.iters > 0:
            drv = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(dpgo_amd.LOSS_NONE, True))
            for _ in range(a.iters):
                assert drv.step() == 0
            what, X = "after %d iterations" % a.iters, np.array(drv.X())
            del drv
        cov = grp.covariance(X, max_bytes=1)[2]   # (the prediction alone)
        for npairs in (int(v) for v in a.pairs.split(",")):
            rng = np.random.default_rng(1000 + npairs)
            pairs = np.stack([rng.choice(np.arange(1, G.num_poses), 2, replace=False) for _ in range(npairs)])
            first = grp.pair_covariance(X, pairs, max_bytes=a.max_bytes)["result"]   # (analysis, allocations, code objects)
            r, fac, sol, gat = first, [], [], []
            if first.outcome != dpgo_amd.PAIRS_SKIPPED:
                for _ in range(a.reps):
                    r = grp.pair_covariance(X, pairs, max_bytes=a.max_bytes)["result"]
                    fac.append(r.factor_ms); sol.append(r.solve_ms); gat.append(r.gate_ms)
            med = lambda v: float(np.median(v)) if v else None
            line = dict(input=name, point=what, d=G.d, poses=G.num_poses, nodes=G.num_nodes, pairs=npairs, unknowns=r.unknowns,
                        fronts=r.fronts, levels=r.levels, max_front=r.max_front, device_bytes=r.device_bytes,
                        covariance_device_bytes=cov.device_bytes, symbolic_s=first.symbolic_s, outcome=dpgo_amd.PAIRS_NAMES[r.outcome],
                        columns=r.columns, batches=r.batches, factor_ms=med(fac), gate_ms=med(gat),
                        solve_ms=med(sol) if r.outcome == dpgo_amd.PAIRS_OK else None, solve_flops=r.solve_flops,
                        factor_bytes=r.factor_bytes, pivot_min=r.pivot_min, pivot_max=r.pivot_max, stationarity=r.stationarity)
            if line["solve_ms"]:
                s = line["solve_ms"] * 1e-3
                line.update(solve_ms_per_batch=line["solve_ms"] / r.batches, solve_tflops=r.solve_flops / s * 1e-12,
                            share_of_fp64_matrix_peak=r.solve_flops / s / PEAK_FP64_MATRIX,
                            factor_tb_per_s=r.factor_bytes / s * 1e-12, share_of_hbm_peak=r.factor_bytes / s / PEAK_HBM)
                vs = [vsolve_baseline(grp, X, r.columns) for _ in range(a.reps + 1)][1:]
                if all(v is not None for v in vs):
                    line.update(vsolve_ms=med(vs), vsolve_ms_per_16=med(vs) * 16 / r.columns, speedup=med(vs) / line["solve_ms"])
            print(json.dumps(line), flush=True)
        # does this path run where covariance is refused?  a limit between the two predictions
        lim = (first.device_bytes + cov.device_bytes) // 2 if first.device_bytes < cov.device_bytes else 0
        if lim:
            c2 = grp.covariance(X, max_bytes=lim)[2]
            p2 = grp.pair_covariance(X, pairs, max_bytes=lim)["result"]
            print(json.dumps(dict(input=name, max_bytes=lim, covariance=dpgo_amd.COV_NAMES[c2.outcome],
                                  pair_covariance=dpgo_amd.PAIRS_NAMES[p2.outcome])), flush=True)


if __name__ == "__main__":
    main()
