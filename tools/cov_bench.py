"""Marginal-covariance benchmark: NodeGroup.covariance (the tangent-space Hessian written on the device, its multifrontal
factorisation and the selected inversion on the fp64 matrix cores; dpgo_amd/csrc/cov.cpp + spd_dev.hip) on one GPU.

  python tools/cov_bench.py [--inputs torus3D,sphere2500,M3500,city10000,headline] [--reps 5] [--iters 300] [--max-bytes 0]
                            [--cpu]

Inputs: torus3D x 8, sphere2500 x 4, M3500 x 4 and city10000 x 8 after a run of --iters AMM-PGO# iterations (LOSS_NONE,
driver options), and the headline lattice of dpgo_amd/synthetic.py (100 k poses, seed 20240817, 8 nodes) at its chordal
point.  All nodes on one GPU.

Per input one JSON line: unknowns, fronts, tree levels, the largest front and the predicted device bytes (from the symbolic
analysis, so they are there for a SKIPPED outcome too), the host seconds of the analysis, and -- medians of --reps calls
after one warm-up call, on the library's host clock, each ending in a synchronise -- factor_ms (k_cov_hessian and the
factorisation up to its verdict) and selinv_ms (the selected inversion), the useful flops of its products
sum (2 u^2 w + 2 u w^2 + w^3) and their share of the 78.6 TFLOP/s fp64 matrix peak, the outcome, the pivot range and the
stationarity.  --cpu adds the only baseline there is: scipy splu of the device's own matrix (NodeGroup.cov_hessian) and one
solve per wanted column (dof N of them), or the dense inverse up to 12 000 unknowns; cpu_s is its wall time and
cpu_max_diff the largest difference of its marginals from the device's.  Nothing here is part of bench.py."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dpgo_amd  # noqa: E402
from dpgo_amd import synthetic  # noqa: E402

NODES = {"torus3D": 8, "sphere2500": 4, "M3500": 4, "city10000": 8}
PEAK_FP64_MATRIX = 78.6e12


def graph(name):
    if name == "headline":
        h = synthetic.HEADLINE
        g = synthetic.grid(h["nx"], h["ny"], h["nz"], h["num_edges"], seed=h["seed"])
        return dpgo_amd.graph_from_edges(g["d"], g["num_poses"], g["I"], g["J"], g["R"], g["t"], g["kappa"], g["tau"], 8)
    return dpgo_amd.read_g2o(os.path.join(ROOT, "fixtures", "g2o", name + ".g2o"), NODES[name])


def cpu_baseline(grp, X, dof, N):
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    ptr, col, val = grp.cov_hessian(X)
    n = dof * N
    H = sp.csc_matrix(sp.csr_matrix((val, col, ptr), shape=(n, n)))
    t0 = time.perf_counter()
    marg = np.zeros((N, dof, dof))
    if n <= 12000:
        S = np.linalg.inv(H.toarray())
        for p in range(N):
            marg[p] = S[dof * p:dof * p + dof, dof * p:dof * p + dof]
        how = "dense inverse"
    else:
        lu = spla.splu(H)
        for p in range(N):
            E = np.zeros((n, dof))
            E[dof * p + np.arange(dof), np.arange(dof)] = 1.0
            marg[p] = lu.solve(E)[dof * p:dof * p + dof]
        how = "splu + %d solves" % n
    marg[0] = 0.0
    return time.perf_counter() - t0, how, marg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="torus3D,sphere2500,M3500,city10000,headline")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--max-bytes", type=int, default=0)
    ap.add_argument("--cpu", action="store_true")
    a = ap.parse_args()
    for name in a.inputs.split(","):
        G = graph(name)
        dof = G.d + G.d * (G.d - 1) // 2
        grp = dpgo_amd.NodeGroup(G, range(G.num_nodes), dpgo_amd.Options.driver(dpgo_amd.LOSS_NONE, True, max_iterations=0))
        what, X = "chordal", np.array(G.chordal_initialization())
        if name != "headline" and a.iters > 0:
            drv = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(dpgo_amd.LOSS_NONE, True))
            for _ in range(a.iters):
                assert drv.step() == 0
            what, X = "after %d iterations" % a.iters, np.array(drv.X())
            del drv
        marg, _, first = grp.covariance(X, max_bytes=a.max_bytes)   # (the analysis, the allocations, the code objects: the warm-up)
        r, fac, inv = first, [], []
        if first.outcome != dpgo_amd.COV_SKIPPED:
            for _ in range(a.reps):
                marg, _, r = grp.covariance(X, max_bytes=a.max_bytes)
                fac.append(r.factor_ms)
                inv.append(r.selinv_ms)
        line = dict(input=name, point=what, d=G.d, poses=G.num_poses, nodes=G.num_nodes, unknowns=r.unknowns, fronts=r.fronts,
                    levels=r.levels, max_front=r.max_front, device_bytes=r.device_bytes, symbolic_s=first.symbolic_s,
                    outcome=dpgo_amd.COV_NAMES[r.outcome], factor_ms=float(np.median(fac)) if fac else None,
                    selinv_ms=float(np.median(inv)) if inv and r.outcome == dpgo_amd.COV_OK else None,
                    selinv_flops=r.selinv_flops, pivot_min=r.pivot_min, pivot_max=r.pivot_max, stationarity=r.stationarity)
        if line["selinv_ms"]:
            line["selinv_tflops"] = r.selinv_flops / (line["selinv_ms"] * 1e-3) * 1e-12
            line["share_of_fp64_matrix_peak"] = r.selinv_flops / (line["selinv_ms"] * 1e-3) / PEAK_FP64_MATRIX
        if a.cpu and r.outcome == dpgo_amd.COV_OK:
            cpu_s, how, cm = cpu_baseline(grp, X, dof, G.num_poses)
            line.update(cpu_s=cpu_s, cpu_method=how, cpu_max_diff=float(np.abs(cm - marg).max()))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
