"""PCM benchmark: dpgo_pcm_update (device pairwise consistency, k_pcm_pairs) and the two host max-clique solvers on a
seeded two-node graph with m inter-node edges (dpgo_amd.synthetic.two_node, 10 % outliers, low noise).

  python tools/pcm_bench.py [--sizes 2500,8192,16384] [--reps 20] [--trace kernel_trace.csv]

Per size: the wall time of one update (a host clock around the call, which ends in a device synchronise: record
upload + kernel + bit-row download), pairs per second, the solvers' wall times, and for m = 2500 the numpy
restatement's time for scale.  Kernel time comes from a separate profiler run: with --trace the kernel trace (CSV or .db) of
`rocprofv3 --kernel-trace --stats -d DIR -o pcm -- python tools/pcm_bench.py` gives each size's median k_pcm_pairs
duration, and the achieved fp64 FLOP/s from the FLOP count below.  One JSON line per size on stdout."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dpgo_amd  # noqa: E402
from dpgo_amd import synthetic  # noqa: E402

FP64_PEAK = 78.6e12   # MI355X vector fp64, AMD's published peak


def flops_per_pair(d):
    """fp64 operations of one pair in the reference's form (PCM.cpp:210-228), a multiply-add counted as 2:
    five d x d products, five matrix-vector products with their vector sums, the two differences and the norm."""
    prod = 2 * d ** 3
    matvec = 2 * d * d
    return 5 * prod + 5 * matvec + 3 * d + 2 * d + 2 * d * d + 2 * d + 6


def kernel_ms_from_trace(path):
    """{rows of the launch grid: [durations in ms]} of the k_pcm_pairs dispatches of a rocprofv3 kernel trace (the
    kernel_trace CSV, or the SQLite database rocprofv3 writes by default)."""
    out = {}
    if path.endswith(".db"):
        import sqlite3
        con = sqlite3.connect(path)
        for name, gy, t0, t1 in con.execute("select name, grid_y, start, end from kernels"):
            if "k_pcm_pairs" in str(name):
                out.setdefault(int(gy), []).append((t1 - t0) * 1e-6)
        return out
    with open(path) as fh:
        for row in csv.DictReader(fh):
            if "k_pcm_pairs" not in row.get("Kernel_Name", ""):
                continue
            gy = int(row.get("Grid_Size_Y") or row.get("Grid_Y") or 0)
            out.setdefault(gy, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2500,8192,16384")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace", default=None)
    ap.add_argument("--no-restatement", action="store_true")
    a = ap.parse_args()
    traced = kernel_ms_from_trace(a.trace) if a.trace else {}
    pcm = dpgo_amd.PCM()
    for m in [int(s) for s in a.sizes.split(",")]:
        g = synthetic.two_node(m, poses_per_node=1024, seed=m, sigma_t=0.01, sigma_r=1e-3, outlier_frac=0.1)
        G = dpgo_amd.graph_from_edges(3, g["num_poses"], g["I"], g["J"], g["R"], g["t"], g["kappa"], g["tau"], 2)
        X = synthetic.global_X(g["Rg"], g["tg"])
        assert pcm.update(G, 0, 1, X) == m          # warm-up (code object load, buffers)
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            pcm.update(G, 0, 1, X)
            ts.append(time.perf_counter() - t0)
        upd = float(np.median(ts))
        t0 = time.perf_counter()
        ex = pcm.solve_exact()
        t_ex = time.perf_counter() - t0
        t0 = time.perf_counter()
        he = pcm.solve_heuristic()
        t_he = time.perf_counter() - t0
        ids = pcm.measurements()
        out = g["outlier"][ids]
        pairs = float(m) * (m - 1)
        flops = pairs * flops_per_pair(3)
        res = dict(m=m, update_ms=upd * 1e3, pairs=pairs, pairs_per_s_update=pairs / upd, flop=flops,
                   solve_exact_ms=t_ex * 1e3, solve_heuristic_ms=t_he * 1e3, clique_exact=int(ex.sum()),
                   clique_heuristic=int(he.sum()), inliers=int((~out).sum()),
                   exact_is_inlier_set=bool((ex == ~out).all()))
        ks = traced.get((m + 31) // 32)
        if ks:
            k = float(np.median(ks))
            res.update(kernel_ms=k, pairs_per_s_kernel=pairs / (k * 1e-3), fp64_flops=flops / (k * 1e-3),
                       fp64_share_of_peak=flops / (k * 1e-3) / FP64_PEAK)
        if m == 2500 and not a.no_restatement:
            import pcm_restatement as pr
            I, J, R, t, kap, tau = G.edges()
            t0 = time.perf_counter()
            _, A_ref, _ = pr.update(0, 1, I, J, R, t, kap, tau, dpgo_amd.pose_nodes(G), X)
            res["numpy_restatement_ms"] = (time.perf_counter() - t0) * 1e3
            res["matches_restatement"] = bool((A_ref == pcm.adjacency()).all())
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
