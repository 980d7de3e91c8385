"""Edge-evaluation benchmark: dpgo_edge_eval_run (k_edge_eval + k_edge_final) at the headline lattice
(dpgo_amd.synthetic.grid(**HEADLINE): 100 000 poses, 400 000 edges, 2 % outlier closures) at its chordal point.

  python tools/edge_bench.py [--nodes 8] [--loss huber] [--reps 50]

Per run: the wall time of one call (a host clock around it: the pose records of X are rebuilt and uploaded, the two kernels
run, four arrays and the summary come back) and the device time of the two kernels from the HIP events the library records
around them (dpgo_edge_eval_kernel_ms).  Algorithmic bytes per call, counted once per operand:
  edge records   m (16 + 8 (d^2 + d + 2))         128 B per edge at d = 3
  pose records   2 m 8 (d + 1) d                  two gathers of 96 B per edge (N (d+1) d 8 if every pose were read once)
  outputs        4 m 8
and the implied share of the MI355X's 8 TB/s.  One JSON line on stdout."""
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

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=8)
    ap.add_argument("--loss", default="huber", choices=sorted(dpgo_amd.LOSS_NAMES))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--small", action="store_true", help="a 10 x 10 x 10 lattice (a functional check of the tool)")
    a = ap.parse_args()
    g = synthetic.grid(10, 10, 10, num_edges=4000) if a.small else synthetic.grid(**synthetic.HEADLINE)
    d, N, m = 3, g["num_poses"], len(g["I"])
    G = dpgo_amd.graph_from_edges(d, N, g["I"], g["J"], g["R"], g["t"], g["kappa"], g["tau"], a.nodes)
    X = np.asfortranarray(G.chordal_initialization())
    loss = dpgo_amd.LOSS_NAMES[a.loss]
    ev = dpgo_amd.EdgeEval(G)
    first = ev.run(X, loss, 0.25)            # warm-up (code object load)
    wall, kern = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        out = ev.run(X, loss, 0.25)
        wall.append(time.perf_counter() - t0)
        kern.append(ev.kernel_ms())
    same = all(np.array_equal(x, y) for x, y in zip(first[:4], out[:4])) and first[4].F == out[4].F
    k = float(np.median(kern)) * 1e-3
    by = m * (16 + 8 * (d * d + d + 2)) + 2 * m * 8 * (d + 1) * d + 4 * m * 8
    s = out[4]
    print(json.dumps(dict(poses=N, edges=m, nodes=a.nodes, loss=a.loss, call_ms=float(np.median(wall)) * 1e3,
                          kernel_us=k * 1e6, kernel_us_min=float(np.min(kern)) * 1e3, algorithmic_bytes=by,
                          bytes_per_s=by / k, share_of_8TBps=by / k / HBM_PEAK, F=s.F, num_inter=s.num_inter,
                          num_downweighted=s.num_downweighted, weight_min=s.weight_min, same_bits=bool(same))), flush=True)


if __name__ == "__main__":
    main()
