"""Riemannian-staircase benchmark: NodeGroup.staircase (TNT at rank r on the kernels of dpgo_amd/csrc/stair.hip and the
certificate's products, verify at the lifted point, the escape, the rounding and the polish; stair.cpp) on one GPU.

  python tools/staircase_bench.py [--inputs torus3D,sphere2500,M3500,city10000] [--iters 300] [--reps 5] [--max-bytes 0]
                                  [--polish 1]

Inputs: torus3D x 8, sphere2500 x 4, M3500 x 4 and city10000 x 8 after 300 AMM-PGO# iterations (LOSS_NONE, driver options).  All
nodes on one GPU.

Per (input, iterations) one JSON line: the result struct of the staircase -- outcome, the final certificate's status, theta and
stationarity, final_rank, levels, the TNT iterations and Hessian products, F_initial / F_sdp / F_rounded / F_final, gap, the
singular values, replaced_by_input, device_bytes -- with total_ms, optimise_ms, verify_ms and round_ms as medians of --reps
calls after one warm-up call (the library's host clock; every call starts from the same X), and the per-level log of the last
call.  A report, not a gate; nothing here is part of bench.py."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dpgo_amd  # noqa: E402

NODES = {"torus3D": 8, "sphere2500": 4, "M3500": 4, "city10000": 8}
TIMES = ("total_ms", "optimise_ms", "verify_ms", "round_ms")
LOG = ("rank", "F_in", "F_out", "grad", "tnt_iterations", "hess_products", "cert_status", "theta", "alpha", "halvings")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="torus3D,sphere2500,M3500,city10000")
    ap.add_argument("--iters", default="300")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-bytes", type=int, default=0)
    ap.add_argument("--polish", type=int, default=1)
    a = ap.parse_args()
    for name in a.inputs.split(","):
        nn = NODES[name]
        G = dpgo_amd.read_g2o(os.path.join(ROOT, "fixtures", "g2o", name + ".g2o"), nn)
        grp = dpgo_amd.NodeGroup(G, range(nn), dpgo_amd.Options.driver(dpgo_amd.LOSS_NONE, True, max_iterations=0))
        drv = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(dpgo_amd.LOSS_NONE, True))
        done = 0
        for iters in sorted(int(v) for v in a.iters.split(",")):
            for _ in range(iters - done):
                assert drv.step() == 0
            done = iters
            X = np.array(drv.X())
            _, first, log, _ = grp.staircase(X, max_bytes=a.max_bytes, polish=a.polish)   # (allocations, code objects: the warm-up)
            r, times = first, {t: [] for t in TIMES}
            if first.outcome != dpgo_amd.STAIR_SKIPPED:
                for _ in range(a.reps):
                    _, r, log, _ = grp.staircase(X, max_bytes=a.max_bytes, polish=a.polish)
                    for t in TIMES:
                        times[t].append(getattr(r, t))
            line = dict(input=name, point="after %d iterations" % iters, d=G.d, poses=G.num_poses, nodes=nn,
                        outcome=dpgo_amd.STAIR_NAMES[r.outcome], cert_status=dpgo_amd.CERT_NAMES[r.cert_status])
            for f, _ in dpgo_amd.StaircaseResult._fields_:
                if f == "sigma":
                    line[f] = list(r.sigma[:2 * G.d])
                elif f not in ("outcome", "cert_status") + TIMES:
                    line[f] = getattr(r, f)
            for t in TIMES:
                line[t] = float(np.median(times[t])) if times[t] else None
            line["levels_log"] = [dict(zip(LOG, row.tolist())) for row in log]
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
