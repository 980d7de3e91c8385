"""Robust-polish benchmark: NodeGroup.robust_polish (dpgo_amd/csrc/robust.cpp + robust.hip under polish.cpp's loop) on one GPU,
with the true Hessian (curvature 1) and the re-weighted one (curvature 0), beside the Hessian assembly alone and beside one
outer step of the route there was before it.

  python tools/robust_polish_bench.py [--inputs torus3D,sphere2500,M3500,city10000] [--iters 300] [--reps 5] [--max-bytes 0]

Inputs: torus3D x 8, sphere2500 x 4, M3500 x 4 and city10000 x 8, each at its Huber (driver options, loss_reg 0.25) AMM-PGO#
point after --iters iterations.  All nodes on one GPU.  Medians of --reps calls after one warm-up call; every timed section
ends in a synchronise (the library's host clocks end behind a read-back; the outer step's clock behind group.sync()).

Per input one JSON line:
  curvature1 / curvature0   the result struct of robust_polish: outcome, steps, factorisations, indefinite, F and |g| at both
                            ends, total_ms and its parts
  evaluation_ms             total_ms of robust_polish with max_steps = 0 (no factorisation is made then): the upload of X,
                            k_robust_edge, k_robust_gather, Lambda, the gradient, k_robust_mval + k_cov_hessian +
                            k_robust_rank1, the shift, the read-back and the download -- an upper bound of the Hessian assembly
                            (the host clocks do not separate kernels); assembly_ms: its factor_ms, the three Hessian kernels
                            with the shift and the read-back; assembly_other_ms: the rest
  cov_evaluation_ms, cov_hessian_ms, cov_hessian_other_ms
                            the same figures of NodeGroup.polish with max_steps = 0 on the same graph (cert_apply_M and
                            k_cov_hessian alone in their place)
  factorisation_ms          (factor_ms - assembly) / factorisations of the curvature-1 run: what one factorisation costs
  outer_step                one step of an IRLS loop built from the older calls: EdgeEval.run, Graph.scale_edges, a new
                            trivial-loss group of the scaled graph, NodeGroup.polish with max_steps = 1 -- wall seconds and
                            the parts
A report, not a gate; nothing here is part of bench.py."""
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
TIMES = ("total_ms", "factor_ms", "solve_ms", "other_ms")
FIELDS = ("steps", "factorisations", "indefinite", "F_initial", "F_final", "grad_initial", "grad_final", "device_bytes")
HUBER = dpgo_amd.LOSS_HUBER


def median_run(call, reps):
    """(the last result struct, medians of its clocks) of `reps` calls after one warm-up call."""
    r = call()
    times = {t: [] for t in TIMES}
    if r.outcome != dpgo_amd.POLISH_SKIPPED:
        for _ in range(reps):
            r = call()
            for t in TIMES:
                times[t].append(getattr(r, t))
    out = dict(outcome=dpgo_amd.POLISH_NAMES[r.outcome])
    out.update({f: getattr(r, f) for f in FIELDS})
    out.update({t: float(np.median(v)) if v else None for t, v in times.items()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="torus3D,sphere2500,M3500,city10000")
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-bytes", type=int, default=0)
    a = ap.parse_args()
    for name in a.inputs.split(","):
        nn = NODES[name]
        G = dpgo_amd.read_g2o(os.path.join(ROOT, "fixtures", "g2o", name + ".g2o"), nn)
        opt = dpgo_amd.Options.driver(HUBER, True)
        dl = opt.loss_reg
        drv = dpgo_amd.DistPGO(G, opt)
        for _ in range(a.iters):
            assert drv.step() == 0
        X = np.array(drv.X())
        del drv
        trivial = dpgo_amd.Options.driver(dpgo_amd.LOSS_NONE, True, max_iterations=0)
        grp = dpgo_amd.NodeGroup(G, range(nn), trivial)
        line = dict(input=name, point="Huber, after %d iterations" % a.iters, d=G.d, poses=G.num_poses, edges=G.num_edges, nodes=nn)
        for curv in (1, 0):
            line["curvature%d" % curv] = median_run(
                lambda: grp.robust_polish(X, HUBER, dl, curvature=curv, max_bytes=a.max_bytes)[1], a.reps)
        asm = median_run(lambda: grp.robust_polish(X, HUBER, dl, curvature=1, max_bytes=a.max_bytes, max_steps=0)[1], a.reps)
        cov = median_run(lambda: grp.polish(X, max_bytes=a.max_bytes, max_steps=0)[1], a.reps)
        line.update(evaluation_ms=asm["total_ms"], cov_evaluation_ms=cov["total_ms"], assembly_ms=asm["factor_ms"], assembly_other_ms=asm["other_ms"], cov_hessian_ms=cov["factor_ms"],
                    cov_hessian_other_ms=cov["other_ms"])
        c1 = line["curvature1"]
        if c1["factor_ms"] is not None and c1["factorisations"]:
            line["factorisation_ms"] = (c1["factor_ms"] - (c1["steps"] + 1) * asm["factor_ms"]) / c1["factorisations"]
        # one outer step of the older route (every call of it is set-up: nothing to warm up but the code objects, which the
        # runs above have loaded)
        outer = []
        for _ in range(a.reps):
            grp.sync()
            t0 = time.perf_counter()
            w = dpgo_amd.EdgeEval(G).run(X, HUBER, dl)[3]
            t1 = time.perf_counter()
            Gw = G.scale_edges(w)
            t2 = time.perf_counter()
            gw = dpgo_amd.NodeGroup(Gw, range(nn), trivial)
            gw.sync()
            t3 = time.perf_counter()
            r = gw.polish(X, max_bytes=a.max_bytes, max_steps=1)[1]
            gw.sync()
            t4 = time.perf_counter()
            outer.append((t4 - t0, t1 - t0, t2 - t1, t3 - t2, t4 - t3))
            del gw, Gw
        med = np.median(np.array(outer), axis=0)
        line["outer_step"] = dict(wall_s=float(med[0]), edge_eval_s=float(med[1]), scale_edges_s=float(med[2]), new_group_s=float(med[3]),
                                  polish_one_step_s=float(med[4]), outcome=dpgo_amd.POLISH_NAMES[r.outcome])
        print(json.dumps(line), flush=True)
        del grp


if __name__ == "__main__":
    main()
