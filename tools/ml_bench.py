"""Maximum-likelihood refinement benchmark: NodeGroup.ml_polish (dpgo_amd/csrc/ml.cpp + ml.hip under polish.cpp's loop) on one
GPU, its evaluation beside the robust objective's evaluation on the same point, and the whole refinement.

  python tools/ml_bench.py [--inputs torus3D,sphere2500,M3500,city10000] [--iters 300] [--reps 5] [--max-bytes 0] [--max-steps 50]

Inputs: torus3D x 8, sphere2500 x 4, M3500 x 4 and city10000 x 8 with the files' own information matrices, each at its
isotropic polished point: --iters AMM-PGO# iterations (trivial loss, driver options), then NodeGroup.polish.  All nodes on one
GPU.  Medians of --reps calls after one warm-up call; the library's host clocks end behind a read-back.

Per input one JSON line:
  evaluation_ms, assembly_ms, assembly_other_ms
        total_ms of ml_polish with max_steps = 0 (no factorisation is made then): the upload of X, k_ml_edge with its final
        pass, k_ml_gather, k_ml_hessian, the shift, the read-back and the download -- an upper bound of one evaluation (the
        host clocks do not separate kernels); its factor_ms (k_ml_hessian with the shift and the read-back); the rest
  robust_evaluation_ms, robust_assembly_ms, robust_assembly_other_ms
        the same figures of robust_polish (trivial loss, curvature 1, max_steps = 0) of THIS build on the same point --
        k_robust_edge, k_robust_gather, Lambda, the gradient, k_robust_mval + k_cov_hessian in their place; that code is the
        parent commit's unchanged, which is what stands in for "the parent commit's robust_hessian evaluation"
  refinement
        the result struct of ml_polish with --max-steps: outcome, steps, factorisations, F_ml and |g| at both ends, near_pi,
        total_ms and its parts
The clocks are the library's host clocks around uploads, launches and read-backs, not kernel times: the two evaluation figures
say that the passes cost the same order, not which is faster.  A report, not a gate; nothing here is part of bench.py."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dpgo_amd  # noqa: E402

NODES = {"torus3D": 8, "sphere2500": 4, "M3500": 4, "city10000": 8}
TIMES = ("total_ms", "factor_ms", "solve_ms", "other_ms")
FIELDS = ("steps", "factorisations", "indefinite", "F_initial", "F_final", "grad_initial", "grad_final", "device_bytes")


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
    return out, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="torus3D,sphere2500,M3500,city10000")
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-bytes", type=int, default=0)
    ap.add_argument("--max-steps", type=int, default=50)
    a = ap.parse_args()
    for name in a.inputs.split(","):
        nn = NODES[name]
        G = dpgo_amd.read_g2o(os.path.join(ROOT, "fixtures", "g2o", name + ".g2o"), nn)
        drv = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(dpgo_amd.LOSS_NONE, True))
        for _ in range(a.iters):
            assert drv.step() == 0
        X = np.array(drv.X())
        del drv
        grp = dpgo_amd.NodeGroup(G, range(nn), dpgo_amd.Options.driver(dpgo_amd.LOSS_NONE, True, max_iterations=0))
        X, pol, _ = grp.polish(X, max_bytes=a.max_bytes)
        line = dict(input=name, point="trivial loss, %d iterations, polish %s" % (a.iters, dpgo_amd.POLISH_NAMES[pol.outcome]), d=G.d,
                    poses=G.num_poses, edges=G.num_edges, nodes=nn)
        ev = median_run(lambda: grp.ml_polish(X, max_bytes=a.max_bytes, max_steps=0)[1], a.reps)[0]
        rb = median_run(lambda: grp.robust_polish(X, dpgo_amd.LOSS_NONE, curvature=1, max_bytes=a.max_bytes, max_steps=0)[1], a.reps)[0]
        line.update(evaluation_ms=ev["total_ms"], assembly_ms=ev["factor_ms"], assembly_other_ms=ev["other_ms"],
                    robust_evaluation_ms=rb["total_ms"], robust_assembly_ms=rb["factor_ms"], robust_assembly_other_ms=rb["other_ms"])
        ref, last = median_run(lambda: grp.ml_polish(X, max_bytes=a.max_bytes, max_steps=a.max_steps)[1], a.reps)
        ref.update(near_pi=last.near_pi, chi2_initial=last.chi2_initial, chi2_final=last.chi2_final)
        line["refinement"] = ref
        print(json.dumps(line), flush=True)
        del grp


if __name__ == "__main__":
    main()
