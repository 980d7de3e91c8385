"""Newton-polish benchmark: NodeGroup.polish (the tangent gradient, the Hessian and its shift written on the device, the
multifrontal factorisation, the vector solve on its W / WT and the retraction; dpgo_amd/csrc/polish.cpp + polish.hip +
spd_dev.hip) on one GPU, beside what the first-order loop needs to reach the same gradient.

  python tools/polish_bench.py [--inputs torus3D,sphere2500,M3500,city10000] [--iters 50,300] [--reps 5]
                               [--amm-max 2000] [--amm-block 10] [--max-bytes 0]

Inputs: torus3D x 8, sphere2500 x 4, M3500 x 4 and city10000 x 8, each after 50 and after 300 AMM-PGO# iterations (LOSS_NONE,
driver options).  All nodes on one GPU.

Per (input, iterations) one JSON line: the result struct of the polish -- outcome, steps, factorisations, indefinite, F and |g|
at both ends, hmax, mu_final, the pivot range, the tree's sizes and the predicted device bytes, symbolic_s -- with total_ms,
factor_ms, solve_ms and other_ms as medians of --reps calls after one warm-up call (the library's host clock; every call
starts from the same X).  Beside it, from the unchanged first-order loop: a fresh driver started AT that point (its
acceleration state begins anew there; the driver that produced the point goes on to the next row), stepped in blocks of
--amm-block iterations with one look at the nodes' results per block, until its own gradient norm is at or below the target,
or "not reached in <amm-max>".  amm_iterations is therefore a multiple of the block, and amm_wall_s holds one host read-back
per block, not per iteration.  The target is the loop's own norm -- sqrt(sum of the nodes' gradFnorm^2), the Riemannian norm
|grad F| -- evaluated by such a driver at the POLISHED point (amm_grad_target), not the polish's grad_final: that one is the
norm of the anchored tangent-basis coefficients, whose rotation generators have norm sqrt(2) and which leaves the anchor's
entries out, so the two agree only up to such factors.  A report, not a gate; nothing here is part of bench.py."""
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


def grad_norm(drv, nn):
    return float(np.sqrt(sum(drv.group.results(a).gradFnorm ** 2 for a in range(nn))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="torus3D,sphere2500,M3500,city10000")
    ap.add_argument("--iters", default="50,300")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--amm-max", type=int, default=2000)
    ap.add_argument("--amm-block", type=int, default=10)
    ap.add_argument("--max-bytes", type=int, default=0)
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
            _, first, _ = grp.polish(X, max_bytes=a.max_bytes)   # (the analysis, the allocations, the code objects: the warm-up)
            r, times = first, {t: [] for t in TIMES}
            if first.outcome != dpgo_amd.POLISH_SKIPPED:
                for _ in range(a.reps):
                    _, r, _ = grp.polish(X, max_bytes=a.max_bytes)
                    for t in TIMES:
                        times[t].append(getattr(r, t))
            line = dict(input=name, point="after %d iterations" % iters, d=G.d, poses=G.num_poses, nodes=nn,
                        outcome=dpgo_amd.POLISH_NAMES[r.outcome], symbolic_s=first.symbolic_s)
            for f, _ in dpgo_amd.PolishResult._fields_:
                if f not in ("outcome", "symbolic_s") + TIMES:
                    line[f] = getattr(r, f)
            for t in TIMES:
                line[t] = float(np.median(times[t])) if times[t] else None
            if r.outcome != dpgo_amd.POLISH_SKIPPED:
                Xp = grp.polish(X, max_bytes=a.max_bytes)[0]
                at = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(dpgo_amd.LOSS_NONE, True), X0=Xp)
                target = grad_norm(at, nn)
                del at
                amm = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(dpgo_amd.LOSS_NONE, True), X0=X)
                line.update(amm_grad_start=grad_norm(amm, nn), amm_grad_target=target)
                amm.group.sync()
                t0, its, now = time.perf_counter(), 0, grad_norm(amm, nn)
                while now > target and its < a.amm_max:
                    for _ in range(a.amm_block):
                        assert amm.step() == 0
                    its += a.amm_block
                    now = grad_norm(amm, nn)
                amm.group.sync()
                line.update(amm_iterations=its if now <= target else "not reached in %d" % a.amm_max,
                            amm_wall_s=time.perf_counter() - t0, amm_grad_end=now)
                del amm
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
