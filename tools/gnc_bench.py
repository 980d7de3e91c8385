"""Graduated non-convexity benchmark: NodeGroup.gnc (dpgo_amd/csrc/gnc.cpp + gnc.hip over polish.cpp's loop) on one GPU, beside
the same levels done by the route there was before it.

  python tools/gnc_bench.py [--inputs smallGrid3D,torus3D,sphere2500] [--kind tls] [--fraction 0.2] [--seed 0] [--iters 100]
                            [--barc2 0] [--reps 3]

Per input: the .g2o fixture on NODES[input] nodes, all on one GPU.  The start X is the trivial-loss AMM-PGO# point of the CLEAN
graph after --iters iterations.  Then --fraction of the robust-set closures (inter-node edges with |i - j| != 1, chosen with
--seed) are replaced by gross outliers: a random rotation and the translation plus 3 N(0, 1) times its own norm.  barc2 = 0
takes three times the largest robust s_e of the clean graph at X.  Medians of --reps calls after one warm-up call.

One JSON line per input:
  gnc          outcome, levels, steps (Newton steps of all inner solves), factorisations, num_zero, num_outliers, rejected_exactly
               (the zero weights are the injected outliers; TLS), and the library's clocks edge_ms, inner_ms, total_ms
  older_route  the same levels at the same mu through the older calls -- EdgeEval.run, the weights on the host
               (gnc_weight_debug), Graph.scale_edges, a new trivial-loss group, NodeGroup.polish -- wall seconds in all and per
               level, and whether it ends with the same zero weights
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
from dpgo_amd import synthetic  # noqa: E402

NODES = {"tinyGrid3D": 2, "smallGrid3D": 2, "torus3D": 8, "sphere2500": 4, "M3500": 4, "city10000": 8}


def corrupt(G, nn, robust, fraction, seed):
    """(the graph with `fraction` of the robust-set closures replaced by gross outliers, their mask)."""
    I, J, R, t, kap, tau = G.edges()
    rng = np.random.default_rng(seed)
    closures = np.nonzero(robust & (np.abs(I - J) != 1))[0]
    bad = rng.choice(closures, max(1, int(round(fraction * len(closures)))), replace=False)
    R, t = R.copy(), t.copy()
    R[bad] = synthetic._random_rotations_d(rng, len(bad), G.d)
    t[bad] += 3.0 * rng.standard_normal((len(bad), G.d)) * (1.0 + np.linalg.norm(t[bad], axis=1, keepdims=True))
    mask = np.zeros(len(I), bool)
    mask[bad] = True
    return dpgo_amd.graph_from_edges(G.d, G.num_poses, I, J, R, t, kap, tau, nn), mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="smallGrid3D,torus3D,sphere2500")
    ap.add_argument("--kind", default="tls", choices=("tls", "gm"))
    ap.add_argument("--fraction", type=float, default=0.2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--barc2", type=float, default=0.0)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    kind = dpgo_amd.GNC_TLS if a.kind == "tls" else dpgo_amd.GNC_GM
    trivial = dpgo_amd.Options.driver(dpgo_amd.LOSS_NONE, True, max_iterations=0)
    for name in a.inputs.split(","):
        nn = NODES[name]
        G = dpgo_amd.read_g2o(os.path.join(ROOT, "fixtures", "g2o", name + ".g2o"), nn)
        drv = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(dpgo_amd.LOSS_NONE, True))
        for _ in range(a.iters):
            assert drv.step() == 0
        X = np.array(drv.X())
        del drv
        clean = dpgo_amd.NodeGroup(G, range(nn), trivial)
        sr, st, w, _ = clean.gnc_eval(G, X, kind, 1.0, 1.0, w_start=np.full(G.num_edges, -1.0))
        robust = w >= 0                                       # (the pass writes its weights on the robust set only)
        barc2 = a.barc2 if a.barc2 > 0 else 3.0 * float((sr + st)[robust].max())
        del clean
        Gc, injected = corrupt(G, nn, robust, a.fraction, a.seed)
        grp = dpgo_amd.NodeGroup(Gc, range(nn), trivial)
        opt = dpgo_amd.GncOptions(kind=kind, barc2=barc2)
        out = grp.gnc(Gc, X, opt)                             # warm-up
        clocks = []
        for _ in range(a.reps):
            out = grp.gnc(Gc, X, opt)
            clocks.append((out[2].edge_ms, out[2].inner_ms, out[2].total_ms))
        Xg, wg, res, log = out
        med = np.median(np.array(clocks), axis=0)
        line = dict(input=name, kind=a.kind, d=G.d, poses=G.num_poses, edges=G.num_edges, nodes=nn, robust=int(robust.sum()),
                    injected=int(injected.sum()), barc2=barc2,
                    gnc=dict(outcome=dpgo_amd.GNC_NAMES[res.outcome], levels=res.levels, steps=res.steps, factorisations=res.factorisations,
                             num_zero=res.num_zero, num_outliers=res.num_outliers, rejected_exactly=bool(np.array_equal(wg == 0, injected)),
                             edge_ms=float(med[0]), inner_ms=float(med[1]), total_ms=float(med[2]), device_bytes=res.device_bytes))
        # the older route: the same levels, every one of them set-up
        walls = []
        for _ in range(a.reps):
            grp.sync()
            t0 = time.perf_counter()
            ev = dpgo_amd.EdgeEval(Gc)
            Xo = dpgo_amd.NodeGroup(Gc, range(nn), trivial).polish(X)[0]
            wo = np.ones(Gc.num_edges)
            for k in range(res.levels):
                s = np.add(*ev.run(Xo)[:2])
                wo = np.ones(Gc.num_edges)
                wo[robust] = dpgo_amd.gnc_weight_debug(kind, log[k, 0], barc2, s[robust])[0]
                Gw = Gc.scale_edges(wo)
                gw = dpgo_amd.NodeGroup(Gw, range(nn), trivial)
                Xo = gw.polish(Xo)[0]
                gw.sync()
                del gw, Gw
            walls.append(time.perf_counter() - t0)
        wall = float(np.median(walls))
        line["older_route"] = dict(wall_s=wall, per_level_s=wall / max(res.levels + 1, 1), same_zero_weights=bool(np.array_equal(wo == 0, wg == 0)))
        print(json.dumps(line), flush=True)
        del grp


if __name__ == "__main__":
    main()
