"""Benchmark of graduated non-convexity on the full information matrices: NodeGroup.ml_gnc (dpgo_amd/csrc/ml_gnc.cpp +
ml_gnc.hip over polish.cpp's loop) on one GPU, beside the same levels done by the only route there was before it.

  python tools/ml_gnc_bench.py [--inputs torus3D,sphere2500,M3500,city10000] [--kind tls] [--fraction 0.2] [--seed 0]
                               [--iters 100] [--barc2 0] [--reps 3]

Per input: the .g2o fixture on NODES[input] nodes, all on one GPU, with the file's own information matrices.  The start X is the
isotropic polished point of the CLEAN graph: --iters trivial-loss AMM-PGO# iterations, then NodeGroup.polish.  Then --fraction of
the inter-node closures (|i - j| != 1, chosen with --seed) are replaced by gross outliers as tools/gnc_bench.py does it: a
random rotation and the translation plus 3 N(0, 1) times (1 + its own norm); their Omega is kept.  barc2 = 0 takes the chi2_dof
quantile at 0.999 (16.266 for d = 2, 22.458 for d = 3).  Host clocks (time.perf_counter around the call, the group synchronised),
medians of --reps calls, no warm-up call.

One JSON line per input:
  ml_gnc       outcome, levels, steps, factorisations, num_zero, num_outliers, near_pi, rejected_exactly (TLS: the zero weights
               are the injected outliers), wall_s, and the library's own clocks edge_ms, inner_ms, total_ms
  older_route  the same levels at the same mu through the calls the library had: NodeGroup.ml_eval for chi2, the weights in
               numpy through gnc_weight_debug, Graph.filter_edges of the zero weights with Omega scaled by the weights through
               graph_from_edges(info=...), a new trivial-loss group, NodeGroup.ml_polish -- wall seconds in all and per level,
               and whether it ends with the same zero weights.  (Graph.scale_edges cannot serve: a zero weight gives Omega = 0,
               which the information check refuses.)
What the two clocks include: ml_gnc's is the call alone, on a group built outside the clock (a caller that iterated has one);
the older route's starts with nothing but the graph, so it holds the level-0 group and its ml_polish too, levels + 1 groups in
all -- per_level_s divides by levels + 1 for that reason.  One group's set-up is the route's unit of cost either way.
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
QUANTILE = {2: 16.266, 3: 22.458}


def corrupt(G, nn, robust, fraction, seed):
    """(the graph with `fraction` of the robust-set closures replaced by gross outliers and Omega kept, their mask)."""
    I, J, R, t, kap, tau = G.edges()
    Om = G.edge_information()[0]
    rng = np.random.default_rng(seed)
    closures = np.nonzero(robust & (np.abs(I - J) != 1))[0]
    bad = rng.choice(closures, max(1, int(round(fraction * len(closures)))), replace=False)
    R, t = R.copy(), t.copy()
    R[bad] = synthetic._random_rotations_d(rng, len(bad), G.d)
    t[bad] += 3.0 * rng.standard_normal((len(bad), G.d)) * (1.0 + np.linalg.norm(t[bad], axis=1, keepdims=True))
    mask = np.zeros(len(I), bool)
    mask[bad] = True
    return dpgo_amd.graph_from_edges(G.d, G.num_poses, I, J, R, t, kap, tau, nn, info=Om), mask


def reweighted(G, nn, w):
    """The graph of the edges with w > 0, Omega_e scaled by w_e (kappa and tau too)."""
    I, J, R, t, kap, tau = G.edges()
    Om = G.edge_information()[0]
    k = w > 0
    return dpgo_amd.graph_from_edges(G.d, G.num_poses, I[k], J[k], R[k], t[k], kap[k] * w[k], tau[k] * w[k], nn,
                                     info=Om[k] * w[k, None, None])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="torus3D,sphere2500,M3500,city10000")
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
        X = drv.group.polish(np.array(drv.X()))[0]
        w0 = drv.group.ml_gnc_eval(G, X, kind, 1.0, 1.0, w_start=np.full(G.num_edges, -1.0))[1]
        robust = w0 >= 0                                      # (the pass writes its weights on the robust set only)
        del drv
        barc2 = a.barc2 if a.barc2 > 0 else QUANTILE[G.d]
        Gc, injected = corrupt(G, nn, robust, a.fraction, a.seed)
        grp = dpgo_amd.NodeGroup(Gc, range(nn), trivial)
        opt = dpgo_amd.GncOptions(kind=kind, barc2=barc2)
        clocks = []
        for _ in range(a.reps):
            grp.sync()
            t0 = time.perf_counter()
            out = grp.ml_gnc(Gc, X, opt)
            clocks.append((time.perf_counter() - t0, out[2].edge_ms, out[2].inner_ms, out[2].total_ms))
        Xg, wg, res, log = out
        med = np.median(np.array(clocks), axis=0)
        line = dict(input=name, kind=a.kind, d=G.d, poses=G.num_poses, edges=G.num_edges, nodes=nn, robust=int(robust.sum()),
                    injected=int(injected.sum()), barc2=barc2,
                    ml_gnc=dict(outcome=dpgo_amd.GNC_NAMES[res.outcome], levels=res.levels, steps=res.steps,
                                factorisations=res.factorisations, num_zero=res.num_zero, num_outliers=res.num_outliers,
                                near_pi=res.near_pi, rejected_exactly=bool(np.array_equal(wg == 0, injected)), wall_s=float(med[0]),
                                edge_ms=float(med[1]), inner_ms=float(med[2]), total_ms=float(med[3]), device_bytes=res.device_bytes))
        # the older route: the same levels, every one of them a new graph and a new group
        walls = []
        for _ in range(a.reps):
            grp.sync()
            t0 = time.perf_counter()
            g0 = dpgo_amd.NodeGroup(Gc, range(nn), trivial)
            Xo = g0.ml_polish(X)[0]
            wo = np.ones(Gc.num_edges)
            for k in range(res.levels):
                chi2 = g0.ml_eval(Xo)[2]
                wo = np.ones(Gc.num_edges)
                wo[robust] = dpgo_amd.gnc_weight_debug(kind, log[k, 0], barc2, chi2[robust])[0]
                Gw = reweighted(Gc, nn, wo)
                gw = dpgo_amd.NodeGroup(Gw, range(nn), trivial)
                Xo = gw.ml_polish(Xo)[0]
                gw.sync()
                del gw, Gw
            walls.append(time.perf_counter() - t0)
        wall = float(np.median(walls))
        line["older_route"] = dict(wall_s=wall, per_level_s=wall / max(res.levels + 1, 1),
                                   same_zero_weights=bool(np.array_equal(wo == 0, wg == 0)))
        print(json.dumps(line), flush=True)
        del grp


if __name__ == "__main__":
    main()
