"""Regenerates tests/golden/robust_trajectories.json and tests/golden/robust_starts.npz: the robust Newton polish of
tests/robust_restatement.py (plain numpy, no GPU) on the inputs of tests/test_gpu_robust_polish.py, with the true Hessian
(curvature 1) and the re-weighted one (curvature 0).

    python tests/golden/make_robust_trajectories.py

Start points: "amm" is the oracle's Huber (delta 0.25) AMM-PGO# run from the chordal point on the row's partition (100
iterations on tinyGrid3D, 200 on smallGrid3D); "chordal" the chordal point; "own" the X of edge_restatement.random_graph;
"prev" the end point of the row named.  delta "median" is the median of the inter-edge s_e at the start point, computed here
and stored.  A row whose curvature-1 run CONVERGED with at most 12 factorisations is a device trajectory case ("device": true).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import edge_restatement as er  # noqa: E402
import robust_restatement as rr  # noqa: E402
from oracle import g2o as og  # noqa: E402
from oracle.hash import Options as OOptions  # noqa: E402
from oracle.problem import LOSS_GM, LOSS_HUBER, LOSS_WELSCH  # noqa: E402
from oracle.star import DistPGO as ODistPGO, chordal_initialization  # noqa: E402

AMM_ITERS = {"tinyGrid3D": 100, "smallGrid3D": 200}
# name, input, nodes, loss, delta (a number or "median"), start
ROWS = [
    ("tiny2_huber", "tinyGrid3D", 2, LOSS_HUBER, 0.25, "amm"),
    ("small2_huber", "smallGrid3D", 2, LOSS_HUBER, 0.25, "amm"),
    ("small5_huber", "smallGrid3D", 5, LOSS_HUBER, 0.25, "amm"),
    ("small2_huber_median", "smallGrid3D", 2, LOSS_HUBER, "median", "amm"),
    ("small2_huber_median_chordal", "smallGrid3D", 2, LOSS_HUBER, "median", "chordal"),
    ("small5_huber_median", "smallGrid3D", 5, LOSS_HUBER, "median", "amm"),
    ("small5_huber_median_chordal", "smallGrid3D", 5, LOSS_HUBER, "median", "chordal"),
    ("small2_gm_median", "smallGrid3D", 2, LOSS_GM, "median", "amm"),
    ("small2_welsch_median", "smallGrid3D", 2, LOSS_WELSCH, "median", "amm"),
    ("tiny2_gm_median", "tinyGrid3D", 2, LOSS_GM, "median", "amm"),
    ("tiny2_welsch_median", "tinyGrid3D", 2, LOSS_WELSCH, "median", "amm"),
    ("random2_huber5", "random:2:160:40", 4, LOSS_HUBER, 5.0, "own"),
    ("random2_huber20", "random:2:160:40", 4, LOSS_HUBER, 20.0, "prev:random2_huber5"),
    ("random3_huber5", "random:3:160:40", 4, LOSS_HUBER, 5.0, "own"),
    ("random2_welsch_median", "random:2:160:40", 4, LOSS_WELSCH, "median", "prev:random2_huber5"),
    ("random2_welsch100", "random:2:160:40", 4, LOSS_WELSCH, 100.0, "prev:random2_huber5"),
    # nodes of 75 poses (a second 64-row segment with a tail), and nodes of one pose
    ("big2_huber5", "random:2:600:150", 2, LOSS_HUBER, 5.0, "own"),
    ("ones2_huber5", "random:2:40:5", 4, LOSS_HUBER, 5.0, "own"),
    ("ones3_huber5", "random:3:40:5", 4, LOSS_HUBER, 5.0, "own"),
]


def load(inp, nn):
    """(problem dict of robust_restatement, own X or None)."""
    if inp.startswith("random:"):
        d, m, N = (int(v) for v in inp.split(":")[1:])
        g = er.random_graph(d, m, N=N)
        return rr.problem(d, N, g["I"], g["J"], g["R"], g["t"], g["kappa"], g["tau"], nn), np.array(g["X"])
    N, mm = og.read_g2o_file(os.path.join(ROOT, "fixtures", "g2o", inp + ".g2o"))
    return rr.problem(mm.d, N, mm.ipose, mm.jpose, mm.R, mm.t, mm.kappa, mm.tau, nn), None


def amm_point(inp, nn):
    path = os.path.join(ROOT, "fixtures", "g2o", inp + ".g2o")
    N, mm = og.read_g2o_file(path)
    orc = ODistPGO(path, nn, OOptions.driver(LOSS_HUBER, True), X0=chordal_initialization(N, mm), mm=mm, num_poses=N)
    for _ in range(AMM_ITERS[inp]):
        orc.step(evaluate=False)
    return orc.gather()


def main():
    starts, ends, table = {}, {}, []
    for name, inp, nn, loss, delta, start in ROWS:
        P, own = load(inp, nn)
        if start == "amm":
            key = "amm_%s_%d" % (inp, nn)
            if key not in starts:
                starts[key] = amm_point(inp, nn)
            X = starts[key]
        elif start == "chordal":
            N, mm = og.read_g2o_file(os.path.join(ROOT, "fixtures", "g2o", inp + ".g2o"))
            X, key = chordal_initialization(N, mm), None
        elif start == "own":
            X, key = own, None
        else:
            key = "end_" + start.split(":")[1]
            X = starts[key] = ends[start.split(":")[1]]
        if delta == "median":
            s = rr.weights(P, X, 0, 1.0)[0]
            dl = float(np.median(s[P["inter"]]))
        else:
            dl = float(delta)
        row = dict(name=name, input=inp, nodes=nn, loss=int(loss), delta=dl, delta_rule=str(delta), start=start, start_key=key)
        for curv in (1, 0):
            r = rr.polish_full(P, X, loss, dl, curv)
            row["curvature%d" % curv] = dict(outcome=int(r["outcome"]), steps=int(r["steps"]), factorisations=int(r["factorisations"]),
                                             indefinite=int(r["indefinite"]), tries=[int(v) for v in r["log"][:, 4]],
                                             F=[float(v) for v in r["log"][:, 0]], grad_final=float(r["grad_final"]))
            if curv == 1:
                ends[name] = r["X"]
        c1 = row["curvature1"]
        row["device"] = bool(c1["outcome"] == rr.CONVERGED and c1["factorisations"] <= 12)
        print(name, dl, "curvature 1:", c1["outcome"], c1["steps"], c1["factorisations"], c1["indefinite"], "| curvature 0:",
              row["curvature0"]["outcome"], row["curvature0"]["steps"], row["curvature0"]["factorisations"], "device", row["device"],
              flush=True)
        table.append(row)
    with open(os.path.join(HERE, "robust_trajectories.json"), "w") as f:
        json.dump(table, f, indent=1)
    np.savez_compressed(os.path.join(HERE, "robust_starts.npz"), **starts)


if __name__ == "__main__":
    main()
