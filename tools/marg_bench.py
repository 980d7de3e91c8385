"""Joint-marginal benchmark: NodeGroup.joint_marginal (the tangent-space Hessian written on the device and factored, the unit
columns of the kept poses solved in batches of 64, Sigma_KK gathered, the dense one-front factorisation of order n and its
inverse; dpgo_amd/csrc/marg.cpp) on one GPU.

  python tools/marg_bench.py [--inputs torus3D,sphere2500,M3500,city10000] [--reps 3] [--iters 300] [--max-poses 0] [--relative]

Inputs: tools/cov_bench.py's -- torus3D x 8, sphere2500 x 4, M3500 x 4 and city10000 x 8 -- after --iters AMM-PGO# iterations
(LOSS_NONE, driver options) and NodeGroup.polish.  The kept set is every pose with an inter-node edge, ascending, without the
anchor 0; --max-poses K > 0 keeps every (count / K)-th of them, so that n = dof K stays inside the widest root front the
factorisation's panel kernel has been measured at.  --relative: the first kept pose is the base.

Per input one JSON line: n, columns, batches, the predicted device bytes, the dense pivots, and -- medians of --reps calls after
one warm-up call, on the library's host clock -- factor_ms, solve_ms, dense_ms; beside them NodeGroup.pair_covariance over the
same poses chained as K - 1 pairs (the same columns: pair_solve_ms should match solve_ms, the gap is reported); and the dense
phase against the fp64 matrix peak, counting n^3 flops (Cholesky, the inverse of the factor and W^T W, n^3 / 3 each) over
dense_ms, which also holds the copies of info to the host.  Nothing here is part of bench.py."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import dpgo_amd  # noqa: E402
import cov_bench  # noqa: E402  (its inputs)

PEAK_FP64_MATRIX = 78.6e12


def boundary_poses(G):
    """Every pose with an edge to a pose of another node, ascending."""
    I, J = (np.asarray(v) for v in G.edges()[:2])
    off = np.array([G.node_offset(a) for a in range(G.num_nodes)])
    node = lambda p: np.searchsorted(off, p, side="right") - 1
    inter = node(I) != node(J)
    return np.unique(np.concatenate([I[inter], J[inter]]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="torus3D,sphere2500,M3500,city10000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--max-poses", type=int, default=0)
    ap.add_argument("--relative", action="store_true")
    a = ap.parse_args()
    med = lambda v: float(np.median(v)) if v else None
    for name in a.inputs.split(","):
        G = cov_bench.graph(name)
        grp = dpgo_amd.NodeGroup(G, range(G.num_nodes), dpgo_amd.Options.driver(dpgo_amd.LOSS_NONE, True, max_iterations=0))
        drv = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(dpgo_amd.LOSS_NONE, True))
        for _ in range(a.iters):
            assert drv.step() == 0
        X0 = np.array(drv.X())
        del drv
        X, pres, _ = grp.polish(X0)
        point = "polished (%s)" % dpgo_amd.POLISH_NAMES[pres.outcome]
        keep = boundary_poses(G)
        keep = keep[keep != 0]
        boundary = len(keep)
        if a.max_poses > 0 and len(keep) > a.max_poses:
            keep = keep[np.linspace(0, len(keep) - 1, a.max_poses).astype(int)]
        base = int(keep[0]) if a.relative else None
        first = grp.joint_marginal(X, keep, base=base)["result"]
        r, fac, sol, den = first, [], [], []
        if first.outcome == dpgo_amd.MARG_OK:
            for _ in range(a.reps):
                r = grp.joint_marginal(X, keep, base=base)["result"]
                fac.append(r.factor_ms); sol.append(r.solve_ms); den.append(r.dense_ms)
        line = dict(input=name, point=point, d=G.d, poses=G.num_poses, nodes=G.num_nodes, boundary_poses=boundary, kept=len(keep),
                    relative=bool(a.relative), outcome=dpgo_amd.MARG_NAMES[r.outcome], info_not_pd=r.info_not_pd, n=r.n, columns=r.columns,
                    batches=r.batches, device_bytes=r.device_bytes, unknowns=r.unknowns, max_front=r.max_front, factor_ms=med(fac),
                    solve_ms=med(sol), dense_ms=med(den), dense_pivot_min=r.dense_pivot_min, dense_pivot_max=r.dense_pivot_max,
                    pivot_min=r.pivot_min, stationarity=r.stationarity)
        if line["dense_ms"]:
            line["dense_share_of_fp64_matrix_peak"] = float(r.n) ** 3 / (line["dense_ms"] * 1e-3) / PEAK_FP64_MATRIX
        if first.outcome == dpgo_amd.MARG_OK and len(keep) > 1:
            pairs = np.stack([keep[:-1], keep[1:]], axis=1)
            ps = [grp.pair_covariance(X, pairs)["result"] for _ in range(a.reps + 1)][1:]
            line.update(pair_columns=ps[-1].columns, pair_solve_ms=med([p.solve_ms for p in ps]))
            line["solve_ms_over_pair_solve_ms"] = line["solve_ms"] / line["pair_solve_ms"]
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
