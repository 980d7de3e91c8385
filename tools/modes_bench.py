"""Hessian-modes benchmark: NodeGroup.hessian_modes (the tangent-space Hessian written on the device and factored, a block of
16 ceil((k + 4) / 16) columns solved in one batch per iteration, two Gram matrices, the host's small eigenproblem, the Ritz
update; dpgo_amd/csrc/modes.cpp) on one GPU.

  python tools/modes_bench.py [--inputs torus3D,sphere2500,M3500,city10000] [--k 8] [--reps 3] [--iters 300]

Inputs: tools/cov_bench.py's -- torus3D x 8, sphere2500 x 4, M3500 x 4 and city10000 x 8 -- after --iters AMM-PGO# iterations
(LOSS_NONE, driver options) and NodeGroup.polish.

Per input one JSON line: the outcome, the iterations, the block, lambda_0 ... lambda_{k-1}, the worst residual, the predicted
device bytes, and -- medians of --reps calls after one warm-up call, on the library's host clock -- factor_ms, solve_ms, gram_ms,
ritz_ms, update_ms, total_ms.  Beside them the route that exists without hessian_modes, as the reference time:
NodeGroup.cov_hessian read back to the host, then scipy.sparse.linalg.eigsh(k, sigma=0) on the matrix without the anchor's rows
(reference_ms, its values, and the largest difference between the two sets of values).  Both kernels of an iteration stream
2 n b doubles (the update writes n b more): that count over gram_ms + update_ms is reported against the HBM peak, read-backs and
launch gaps included.  Nothing here is part of bench.py."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import dpgo_amd  # noqa: E402
import cov_bench  # noqa: E402  (its inputs)

PEAK_HBM = 8.0e12


def reference_route(grp, X, d, N, k):
    """cov_hessian to the host, the anchor's rows struck out, eigsh in shift-invert mode about 0: (ms, values ascending)."""
    dof = d + d * (d - 1) // 2
    t0 = time.perf_counter()
    ptr, col, val = grp.cov_hessian(X)
    H = sp.csr_matrix((val, col, ptr), shape=(dof * N, dof * N))[dof:, dof:].tocsc()
    w = spla.eigsh(H, k=k, sigma=0.0, which="LM", return_eigenvectors=True)[0]
    return 1e3 * (time.perf_counter() - t0), np.sort(w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="torus3D,sphere2500,M3500,city10000")
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=300)
    a = ap.parse_args()
    med = lambda v: float(np.median(v)) if v else None
    phases = ("factor_ms", "solve_ms", "gram_ms", "ritz_ms", "update_ms", "total_ms")
    for name in a.inputs.split(","):
        G = cov_bench.graph(name)
        grp = dpgo_amd.NodeGroup(G, range(G.num_nodes), dpgo_amd.Options.driver(dpgo_amd.LOSS_NONE, True, max_iterations=0))
        drv = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(dpgo_amd.LOSS_NONE, True))
        for _ in range(a.iters):
            assert drv.step() == 0
        X0 = np.array(drv.X())
        del drv
        X, pres, _ = grp.polish(X0)
        out = grp.hessian_modes(X, a.k)
        r = out["result"]
        times = {p: [] for p in phases}
        if r.outcome in (dpgo_amd.MODES_CONVERGED, dpgo_amd.MODES_MAX_ITERS):
            for _ in range(a.reps):
                out = grp.hessian_modes(X, a.k)
                r = out["result"]
                for p in phases:
                    times[p].append(getattr(r, p))
        line = dict(input=name, point="polished (%s)" % dpgo_amd.POLISH_NAMES[pres.outcome], d=G.d, poses=G.num_poses, nodes=G.num_nodes,
                    k=a.k, outcome=dpgo_amd.MODES_NAMES[r.outcome], iterations=r.iterations, factorisations=r.factorisations,
                    shift_tries=r.shift_tries, block=r.block, negative=r.negative, mu=r.mu, hmax=r.hmax, unknowns=r.unknowns,
                    fronts=r.fronts, levels=r.levels, max_front=r.max_front, device_bytes=r.device_bytes, stationarity=r.stationarity,
                    values=out["values"].tolist(), worst_residual=float(out["residuals"].max()),
                    largest_covariance_eigenvalue=(1.0 / out["values"][0] if out["values"][0] > 0 else None),
                    top_pose_of_mode_0=int(np.argmax(out["energy"][0])), **{p: med(times[p]) for p in phases})
        if line["gram_ms"] and r.iterations:
            moved = 8.0 * r.unknowns * r.block * 5 * r.iterations
            line["stream_bytes"] = moved
            line["stream_share_of_hbm_peak"] = moved / ((line["gram_ms"] + line["update_ms"]) * 1e-3) / PEAK_HBM
            line["ms_per_iteration"] = (line["solve_ms"] + line["gram_ms"] + line["ritz_ms"] + line["update_ms"]) / r.iterations
        if r.outcome in (dpgo_amd.MODES_CONVERGED, dpgo_amd.MODES_MAX_ITERS):
            try:
                refs = [reference_route(grp, np.asarray(X), G.d, G.num_poses, a.k) for _ in range(a.reps + 1)][1:]
                line.update(reference_ms=med([v[0] for v in refs]), reference_values=refs[-1][1].tolist(),
                            worst_value_difference=float(np.abs(refs[-1][1] - out["values"]).max()))
                line["reference_ms_over_device_ms"] = line["reference_ms"] / line["total_ms"]
            except Exception as e:   # (eigsh's factorisation refuses a matrix that is not positive definite enough for sigma = 0)
                line["reference_error"] = repr(e)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
