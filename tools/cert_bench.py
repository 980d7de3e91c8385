"""Certificate benchmark: NodeGroup.certify (LOBPCG on S = M - Lambda(X), dpgo_amd/csrc/cert.cpp) on one GPU.

  python tools/cert_bench.py [--inputs headline-chordal,headline-50,torus3D,sphere2500] [--reps 5] [--iters 200]
                             [--cpu-iters 20] [--no-cpu] [--trace kernel_trace.csv]

Inputs: the headline lattice of dpgo_amd/synthetic.py (100 k poses, seed 20240817, 8 nodes) at its chordal point and after
50 AMM-PGO# iterations; torus3D x 8 and sphere2500 x 4 at their chordal points.  LOSS_NONE, all nodes on one GPU.

Per input, one JSON line:
  * the decision with default options (status, iterations, theta, wall time of the call);
  * the time per LOBPCG iteration: a run of exactly --iters iterations (stop_on_negative off, tau = 1e-300) against a run of
    none, both host clocks around calls that end synchronised -- the difference is the loop alone (uploads, the norm
    estimate and the final product are in both); median of --reps after one warm-up;
  * the CPU restatement (tests/cert_restatement.py: scipy sparse products, numpy for the row-local part) on the same X and
    V0: time per iteration over --cpu-iters iterations and the time of its default-options decision.  There is no
    reference binary to time (its Eigen / CHOLMOD stack is not here) and no earlier implementation in this project: the
    restatement is the only baseline there is.
Kernel times come from a separate profiler run, never combined with counters:
  rocprofv3 --kernel-trace --stats -f csv -d DIR -o cert -- python tools/cert_bench.py --inputs headline-chordal --no-cpu
and --trace DIR/.../cert_kernel_trace.csv then adds, per kernel, the median duration and the fraction of the HBM roofline
(8 TB/s) at its algorithmic bytes per row, P = (d+1) d 8 the bytes of a record:
  k_cert_gram    6 P + 8 d^2 read, P written        k_cert_update  6 P + 8 (d+1)^2 read, 5 P written
  k_bsr          nnzb (8 (d+1)^2 + 4) + 2 P per row (the count bench.py's profile uses)."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dpgo_amd  # noqa: E402
from dpgo_amd import synthetic  # noqa: E402

HBM_BYTES_PER_S = 8e12


def load(name):
    """(graph, X, label, edges for the oracle)"""
    if name.startswith("headline"):
        h = synthetic.HEADLINE
        g = synthetic.grid(h["nx"], h["ny"], h["nz"], h["num_edges"], seed=h["seed"])
        G = dpgo_amd.graph_from_edges(g["d"], g["num_poses"], g["I"], g["J"], g["R"], g["t"], g["kappa"], g["tau"], 8)
        if name == "headline-50":
            drv = dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(dpgo_amd.LOSS_NONE, True))
            for _ in range(50):
                assert drv.step() == 0
            return G, np.array(drv.X()), g
        return G, np.array(G.chordal_initialization()), g
    nn = {"torus3D": 8, "sphere2500": 4, "M3500": 4}[name]
    G = dpgo_amd.read_g2o(os.path.join(ROOT, "fixtures", "g2o", name + ".g2o"), nn)
    I, J, R, t, kap, tau = G.edges()
    return G, np.array(G.chordal_initialization()), dict(d=G.d, num_poses=G.num_poses, I=I, J=J, R=R, t=t, kappa=kap, tau=tau)


def kernel_ms_from_trace(path):
    out = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row.get("Kernel_Name", "")
            for k in ("k_cert_gram", "k_cert_update", "k_cert_reduce", "k_cert_apply", "k_bsr", "k_copy_indexed"):
                if k + "<" in name or k + "(" in name or name.endswith(k) or ("::" + k) in name:
                    out.setdefault(k, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6)
                    break
    return out


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="headline-chordal,headline-50,torus3D,sphere2500")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--cpu-iters", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--trace", default=None)
    a = ap.parse_args()
    traced = kernel_ms_from_trace(a.trace) if a.trace else {}
    for name in a.inputs.split(","):
        G, X, g = load(name)
        d, N = G.d, G.num_poses
        grp = dpgo_amd.NodeGroup(G, range(G.num_nodes), dpgo_amd.Options.driver(dpgo_amd.LOSS_NONE, True, max_iterations=0))
        V0 = np.random.default_rng(0).standard_normal(X.shape)
        t0 = time.perf_counter()
        res, _ = grp.certify(X, V0=V0)
        t_dec = time.perf_counter() - t0
        fixed = dict(V0=V0, stop_on_negative=False, tau=1e-300)
        t_none = timed(lambda: grp.certify(X, max_iters=0, **fixed), a.reps)
        t_loop = timed(lambda: grp.certify(X, max_iters=a.iters, **fixed), a.reps)
        out = dict(input=name, d=d, poses=N, nodes=G.num_nodes, status=dpgo_amd.CERT_NAMES[res.status], iterations=res.iterations,
                   restarts=res.restarts, theta=res.theta, residual=res.residual, stationarity=res.stationarity,
                   decision_s=t_dec, setup_s=t_none, ms_per_iteration=(t_loop - t_none) / a.iters * 1e3, timed_iterations=a.iters)
        P = (d + 1) * d * 8.0
        if traced:
            I, J = np.asarray(g["I"]), np.asarray(g["J"])
            bytes_row = dict(k_cert_gram=7 * P + 8 * d * d, k_cert_update=11 * P + 8 * (d + 1) ** 2)
            for k, b in bytes_row.items():
                if k in traced:
                    ms = float(np.median(traced[k]))
                    out[k] = dict(median_ms=ms, launches=len(traced[k]), bytes=b * N, hbm_fraction=b * N / (ms * 1e-3) / HBM_BYTES_PER_S)
            if "k_bsr" in traced:
                # the two passes of one product together read every block of M once: 2 m off-diagonal blocks + the diagonals of G and S
                ms = float(np.median(traced["k_bsr"]))
                blocks = 2 * len(I) + 2 * N
                b = blocks * (8.0 * (d + 1) ** 2 + 4) + 2 * 2 * N * P
                out["k_bsr"] = dict(median_ms=ms, launches=len(traced["k_bsr"]), bytes_of_a_pair=b,
                                    hbm_fraction_of_a_pair=b / (2 * ms * 1e-3) / HBM_BYTES_PER_S)
            for k in ("k_cert_reduce", "k_copy_indexed"):
                if k in traced:
                    out[k] = dict(median_ms=float(np.median(traced[k])), launches=len(traced[k]))
        if not a.no_cpu:
            import cert_restatement as cr
            from oracle import g2o as og
            from oracle.hash import Options as OOptions
            from oracle.star import GlobalProblem
            z = np.zeros(len(g["I"]), np.int64)
            mm = og.Measurements(z, g["I"], z, g["J"], g["R"], g["t"], g["kappa"], g["tau"])
            M = GlobalProblem(N, mm, 1, OOptions.driver(0, True)).M.tocsr()
            t0 = time.perf_counter()
            cr.lobpcg(M, X, d, V0, max_iters=0)
            c_none = time.perf_counter() - t0
            t0 = time.perf_counter()
            cr.lobpcg(M, X, d, V0, max_iters=a.cpu_iters, stop_on_negative=False, tau=1e-300)
            c_loop = time.perf_counter() - t0
            t0 = time.perf_counter()
            c = cr.lobpcg(M, X, d, V0)
            c_dec = time.perf_counter() - t0
            out.update(cpu_ms_per_iteration=(c_loop - c_none) / a.cpu_iters * 1e3, cpu_decision_s=c_dec, cpu_iterations=c["iterations"],
                       cpu_status=dpgo_amd.CERT_NAMES[c["status"]], cpu_theta=c["theta"], cpu_threads=os.cpu_count() if not
                       os.environ.get("OMP_NUM_THREADS") else int(os.environ["OMP_NUM_THREADS"]))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
