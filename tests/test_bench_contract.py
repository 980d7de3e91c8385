"""The bench.py contract (one JSON line): the keys the driver and the judge read, checked on the committed line of the
last profiling run (profiles/rNN_bench_n1.json) and, on a GPU box, on a fresh short run."""
import glob
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check(j, n1=True, full=True):
    """full: a line of `bench.py --full` (roofline, cpu_baseline, convergence); otherwise a plain line, which has none."""
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config"):
        assert k in j, k
    assert j["unit"] == "iters/s" and j["higher_is_better"] is True and j["dtype"] == "f64" and j["data"] == "synthetic"
    assert j["vs_baseline"] is None                       # BASELINE.md publishes no number for this metric
    assert "workload" in j["config"] and "model" not in j["config"]
    assert abs(j["value"] * j["ms_per_step"] * 1e-3 - 1.0) < 1e-6      # iterations / s and ms / iteration agree
    if not full:
        assert j["roofline"] is None and not j["kernels"] and j["cpu_baseline"] is None and "convergence" not in j
        return
    r = j["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and 0.0 < r["frac"] < 1.0
    if n1:
        c = j["cpu_baseline"]
        for k in ("value", "unit", "cores", "kind", "sample"):
            assert k in c, k
        assert c["kind"] == "port" and c["unit"] == j["unit"] and c["cores"] >= 1
        cv = j["convergence"]
        assert cv["iterations_to_1e-6"] > 0 and cv["seconds_to_1e-6"] > 0
        if "iters_per_s_to_objective" in j:      # (lines committed before round 5 do not carry it)
            assert abs(j["iters_per_s_to_objective"] - cv["iterations_to_1e-6"] / cv["seconds_to_1e-6"]) < 1e-6 * j["iters_per_s_to_objective"]


def test_committed_bench_line():
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_bench_n1.json")))
    assert files
    _check(json.load(open(files[-1])))


def test_bench_help_runs_without_a_gpu():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True)
    text = out.stdout + out.stderr      # (bench.py keeps stdout for the JSON line)
    assert out.returncode == 0 and "--gpus" in text and "--steps" in text and "--warmup" in text


def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus 2` with no launcher around it (the way the driver may start it) must spawn its two
    ranks itself and reach the rendezvous -- not exit with "WORLD_SIZE=1"; a failing rank makes it return non-zero."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--share-gpu",
                          "--rendezvous-only"], capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["rendezvous"] == "ok" and j["n_gpus"] == 2
    assert sorted(r[0] for r in j["ranks"]) == [0, 1] and len({r[2] for r in j["ranks"]}) == 1
    # num_nodes = 8 is not divisible by 3 ranks: every rank exits with an error, and so does the launcher
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "3", "--backend", "gloo", "--share-gpu",
                          "--rendezvous-only"], capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
    assert bad.returncode != 0 and not [l for l in bad.stdout.splitlines() if l.startswith("{")]


def test_launcher_names_and_stops_ranks_that_hang_or_die():
    """The first N > 1 run must end with an exit code and a message, never at the caller's own timeout: (i) a rank that
    dies while the other waits in a collective makes `bench.py --gpus 2` return non-zero at once, (ii) a rank that hangs
    is stopped at --rank-timeout with the ranks still alive named on stderr (exit code 124).  gloo on the CPU; the
    launcher only ever starts and stops fresh children."""
    import time
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--share-gpu", "--rendezvous-only"]
    t0 = time.time()
    died = subprocess.run(cmd + ["--rank-timeout", "240"], capture_output=True, text=True, cwd=ROOT, timeout=300,
                          env=dict(env, DPGO_BENCH_TEST_DIE_RANK="1"))
    assert died.returncode not in (0, 124) and time.time() - t0 < 200, died.stderr[-2000:]
    assert "rank 1 exited with code 3" in died.stderr and not [l for l in died.stdout.splitlines() if l.startswith("{")]
    t0 = time.time()
    hung = subprocess.run(cmd + ["--rank-timeout", "45"], capture_output=True, text=True, cwd=ROOT, timeout=300,
                          env=dict(env, DPGO_BENCH_TEST_HANG_RANK="1"))
    assert hung.returncode == 124, hung.stderr[-2000:]
    assert 40 < time.time() - t0 < 120
    # (rank 1 sleeps, rank 0 waits for it in the barrier: both are named)
    assert "ranks [0, 1] still running after --rank-timeout 45 s" in hung.stderr, hung.stderr[-2000:]
    assert not [l for l in hung.stdout.splitlines() if l.startswith("{")]


_CONV_WORKER = r"""
import json, os, sys
sys.path.insert(0, %r)
import torch.distributed as dist
import bench
os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
dist.init_process_group("gloo")
rank = dist.get_rank()
# rank r's own clock and its four nodes' sums per iteration: the objective halves every iteration towards 100 (rank 0) /
# 300 (rank 1); rank 1 is the slower one
trace = [((k + 1) * (0.001 + 0.0005 * rank), (100.0 + 200.0 * rank) * (1.0 + 0.5 ** k), 8.0 * (k %% 3 == 0), 2.0 + rank) for k in range(30)]
out = bench.reduce_trace(trace, dist, 8)
conv = bench.summarize_convergence(out, 30, None)
if rank == 0:
    print(json.dumps({"trace": out, "convergence": conv}))
dist.destroy_process_group()
"""


def test_convergence_block_of_the_two_rank_line():
    """The second half of BASELINE's metric at N > 1 (missing item 1): every rank keeps its own per-iteration
    clock and sums, bench.reduce_trace combines them (objective, CG steps, refined nodes: sums over the ranks; time: the
    slowest rank's) and bench.summarize_convergence writes the same block the N = 1 line carries.  World 2, gloo, CPU."""
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, "-c", _CONV_WORKER % ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=240) for p in procs]
    assert all(p.returncode == 0 for p in procs), outs[1][1][-2000:] + outs[0][1][-2000:]
    j = json.loads([l for l in outs[0][0].splitlines() if l.startswith("{")][-1])
    tr, cv = j["trace"], j["convergence"]
    assert len(tr) == 30
    for k, (t, f, cg, ref) in enumerate(tr):
        assert abs(t - (k + 1) * 0.0015) < 1e-12                          # the slower rank's clock
        assert abs(f - 400.0 * (1.0 + 0.5 ** k)) < 1e-9                   # the objective is the sum over the ranks
        assert ref == 5.0 and cg == (2.0 if k % 3 == 0 else 0.0)           # sums; CG steps per node of the 8
    # the objective first comes within 1e-6 of the run's lowest (400 (1 + 2^-29)) at iteration 20: 2^-19 < 1e-6 < 2^-18
    assert cv["target"] == "lowest objective of this run" and cv["iterations_to_1e-6"] == 21
    assert abs(cv["seconds_to_1e-6"] - 21 * 0.0015) < 1e-12
    assert abs(cv["iters_per_s_to_objective"] - 1.0 / 0.0015) < 1e-6
    for k in ("mean_ms_per_iter_to_1e-6", "mean_ms_per_iter_whole_run", "last20_ms_per_iter", "objective_2F_at", "lowest_2F"):
        assert k in cv


_DUMP_WORKER = r"""
import os, sys, types
import numpy as np
sys.path.insert(0, %r)
import bench
n, d, nodes = 1000, 3, 4
bench.DUMP_MAX_BYTES = 2 * 8 * (d + 1) * d * 50         # room for a sample of 50 poses
G = types.SimpleNamespace(d=d, num_poses=n)
class Group:
    def scatter_global(self, X):
        X[:] = np.arange(X.size, dtype=np.float64).reshape(X.shape, order="F")
        return 0
    def results(self, k):
        return types.SimpleNamespace(fobj=10.0 + k, gradFnorm=0.5 * k)
for out in sys.argv[1:]:
    bench.dump_outputs(out, G, Group(), [1, 3], nodes, None, 0)
"""


def test_dump_outputs_of_a_large_iterate_are_a_seeded_sample(tmp_path):
    """--dump-outputs stays within its 64 MB: an iterate larger than half of that is written as a fixed, seeded sample of
    poses (each pose's translation row and its rotation rows, and the poses' indices), the same one every time."""
    import numpy as np
    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    out = subprocess.run([sys.executable, "-c", _DUMP_WORKER % ROOT] + dirs, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    n, d = 1000, 3
    X = np.arange((d + 1) * n * d, dtype=np.float64).reshape(((d + 1) * n, d), order="F")
    got = [{f: np.load(os.path.join(p, f + ".npy")) for f in ("X_sample", "X_sample_poses", "fobj", "gradFnorm")} for p in dirs]
    g = got[0]
    assert sorted(os.listdir(dirs[0])) == ["X_sample.npy", "X_sample_poses.npy", "fobj.npy", "gradFnorm.npy"]
    assert sum(os.path.getsize(os.path.join(dirs[0], f)) for f in os.listdir(dirs[0])) <= 2 * 8 * (d + 1) * d * 50
    assert all(a.dtype == np.float64 for a in g.values())
    poses = g["X_sample_poses"].astype(int)
    assert len(poses) == 50 and len(set(poses)) == 50 and poses.min() >= 0 and poses.max() < n
    rows = np.concatenate([[p] + [n + d * p + r for r in range(d)] for p in poses])
    assert np.array_equal(g["X_sample"], X[rows])
    # the nodes this rank hosts (1 and 3) carry their results, the others 0
    assert np.array_equal(g["fobj"], [0.0, 10.0, 0.0, 11.0]) and np.array_equal(g["gradFnorm"], [0.0, 0.0, 0.0, 0.5])
    for f in g:
        assert np.array_equal(g[f], got[1][f]), f


@pytest.mark.gpu
def test_fresh_bench_line():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--grid", "20,20,16,25000", "--steps", "5",
                          "--warmup", "2", "--full", "--converge", "40", "--cpu-steps", "1"], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                                # ONE JSON line
    _check(json.loads(lines[0]))


@pytest.mark.gpu
def test_plain_bench_line_and_its_outputs(tmp_path):
    """A plain run (no --full) times --steps steps and prints the headline line only; --dump-outputs writes what the last
    timed step computed (float64), and the same arguments give the same outputs in a second process."""
    import numpy as np
    lines = []
    for k in range(2):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--grid", "20,20,16,25000",
                              "--steps", "7", "--warmup", "2", "--dump-outputs", str(tmp_path / str(k))],
                             capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        lines.append([l for l in out.stdout.splitlines() if l.startswith("{")])
        assert len(lines[k]) == 1
        j = json.loads(lines[k][0])
        _check(j, full=False)
        assert j["steps"] == 7 and j["warmup"] == 2
    dumped = [{f: np.load(str(tmp_path / str(k) / (f + ".npy"))) for f in ("X", "fobj", "gradFnorm")} for k in range(2)]
    d = dumped[0]
    assert d["X"].shape == (4 * 20 * 20 * 16, 3) and d["fobj"].shape == d["gradFnorm"].shape == (8,)
    assert all(a.dtype == np.float64 and np.isfinite(a).all() for a in d.values())
    # the objective of the line is the sum of the nodes' fobj, and the rotation rows of X are rotations
    assert abs(d["fobj"].sum() - 0.5 * j["objective_2F"]) <= 1e-12 * abs(j["objective_2F"])
    n = 20 * 20 * 16
    R = d["X"][n:].reshape(n, 3, 3)
    assert np.abs(np.einsum("nij,nkj->nik", R, R) - np.eye(3)).max() < 1e-8
    for f in d:
        assert np.array_equal(d[f], dumped[1][f]), f
