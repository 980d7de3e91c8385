"""Inputs shared by the tests of the robust objective (tests/test_robust_host.py, tests/test_gpu_robust_*.py): test
infrastructure.  Every input is (problem dict of robust_restatement, a point X, nodes); `graph` and `group` make the library's
objects of it.  References are computed once per process and handed out unchanged."""
import json
import os

import numpy as np

import edge_restatement as er
import robust_restatement as rr

import dpgo_amd
from dpgo_amd import synthetic
from oracle import g2o as og
from oracle.problem import LOSS_NONE
from oracle.star import chordal_initialization

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = os.path.join(ROOT, "fixtures", "g2o")
GOLDEN = os.path.join(ROOT, "tests", "golden")

_inputs, _refs = {}, {}


def fixture(name, nn):
    """(P, chordal point) of a .g2o fixture."""
    key = (name, nn)
    if key not in _inputs:
        N, mm = og.read_g2o_file(os.path.join(FIXTURES, name + ".g2o"))
        P = rr.problem(mm.d, N, mm.ipose, mm.jpose, mm.R, mm.t, mm.kappa, mm.tau, nn)
        _inputs[key] = (P, np.asfortranarray(chordal_initialization(N, mm)))
    return _inputs[key]


def random(d, m, N, nn=4):
    key = ("random", d, m, N, nn)
    if key not in _inputs:
        g = er.random_graph(d, m, N=N)
        _inputs[key] = (rr.problem(d, N, g["I"], g["J"], g["R"], g["t"], g["kappa"], g["tau"], nn), np.asfortranarray(g["X"]))
    return _inputs[key]


def ladder(d, nn=4):
    """synthetic.inter_ladder(d) with its unused pose ids dropped (200 poses), at its ground truth, where the residual of
    every edge is its own noise and the kink edges sit at s / kink = 1 -+ [0.001, 0.1].  Compacting keeps the edges, their
    order and every incidence list (the hub's 300, the poses with 0 ... 40); the contiguous partition of the 200 poses into
    4 nodes of 50 is what the graph loader makes of it, so which edges are inter-node differs from the uncompacted graph."""
    key = ("ladder", d, nn)
    if key not in _inputs:
        g = synthetic.inter_ladder(d)
        used = np.unique(np.concatenate([g["I"], g["J"]]))
        new = np.full(g["num_poses"], -1, np.int64)
        new[used] = np.arange(len(used))
        P = rr.problem(d, len(used), new[g["I"]], new[g["J"]], g["R"], g["t"], g["kappa"], g["tau"], nn)
        X = synthetic.global_X(g["Rg"][used], g["tg"][used])
        _inputs[key] = (P, np.asfortranarray(X))
    return _inputs[key]


# random_graph(d, m, N) by m: (N, nodes).  600 edges on 150 poses in 2 nodes: 75 own poses per node, a second 64-row segment with
# a tail of 11; 40 edges on 5 poses in 4 nodes: node sizes 2, 1, 1, 1 -- one-pose nodes
RANDOM = {70: (20, 4), 160: (40, 4), 600: (150, 2), 40: (5, 4)}


def named(name):
    """tiny | rand{d}_{m} | ladder{d} | ladder{d}x2 (on 2 nodes of 100 poses: two segments per node) -> (P, X)."""
    if name == "tiny":
        return fixture("tinyGrid3D", 2)
    if name.startswith("rand"):
        d, m = int(name[4]), int(name.split("_")[1])
        return random(d, m, *RANDOM[m])
    if name.endswith("x2"):
        return ladder(int(name[6]), 2)
    return ladder(int(name[-1]))


def graph(P):
    return dpgo_amd.graph_from_edges(P["d"], P["N"], P["I"], P["J"], P["R"], P["t"], P["kappa"], P["tau"], P["num_nodes"])


def group(G, nn=None, loss=LOSS_NONE):
    nn = G.num_nodes if nn is None else nn
    return dpgo_amd.NodeGroup(G, range(nn), dpgo_amd.Options.driver(loss, True, max_iterations=0))


def scaled_graph(P, w):
    return graph(dict(P, kappa=P["kappa"] * w, tau=P["tau"] * w))


def reference(name, loss, delta, curvature=1, anchor=0):
    key = (name, loss, float(delta), curvature, anchor)
    if key not in _refs:
        P, X = named(name)
        _refs[key] = rr.reference(P, X, loss, delta, curvature, anchor)
    return _refs[key]


def trajectories():
    with open(os.path.join(GOLDEN, "robust_trajectories.json")) as f:
        return json.load(f)


def trajectory_problem(row):
    """(P, start point) of a row of the committed table."""
    inp, nn = row["input"], row["nodes"]
    if inp.startswith("random:"):
        d, m, N = (int(v) for v in inp.split(":")[1:])
        P, own = random(d, m, N, nn)
    else:
        P, chordal = fixture(inp, nn)
    if row["start"] == "own":
        X = own
    elif row["start"] == "chordal":
        X = chordal
    else:
        X = np.load(os.path.join(GOLDEN, "robust_starts.npz"))[row["start_key"]]
    return P, np.asfortranarray(X)
