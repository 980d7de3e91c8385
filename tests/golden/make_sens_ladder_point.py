"""Regenerates tests/golden/sens_ladder2_point.npz: a critical point of the compacted synthetic.ladder(d=2) (403 poses, 1358
edges) with pose 0 held fixed -- newton_restatement.polish from the chordal point, 69 steps of a dense 1209 x 1209
factorisation each (about 15 s), which is why tests/test_sens_host.py reads the point instead of computing it.  No GPU.

    python tests/golden/make_sens_ladder_point.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import newton_restatement as nr  # noqa: E402
import robust_restatement as rr  # noqa: E402
import test_sens_host as tsh  # noqa: E402
from oracle import g2o as og  # noqa: E402
from oracle.star import chordal_initialization  # noqa: E402

if __name__ == "__main__":
    P = tsh.ladder2_problem()
    z = np.zeros(len(P["I"]), np.int64)
    mm = og.Measurements(z, P["I"], z, P["J"], P["R"], P["t"], P["kappa"], P["tau"])
    X0 = chordal_initialization(P["N"], mm)
    M = rr.weighted_matrix(P, np.ones(len(P["I"])))
    out = nr.polish_full(M, X0, 2, 0, max_steps=400, grad_tol=1e-9)
    assert out["outcome"] == nr.CONVERGED
    print("%d steps, |g| = %.3g" % (out["steps"], out["grad_final"]))
    np.savez_compressed(os.path.join(HERE, "sens_ladder2_point.npz"), X=out["X"])
