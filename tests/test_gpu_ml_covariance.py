"""Marginal covariances of the maximum-likelihood objective on the device (Group::ml_covariance: cov_finish on the
Gauss-Newton Hessian of ml.hip) against the dense long-double inverse of the restated anchored H = sum J' Omega J, at the
restated refinement's final point, on tinyGrid3D x {1, 2} nodes, smallGrid3D x {1, 2, 5} and the d = 2 grid x {1, 3}; and on
the d = 2 ladder x 6 at the point its six replayed steps reach (its refinement cannot converge, tests/test_ml_host.py: WHOLE;
the Gauss-Newton H is positive definite there all the same, and the bound does not ask for a critical point).

The bound has tests/test_gpu_covariance.py's form: C u kappa_2(A) ||A^-1||_2 of tests/cov_restatement.py for the factorisation
and the selected inversion of A, plus what the matrix's own error moves the inverse by to first order, ||A^-1||_2^2 times the
2-norm of the bound of the matrix (tests/ml_restatement.py: sum_bounds, times tests/test_ml_host.py's constant).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_restatement as cr  # noqa: E402
import factor_restatement as fr  # noqa: E402
import ml_restatement as mr  # noqa: E402
import test_gpu_ml_ops as ops  # noqa: E402  (its groups; none of its tests is imported)
import test_ml_host as tmh  # noqa: E402  (the whole-call inputs and their trajectories; none of its tests is imported)

import dpgo_amd  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
CASES = [("tinyGrid3D", 1), ("tinyGrid3D", 2), ("smallGrid3D", 1), ("smallGrid3D", 2), ("smallGrid3D", 5), ("grid2", 1), ("grid2", 3),
         ("ladder2", 6)]
_ref = {}


def reference(fixtures_dir, name, anchor):
    key = (name, anchor)
    if key not in _ref:
        E = tmh.iso_point(fixtures_dir, name)[0]
        X = tmh.trajectory(fixtures_dir, name)["X"]
        N, dof = E["N"], cr.dof_of(E["d"])
        ref = mr.edges_all(E, X, cr.LD)
        bH = tmh.CONSTANTS["H"] * mr.sum_bounds(E, N, ref, mr.edge_bounds(E, X, ref))[2]
        A = np.asarray(mr.assemble(E, X, anchor, cr.LD, per_edge=ref)[2], np.float64)
        A = 0.5 * (A + A.T)
        lam = np.linalg.eigvalsh(A)
        assert lam[0] > 0
        L, kstar, _ = fr.cholesky_ld(A)
        assert kstar < 0
        Xi = fr.lower_inverse_ld(L)
        bSigma = cr.C * U * float(lam[-1] / lam[0]) / float(lam[0]) + float(np.linalg.norm(bH, 2)) / float(lam[0]) ** 2
        edges = np.unique(np.stack([E["I"], E["J"]], axis=1), axis=0).astype(np.int32)
        _ref[key] = dict(E=E, X=X, N=N, dof=dof, Sigma=Xi.T @ Xi, bSigma=bSigma, edges=edges)
    return _ref[key]


def blocks_of(Sigma, dof, pairs):
    return np.stack([Sigma[dof * p:dof * p + dof, dof * q:dof * q + dof] for p, q in pairs])


@pytest.mark.parametrize("name,nn", CASES)
def test_marginals_and_edge_blocks_against_the_dense_inverse(fixtures_dir, name, nn):
    grp = None
    for a in (0, reference(fixtures_dir, name, 0)["N"] - 1):
        R = reference(fixtures_dir, name, a)
        N, dof = R["N"], R["dof"]
        grp = grp or ops.group_of(R["E"], nn)
        marg, cross, res = grp.ml_covariance(R["X"], anchor=a, pairs=R["edges"])
        assert res.outcome == dpgo_amd.COV_OK and res.unknowns == dof * N and res.pivot_min > 0 and res.device_bytes > 0
        want_m = blocks_of(R["Sigma"], dof, [(p, p) for p in range(N)])
        want_c = blocks_of(R["Sigma"], dof, R["edges"])
        touch = (R["edges"] == a).any(axis=1)
        want_m[a] = 0
        want_c[touch] = 0
        assert not marg[a].any() and not cross[touch].any()      # the anchor's blocks: exactly zero
        em = float(np.abs(np.asarray(marg, fr.LD) - want_m).max()) / R["bSigma"]
        ec = float(np.abs(np.asarray(cross, fr.LD) - want_c).max()) / R["bSigma"]
        print("%s x %d, anchor %d: marginals %.3g, edge blocks %.3g of the bound; max|Sigma| %.3g, stationarity %.3g" %
              (name, nn, a, em, ec, np.abs(marg).max(), res.stationarity))
        assert em < 1.0 and ec < 1.0
        for p in range(N):
            assert np.array_equal(marg[p], marg[p].T)
        again = grp.ml_covariance(R["X"], anchor=a, pairs=R["edges"])
        assert np.array_equal(again[0], marg) and np.array_equal(again[1], cross)

