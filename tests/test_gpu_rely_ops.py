"""k_rely_edge alone on the device (dpgo_debug_rely_edge; dpgo_amd/csrc/rely.hip, rely_math.h) at m = 1, 63, 64, 65 and 130 edges
-- under, at and over one wave, and three blocks -- for d = 2 and 3, on seeded inputs: residual covariances C = Q diag Q^T
with kappa_2 up to 1e6, one C with a negative eigenvalue (flag 1) and one edge without weight (flag 2) in every call that has
room for them.  The reference is the long-double restatement on the same fp64 inputs, the bounds are
tests/rely_restatement.py's margins for exact inputs: nothing in them comes from the device.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_restatement as cr  # noqa: E402
import pairs_restatement as pr  # noqa: E402
import rely_restatement as rr  # noqa: E402
import test_rely_host as trh  # noqa: E402  (its comparison; none of its tests is imported)

import dpgo_amd  # noqa: E402

pytestmark = pytest.mark.gpu
SIZES = [1, 63, 64, 65, 130]


def inputs(d, m, seed):
    """(rel, r, kappa, tau, the flag every record must carry): entry m // 2 is flag 1 and entry m - 1 flag 2 where m >= 3."""
    dof = cr.dof_of(d)
    rng = np.random.default_rng(seed)
    rel, r, kappa, tau, flag = [], [], [], [], []
    for e in range(m):
        Q = np.linalg.qr(rng.standard_normal((dof, dof)))[0]
        k, t = float(rng.uniform(5, 50)), float(rng.uniform(5, 50))
        lam = 0.02 * np.logspace(0, -2 * (e % 4), dof)
        f = 0
        if m >= 3 and e == m // 2:
            lam[int(rng.integers(0, dof))] = -0.01
            f = 1
        if m >= 3 and e == m - 1:
            k, f = 0.0, 2
        Cm = (Q * lam) @ Q.T
        rel.append(np.diag(1 / np.diag(pr.omega(d, k if k > 0 else 1.0, t))) - (Cm + Cm.T) / 2)
        r.append(rng.standard_normal(dof) * 0.1)
        kappa.append(k), tau.append(t), flag.append(f)
    return np.stack(rel), np.stack(r), np.array(kappa), np.array(tau), np.array(flag)


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("m", SIZES)
def test_records_against_the_restatement(d, m):
    dof = cr.dof_of(d)
    rel, r, kappa, tau, flag = inputs(d, m, 100 * d + m)
    rec = dpgo_amd.rely_edge_debug(d, rel, r, kappa, tau, device=0)
    assert rec.shape == (m, 6 + 2 * dof) and np.array_equal(rec[:, 1], flag.astype(float))
    worst = 0.0
    for e in range(m):
        w, ref, same = trh.compare(d, rec[e], rel[e], r[e], kappa[e], tau[e])
        assert same and ref["flag"] == flag[e]
        worst = max(worst, w)
        if flag[e] == 1:   # its zeros; the rest is filled
            assert rec[e][0] == 0 and rec[e][5] == 0 and not rec[e][6 + dof:].any()
            assert rec[e][2] != 0 and rec[e][4] > 0 and np.array_equal(rec[e][6:6 + dof], r[e])
        if flag[e] == 2:
            assert not rec[e][0] and not rec[e][2:].any()
        if flag[e] == 0:
            assert rec[e][0] > 0 and np.array_equal(rec[e][6:6 + dof], r[e])
    print("d = %d, m = %d: worst error / margin %.3g" % (d, m, worst))
    assert worst <= 1.0
    # the host twin runs the same header: the same flags, and values within twice the margins of each other
    host = dpgo_amd.rely_edge_debug(d, rel, r, kappa, tau)
    assert np.array_equal(host[:, 1], rec[:, 1])
    for e in range(m):
        ref = rr.record(rel[e], r[e], d, kappa[e], tau[e])
        assert np.all(np.abs(host[e] - rec[e]) <= 2 * rr.margins(ref, rel[e], d, kappa[e], tau[e]))


@pytest.mark.parametrize("d", [2, 3])
def test_an_edge_alone_and_among_129_others_has_the_same_bits(d):
    rel, r, kappa, tau, flag = inputs(d, 130, 7 + d)
    many = dpgo_amd.rely_edge_debug(d, rel, r, kappa, tau, device=0)
    for e in (0, 63, 64, 65, 77, 128, 129):
        alone = dpgo_amd.rely_edge_debug(d, rel[e:e + 1], r[e:e + 1], kappa[e:e + 1], tau[e:e + 1], device=0)
        assert np.array_equal(alone[0], many[e]), e
    assert np.array_equal(many, dpgo_amd.rely_edge_debug(d, rel, r, kappa, tau, device=0))


def test_bad_arguments():
    with pytest.raises(RuntimeError):
        dpgo_amd.rely_edge_debug(3, np.zeros((0, 6, 6)), np.zeros((0, 6)), [], [], device=0)
    import ctypes as C
    L = dpgo_amd.lib()
    a = np.zeros(40)
    dp = a.ctypes.data_as(C.POINTER(C.c_double))
    assert L.dpgo_debug_rely_edge(0, 3, 1, None, dp, dp, dp, dp) == -1 and L.dpgo_debug_rely_edge(0, 3, 1, dp, dp, dp, dp, None) == -1
    assert L.dpgo_debug_rely_edge(0, 4, 1, dp, dp, dp, dp, dp) == -1
