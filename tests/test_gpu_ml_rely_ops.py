"""k_ml_rel and k_ml_rely_edge alone on the device (dpgo_debug_ml_rely_edge; dpgo_amd/csrc/ml_rely.hip, ml_rely_math.h) at n = 1,
63, 64, 65 and 130 edges -- under, at and over one wave, and more than one block of either kernel -- for d = 2 and 3 and both
signs.  The inputs are the edges of smallGrid3D (d = 3) and of the d = 2 grid with their seeded Omega_e at the isotropic polished
point (tests/test_ml_rely_host.py: point), repeated where n asks for more, led by three special ones: an edge at the anchor
(an all-zero block of joint), the edge whose Omega is scaled by 1e4, and a pendant edge, whose joint covariance is built so that
rel = Omega^-1 up to the rounding of its entries (redundancy 0, Q = I - A at rounding level: its flag is rounding's to decide).
The reference is the long-double restatement on the same fp64 inputs, the bounds tests/ml_rely_restatement.py's with
tests/test_ml_rely_host.py's constants: nothing in them comes from the device.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ml_rely_restatement as mrr  # noqa: E402
import test_ml_rely_host as tmr  # noqa: E402  (its points, comparison and constants; none of its tests is imported)

import dpgo_amd  # noqa: E402

pytestmark = pytest.mark.gpu
SIZES = [1, 63, 64, 65, 130]
LD, U = mrr.LD, mrr.U
PENDANT = 2   # its place in the inputs
_in = {}


def pendant(x, dof):
    """joint (3, dof, dof) of a pose q that hangs on p by this edge alone: H_qq = J_q' Omega J_q, so with G = -J_q^-1 J_p
    S_pq = S_pp G', S_qq = G S_pp G' + H_qq^-1 and J Sj J' = Omega^-1.  Long double, rounded to fp64."""
    Spp = x["Sj"][:dof, :dof]
    G = -mrr.inverse(x["Jj"].T @ x["Jj"]) @ x["Jj"].T @ x["Ji"]
    Sqq = G @ Spp @ G.T + mrr.inverse(x["Jj"].T @ x["Om"] @ x["Jj"])
    return np.stack([np.asarray(b, np.float64) for b in (Spp, Spp @ G.T, 0.5 * (Sqq + Sqq.T))])


def inputs(fixtures_dir, d):
    """(J, joint, Om, r) of 130 edges; the first n of them are the inputs of size n."""
    if d not in _in:
        P = tmr.point(fixtures_dir, "smallGrid3D" if d == 3 else "grid2")
        J, joint, Om, r = tmr.fp64_inputs(P)
        m = len(J)
        at_anchor = next(e for e, x in enumerate(P["edges"]) if 0 in (x["p"], x["q"]))
        free = next(e for e, x in enumerate(P["edges"]) if 0 not in (x["p"], x["q"]) and e % 5 != 0)
        order = [at_anchor, m // 2, free] + [e % m for e in range(130 - 3)]
        J, joint, Om, r = (np.ascontiguousarray(a[order]) for a in (J, joint, Om, r))
        joint[PENDANT] = pendant(P["edges"][free], P["dof"])
        assert not joint[0][0].any() or not joint[0][2].any()
        assert Om[1].max() > 1e3 * np.median(Om[:, 0, 0])
        _in[d] = (J, joint, Om, r)
    return _in[d]


@pytest.mark.parametrize("sign", [-1, 1])
@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("n", SIZES)
def test_rel_and_records_against_the_restatement_and_the_host_twin(fixtures_dir, d, n, sign):
    J, joint, Om, r = (a[:n] for a in inputs(fixtures_dir, d))
    dof = J.shape[-1]
    rel, rec = dpgo_amd.ml_rely_edge_debug(d, J, joint, Om, r, sign=sign, device=0)
    host_rel, host_rec = dpgo_amd.ml_rely_edge_debug(d, J, joint, Om, r, sign=sign)
    assert rel.shape == (n, dof, dof) and rec.shape == (n, mrr.width(d, sign))
    assert np.array_equal(rel, np.transpose(rel, (0, 2, 1)))   # symmetric bit for bit
    assert np.array_equal(rel, host_rel)                       # the host twin's bits
    worst_rel = worst = 0.0
    undecided = 0
    off = 2 if sign > 0 else 6
    for e in range(n):
        wr, w, ref, dec, same = tmr.compare(d, sign, rel[e], rec[e], J[e], joint[e], Om[e], r[e])
        worst_rel, worst = max(worst_rel, wr), max(worst, w)
        if dec:
            assert same and host_rec[e][1] == rec[e][1], (e, rec[e][1], ref["flag"], ref["pivots"])
        else:
            undecided += 1
        assert rec[e][1] in (0.0, 1.0) and np.array_equal(rec[e][off:off + dof], r[e])
        if rec[e][1] == 1:   # its zeros; the rest is filled
            assert rec[e][0] == 0 and (sign > 0 or (rec[e][5] == 0 and not rec[e][6 + dof:].any() and rec[e][2] != 0 and rec[e][4] > 0))
        else:
            assert rec[e][0] >= 0
        # host and device run one header: within the sum of both bounds of each other (the division and the square root are
        # correctly rounded on either side, so in practice the bits are the same)
        if host_rec[e][1] == rec[e][1]:
            b = mrr.bound(ref, d, tmr.CONSTANTS, tmr.CONSTANTS["rel"] * mrr.rel_margin(J[e][0], J[e][1], mrr.joint_matrix(joint[e])))[0]
            assert np.all(np.abs(host_rec[e] - rec[e]) <= 2 * b)
    print("d = %d, n = %d, sign %+d: rel %.3g and records %.3g of their bounds, %d flags left to rounding, records bit-equal to the "
          "host twin: %s" % (d, n, sign, worst_rel, worst, undecided, np.array_equal(rec, host_rec)))
    assert worst_rel <= 1.0 and worst <= 1.0
    if sign > 0:
        assert not rec[:, 1].any()
    if n > PENDANT and sign < 0:
        # the pendant edge: nothing checks it -- redundancy 0 within its bound, with the rounding of joint's entries counted in
        e = PENDANT
        Sj = mrr.joint_matrix(joint[e])
        Ja = np.abs(np.concatenate([J[e][0], J[e][1]], axis=1))
        m_rel = tmr.CONSTANTS["rel"] * mrr.rel_margin(J[e][0], J[e][1], Sj) + Ja @ (U * np.abs(np.asarray(Sj, np.float64))) @ Ja.T
        ref = mrr.record(mrr.rel_of(J[e][0], J[e][1], Sj), Om[e], r[e], d)
        b = mrr.bound(ref, d, tmr.CONSTANTS, m_rel)[0]
        print("  the pendant edge: redundancy %.3g (bound %.3g), redundancy_trans %.3g (bound %.3g), flag %d"
              % (rec[e][2], b[2], rec[e][3], b[3], rec[e][1]))
        assert abs(rec[e][2]) <= b[2] and abs(rec[e][3]) <= b[3]
    if n > 1:
        # the edge at the anchor and the edge whose Omega is scaled by 1e4 are decided and well inside
        for e in (0, 1):
            assert tmr.compare(d, sign, rel[e], rec[e], J[e], joint[e], Om[e], r[e])[3]


@pytest.mark.parametrize("sign", [-1, 1])
@pytest.mark.parametrize("d", [2, 3])
def test_an_edge_alone_and_among_129_others_has_the_same_bits(fixtures_dir, d, sign):
    J, joint, Om, r = inputs(fixtures_dir, d)
    rel, rec = dpgo_amd.ml_rely_edge_debug(d, J, joint, Om, r, sign=sign, device=0)
    for e in (0, 1, 2, 63, 64, 65, 77, 128, 129):
        one_rel, one_rec = dpgo_amd.ml_rely_edge_debug(d, J[e:e + 1], joint[e:e + 1], Om[e:e + 1], r[e:e + 1], sign=sign, device=0)
        assert np.array_equal(one_rel[0], rel[e]) and np.array_equal(one_rec[0], rec[e]), e
    again = dpgo_amd.ml_rely_edge_debug(d, J, joint, Om, r, sign=sign, device=0)
    assert np.array_equal(again[0], rel) and np.array_equal(again[1], rec)


def test_bad_arguments():
    L = dpgo_amd.lib()
    dof = 6
    J, joint, Om, r = np.zeros((1, 2, dof, dof)), np.zeros((1, 3, dof, dof)), np.eye(dof)[None].copy(), np.zeros((1, dof))
    rel, rec = np.zeros((1, dof, dof)), np.zeros((1, 6 + 2 * dof))
    p = [a.ctypes.data_as(C.POINTER(C.c_double)) for a in (J, joint, Om, r, rel, rec)]
    assert L.dpgo_debug_ml_rely_edge(0, 3, 1, -1, *p) == 0 and rec[0, 2] == dof
    for k in range(6):
        q = list(p)
        q[k] = None
        assert L.dpgo_debug_ml_rely_edge(0, 3, 1, -1, *q) == -1
    assert L.dpgo_debug_ml_rely_edge(0, 4, 1, -1, *p) == -1 and L.dpgo_debug_ml_rely_edge(0, 3, 1, 0, *p) == -1
    assert L.dpgo_debug_ml_rely_edge(0, 3, 0, -1, *p) == -1 and L.dpgo_debug_ml_rely_edge(0, 3, -1, -1, *p) == -1
    Om[0, 1, 1] = 0.0
    assert L.dpgo_debug_ml_rely_edge(0, 3, 1, -1, *p) == -1
    with pytest.raises(RuntimeError):
        dpgo_amd.ml_rely_edge_debug(3, np.zeros((0, 2, 6, 6)), np.zeros((0, 3, 6, 6)), np.zeros((0, 6, 6)), np.zeros((0, 6)), device=0)
