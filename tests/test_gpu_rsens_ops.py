"""The kernels of the robust objective's sensitivities on the device (dpgo_amd/csrc/rsens.hip: k_rsens_prep, k_rsens_edge, behind
robust.hip's edge pass and Hessian and sens.hip's right-hand sides), through NodeGroup.robust_sensitivity with want_adjoint.

Inputs (tests/robust_inputs.py), each at the point NodeGroup.robust_polish reaches from the input's own point with pose 0 fixed,
the pairs (loss, delta) chosen on the CPU (robust_restatement.polish_full converges there and the restated H is positive
definite for both anchors):
  tiny x 2           9 poses, 11 edges: fewer than 64 edges                              Huber 5, Geman-McClure 50, Welsch 50
  rand2_70 x 4       a partial last wave, parallel and reversed edges, d = 2              Huber 5, Geman-McClure 50, Welsch 50
  rand3_70 x 4       likewise, d = 3                                                      Huber 5, Geman-McClure 50, Welsch 50
  rand3_40 x 4       5 poses on 4 nodes: one-pose nodes                                   Huber 5, Welsch 0.25 (weights exactly 0)
  ladder3 x 4        200 poses, 1349 edges, a hub with 300 incidences                      Huber 50 (173 inter edges above the kink),
                     Welsch 50 (4 weights exactly 0).  The polish needs more than its default budget there: from the ground
                     truth under Huber 50 it ends MAX_STEPS after 20 and after 60 steps (|g| = 11 and 13) and CONVERGED after 209
                     (0.4 s), so max_steps = 400; the Welsch point is reached from the Huber one (230 steps).
Anchors 0 and N - 1, k = 1, 16, 17 and 65 columns: the tile edge of the block solve and the batch edge.  The 65 upstream columns
are seeded dense ones (their anchor rows are not zero), one zero column, and the unit columns of one pose.

Bounds; nothing in them comes from the device.
  lambda     bSigma |c|_1 entrywise against the long-double solve of the restated robust H (robust_restatement.reference),
             bSigma = C u kappa_2(H) / lambda_min + |bH|_2 / lambda_min^2 as tests/test_gpu_robust_covariance.py has it
  sens       tests/rsens_restatement.py: margin_rsens with that bound of lambda, against the long-double restatement at the
             long-double lambda; and, the edge kernels alone, margin_rsens with b = 0 at the DEVICE's lambda
  dloss_reg  the sum over the edges of the last entries' margins, plus num_edges roundings of the sum on its terms' magnitudes
  residual   |H lambda - c|_2 <= (C u |H|_2 + |bH|_2) |lambda|_2 per column, H the long-double restated matrix and lambda the
             DEVICE's: the same model of the factorisation (C u |H|_2) and of the matrix (bH) as bSigma, before the division by
             lambda_min that makes bSigma loose.  How loose, from the CPU restatement (the median of |lambda| / its bound, and
             of |sens| / margin_rsens with that bound): tiny 2e7 ... 8e7 and 7e4 ... 5e5; rand2_70 2e3 ... 8e3 and 28 ... 85;
             rand3_70 2e2 ... 4e3 and 0.8 ... 9.5; rand3_40 under Huber 2e4 and 3e2 ... 4e2, under Welsch 0.25 16 ... 32 and 5e-3;
             ladder3 (lambda_min = 2.4e-3 and 1.6e-4 at the two anchors, kappa_2 up to 1.4e9) 0.003 ... 0.7 and 5e-10 ... 3e-6.
             So the bound of lambda says something everywhere but on ladder3 (asserted: the median is above 10 elsewhere), and
             margin_rsens with the b-term (T(1) b: every entry of lambda off by b at once) says little on rand3_70 and nothing on
             rand3_40 under Welsch and on ladder3.  What holds the device there is the pair that carries no lambda_min: the
             residual for the adjoint, and the b = 0 comparison at that adjoint for the edge kernels.
  intra      the intra edges against sens_math.h on the host at the device's own lambda (sens_edge_debug): two fp64
             evaluations of one formula, each within margin_sens (b = 0) of its value
The device's worst figure per case is printed and held below 1.  Exact zeros where the device's weight is exactly 0.  Bit for
bit: a column alone, in calls of 1, 16 and 17 columns and in the reversed call; the call repeated; twice the column (on the edges
whose weight is a normal number); a zero column.

"Intra edges equal sensitivity's on the graph scaled by w" can hold only where no edge has curvature (the adjoint of the scaled
graph is H(S_w)^-1 c, without the rank-one terms): it is tested where that is so -- Huber with delta above every residual, where
the scaled graph is the graph and the bits are the trivial loss's -- and at the robust points the intra edges are held to the
restatement like every other edge.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_restatement as cr  # noqa: E402
import factor_restatement as fr  # noqa: E402
import robust_inputs as ri  # noqa: E402
import robust_restatement as rr  # noqa: E402
import rsens_restatement as rs  # noqa: E402
import sens_restatement as sn  # noqa: E402
import solve_restatement as sr  # noqa: E402

import dpgo_amd  # noqa: E402
from oracle.problem import LOSS_GM, LOSS_HUBER, LOSS_NONE, LOSS_WELSCH  # noqa: E402

pytestmark = pytest.mark.gpu

LD, U = rs.LD, rs.U
K = 65
ZERO_COL = 5
CASES = [("tiny", LOSS_HUBER, 5.0), ("tiny", LOSS_GM, 50.0), ("tiny", LOSS_WELSCH, 50.0),
         ("rand2_70", LOSS_HUBER, 5.0), ("rand2_70", LOSS_GM, 50.0), ("rand2_70", LOSS_WELSCH, 50.0),
         ("rand3_70", LOSS_HUBER, 5.0), ("rand3_70", LOSS_GM, 50.0), ("rand3_70", LOSS_WELSCH, 50.0),
         ("rand3_40", LOSS_HUBER, 5.0), ("rand3_40", LOSS_WELSCH, 0.25), ("ladder3", LOSS_HUBER, 50.0), ("ladder3", LOSS_WELSCH, 50.0)]
LOOSE = "ladder3"     # where bSigma's bound of lambda says nothing (the module's text)

_pt, _ref = {}, {}


def polished(name, loss, delta):
    """(P, graph, group, the device's robust-polished point) once per case."""
    key = (name, loss, delta)
    if key not in _pt:
        if (name, loss) == ("ladder3", LOSS_WELSCH):          # from the Huber point (the module's text)
            P, G, grp, X = polished(name, LOSS_HUBER, delta)
        else:
            P, X = ri.named(name)
            G = ri.graph(P)
            grp = ri.group(G)
        Xp, res, _, _ = grp.robust_polish(X, loss, delta, graph=G, max_steps=400 if name == "ladder3" else 60)
        assert res.outcome == dpgo_amd.POLISH_CONVERGED, (name, loss, delta, res.outcome, res.grad_final)
        _pt[key] = (P, G, grp, np.asfortranarray(Xp))
    return _pt[key]


def reference(name, loss, delta, anchor):
    """Once per (case, anchor): the restated anchored robust H in long double and its bound, the 65 columns, the long-double
    adjoints of the columns with the anchor's rows struck out, bSigma |c|_1 per column."""
    key = (name, loss, delta, anchor)
    if key not in _ref:
        P, G, grp, Xp = polished(name, loss, delta)
        N, d = P["N"], P["d"]
        dof = cr.dof_of(d)
        R = rr.reference(P, Xp, loss, delta, 1, anchor)
        ev = np.linalg.eigvalsh(np.asarray(R["H"], np.float64))
        assert ev[0] > 0                                                   # the restated H is positive definite at the point
        bSigma = cr.C * U * float(ev[-1] / ev[0]) / float(ev[0]) + float(np.linalg.norm(R["bH"], 2)) / float(ev[0]) ** 2
        rng = np.random.default_rng(100 + anchor)
        C = np.asfortranarray(rng.standard_normal((dof * N, K)))
        C[:, ZERO_COL] = 0.0
        pose = (anchor + 1 + int(rng.integers(0, N - 1))) % N
        C[:, K - dof:] = dpgo_amd.unit_upstream(N, d, pose)
        assert np.abs(C[dof * anchor:dof * anchor + dof]).min(axis=0).max() > 0
        Cz = np.array(C)
        Cz[dof * anchor:dof * anchor + dof] = 0.0
        L, kstar, _ = fr.cholesky_ld(R["H"])
        assert kstar < 0
        lam = sr.solve_cholesky_ld(R["H"], Cz, L)
        _ref[key] = dict(C=C, Cz=np.asfortranarray(Cz), lam=lam, b_lam=bSigma * np.abs(Cz).sum(axis=0), w=np.asarray(R["w"], np.float64),
                         H=R["H"], res_coef=cr.C * U * float(ev[-1]) + float(np.linalg.norm(R["bH"], 2)))
    return _ref[key]


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name,loss,delta", CASES)
def test_adjoints_and_sensitivities_against_the_restatement(name, loss, delta):
    P, G, grp, X = polished(name, loss, delta)
    N, m, dof = P["N"], len(P["I"]), cr.dof_of(P["d"])
    w_dev = grp.robust_hessian(X, loss, delta, graph=G)[5]
    for a in (0, N - 1):
        Rf = reference(name, loss, delta, a)
        res, sens, dreg, lam = grp.robust_sensitivity(X, Rf["C"], loss, delta, anchor=a, graph=G, want_adjoint=True)
        assert res.outcome == dpgo_amd.SENS_OK and res.unknowns == dof * N and res.fronts >= 1 and res.device_bytes > 0
        assert (res.columns, res.batches, res.edges) == (K, 2, m) and res.pivot_min > 0 and res.stationarity < 1e-3
        assert sens.shape == (K, m, 3 + dof) and lam.shape == (dof * N, K) and dreg.shape == (K,)
        assert not lam[dof * a:dof * a + dof].any() and not lam[:, ZERO_COL].any() and not sens[ZERO_COL].any() and dreg[ZERO_COL] == 0
        live = np.arange(K) != ZERO_COL
        worst = np.zeros(6)
        worst[0] = float(np.max(np.abs(np.asarray(lam, LD) - Rf["lam"]) / (Rf["b_lam"][None, :] + 1e-300)))
        want = np.moveaxis(rs.rsens_edge(P, X, Rf["lam"], loss, delta, LD), 1, 0)
        margin = np.moveaxis(rs.margin_rsens(P, X, np.asarray(Rf["lam"], np.float64), loss, delta, Rf["b_lam"]), 1, 0)
        assert np.all(np.isfinite(margin))
        worst[1] = float(np.max(np.abs(np.asarray(sens, LD) - want)[live] / (margin[live] + 1e-300)))
        # the edge kernels alone: at the device's own adjoints
        own = np.moveaxis(rs.rsens_edge(P, X, lam, loss, delta, LD), 1, 0)
        m0 = np.moveaxis(rs.margin_rsens(P, X, lam, loss, delta), 1, 0)
        worst[2] = float(np.max(np.abs(np.asarray(sens, LD) - own)[live] / (m0[live] + 1e-300)))
        # dL/ddelta: the sum of the last entries in edge order, in plain fp64
        want_d = np.sum(own[..., -1], axis=1)
        m_d = np.sum(m0[..., -1], axis=1) + m * U * np.sum(np.abs(np.asarray(own[..., -1], np.float64)), axis=1)
        worst[3] = float(np.max(np.abs(np.asarray(dreg, LD) - want_d)[live] / (m_d[live] + 1e-300)))
        assert np.array_equal(dreg, np.array([np.cumsum(sens[l, :, -1])[-1] for l in range(K)]))
        # the device's adjoint in the restated matrix: the residual of every column
        lam_l = np.asarray(lam, LD)
        r = np.sqrt(np.sum((Rf["H"] @ lam_l - np.asarray(Rf["Cz"], LD)) ** 2, axis=0))
        worst[4] = float(np.max(r[live] / (Rf["res_coef"] * np.sqrt(np.sum(lam_l ** 2, axis=0))[live])))
        # the intra edges against sens_math.h on the host at the device's own adjoint
        intra = ~P["inter"]
        for col in (0, 40, 64):
            host = dpgo_amd.sens_edge_debug(G, X, np.ascontiguousarray(lam[:, col]))[0]
            two = 2 * sn.margin_sens(P, X, lam[:, col])
            worst[5] = max(worst[5], float(np.max(np.abs(sens[col][intra, :-1] - host[intra]) / two[intra])))
        vac = float(np.median(np.abs(lam[:, live]) / Rf["b_lam"][None, live]))
        print("%s loss %d delta %g, anchor %d: lambda %.3g, sens %.3g, the edge kernels alone %.3g, dloss_reg %.3g, the residual %.3g, "
              "intra against the host %.3g of their bounds; median |lambda| / its bound %.3g"
              % ((name, loss, delta, a) + tuple(worst) + (vac,)))
        assert worst.max() < 1.0, worst
        assert name == LOOSE or vac > 10           # bSigma's bound is no blanket, except where the module's text says it is
        if name == "ladder3":
            assert np.bincount(np.concatenate([P["I"], P["J"]])).max() >= 300                     # the hub
            s_e = np.asarray(rr.weights(P, X, loss, delta)[0])[P["inter"]]
            assert (s_e > delta).sum() >= 100 and (s_e <= delta).sum() >= 100                     # either side of the kink
            assert loss != LOSS_WELSCH or (w_dev == 0).sum() >= 1                                 # weights exactly 0
        # the sensitivities are there to be checked: far above the edge kernels' margin on most entries of the weighted edges
        heavy = w_dev > 1e-6
        assert np.median(np.abs(sens[live][:, heavy, :-1]) / m0[live][:, heavy, :-1]) > 1e6
        assert (w_dev < 1).any() and np.median(np.abs(dreg[live]) / m_d[live]) > 1e3
        # exact zeros where the weight is exactly 0; no delta term on intra edges
        assert not sens[:, w_dev == 0].any() and not sens[:, ~P["inter"], -1].any()
        if (name, loss, delta) == ("rand3_40", LOSS_WELSCH, 0.25):
            assert (w_dev == 0).sum() >= 1


@pytest.mark.parametrize("name,loss,delta", CASES)
def test_a_columns_bits_do_not_depend_on_its_companions(name, loss, delta):
    P, G, grp, X = polished(name, loss, delta)
    N = P["N"]
    kw = dict(graph=G, want_adjoint=True)
    for a in (0, N - 1):
        Rf = reference(name, loss, delta, a)
        C = Rf["C"]
        _, sens, dreg, lam = grp.robust_sensitivity(X, C, loss, delta, anchor=a, **kw)
        for k in (1, 16, 17):                                                 # the first columns of the 65
            res, s, dr, l = grp.robust_sensitivity(X, C[:, :k], loss, delta, anchor=a, **kw)
            assert (res.columns, res.batches) == (k, 1)
            assert np.array_equal(s, sens[:k]) and np.array_equal(l, lam[:, :k]) and np.array_equal(dr, dreg[:k]), k
        for col in (40, 64):                                                  # a column of each batch alone, no adjoint asked for
            res, s, dr = grp.robust_sensitivity(X, C[:, col], loss, delta, anchor=a, graph=G)
            assert s.shape == sens[:1].shape and np.array_equal(s[0], sens[col]) and dr[0] == dreg[col], col
        _, s, dr, l = grp.robust_sensitivity(X, C[:, ::-1], loss, delta, anchor=a, **kw)
        assert np.array_equal(s[::-1], sens) and np.array_equal(l[:, ::-1], lam) and np.array_equal(dr[::-1], dreg)
        assert same(grp.robust_sensitivity(X, Rf["Cz"], loss, delta, anchor=a, **kw)[1:], (sens, dreg, lam))   # the anchor's rows zeroed
        assert same(grp.robust_sensitivity(X, C, loss, delta, anchor=a, **kw)[1:], (sens, dreg, lam))          # the call repeated
        # twice the column, twice the bits -- on every edge whose weight is a normal number.  Where a Welsch weight is about
        # to underflow (ladder3 under Welsch 50: w = 7.8e-312 and 4.9e-324 on two edges, nowhere else among the inputs) w, c
        # and with them (c / 2) phi, w o and (dw) phi are subnormal: rounded to multiples of 2^-1074 whatever their size, so
        # the results of phi and of 2 phi differ by up to 1.5 such units, times |ds| behind the fma; the host hook shows the
        # same at an exactly doubled adjoint.  Those edges are held to 4 TINY (1 + |ds|) instead
        _, s2, d2 = grp.robust_sensitivity(X, 2.0 * C[:, 7], loss, delta, anchor=a, graph=G)
        twice = 2.0 * sens[7]
        w_dev = grp.robust_hessian(X, loss, delta, graph=G)[5]
        sub = (w_dev != 0) & (w_dev < 2.0 ** -1022)
        assert not sub.any() or (name, loss) == ("ladder3", LOSS_WELSCH)
        assert np.array_equal(s2[0][~sub], twice[~sub])
        room = 4 * rr.TINY * (1 + np.abs(np.asarray(rs.ds_dtheta(P, X), np.float64)))
        assert np.all(np.abs(s2[0][sub, :-1] - twice[sub, :-1]) <= room[sub]) and np.all(np.abs(s2[0][sub, -1] - twice[sub, -1]) <= 4 * rr.TINY)
        assert d2[0] == 2.0 * dreg[7] or abs(d2[0] - 2.0 * dreg[7]) <= 8 * rr.TINY * sub.sum()


@pytest.mark.parametrize("name", ["tiny", "rand2_70", "rand3_70"])
def test_without_curvature_the_bits_are_those_of_the_trivial_loss(name):
    """Huber with delta above every residual: w = 1 and c = 0 on every edge, the graph scaled by w is the graph itself, and
    the call gives the bits of the trivial loss; the delta terms are zero.  (The trivial loss against NodeGroup.sensitivity,
    whose H is written from another matrix array: tests/test_gpu_robust_sensitivity.py.)"""
    P, G, grp, X = polished(name, LOSS_HUBER, 5.0)
    s = np.asarray(rr.weights(P, X, LOSS_HUBER, 5.0)[0])
    big = 4.0 * float(s.max())
    w = grp.robust_hessian(X, LOSS_HUBER, big, graph=G)[5]
    assert np.all(w == 1.0)
    C = reference(name, LOSS_HUBER, 5.0, 0)["C"][:, :17]
    res, sens, dreg = grp.robust_sensitivity(X, C, LOSS_HUBER, big, graph=G)
    res0, sens0, dreg0 = grp.robust_sensitivity(X, C, LOSS_NONE, graph=G)
    assert res.outcome == res0.outcome and res.outcome in (dpgo_amd.SENS_OK, dpgo_amd.SENS_NOT_PD)
    assert np.array_equal(sens, sens0) and not sens[..., -1].any() and not dreg.any() and not dreg0.any()


def test_ladder3_welsch_at_the_huber_point_is_honestly_not_positive_definite():
    """The Huber-50 critical point of ladder3 is no minimum of the Welsch objective: the restated H has lambda_min = -193."""
    P, G, grp, X = polished("ladder3", LOSS_HUBER, 50.0)
    assert np.linalg.eigvalsh(rr.hessian(P, X, LOSS_WELSCH, 50.0, 1, 0))[0] < -1.0
    C = reference("ladder3", LOSS_HUBER, 50.0, 0)["C"][:, :17]
    res, sens, dreg = grp.robust_sensitivity(X, C, LOSS_WELSCH, 50.0, graph=G)
    assert res.outcome == dpgo_amd.SENS_NOT_PD and not sens.any() and not dreg.any()
