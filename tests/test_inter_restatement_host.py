"""The restatement of the inter-edge pass, the objective and the Dynamic rescale (tests/inter_restatement.py) held to the fp64
oracle, and its bounds held honest in both directions, on the inputs the GPU tests use (synthetic.inter_ladder); no GPU.

  not too tight:  the oracle's evaluate_E, evaluate_g, evaluate_g_and_f0, evaluate_g_and_f, proximal, _maybe_rescale and
                  assemble_node(..., scale) lie within the restatement's bounds (the worst error / bound ratio per quantity is
                  printed: pytest -s)
  tight enough:   every mutant of inter_restatement.MUTANTS -- the restatement wrong in one ingredient -- violates a bound in at
                  least one entry
"""
import os
import sys

import numpy as np
import pytest

from dpgo_amd import synthetic
from oracle import g2o as og
from oracle.problem import DPGOProblem, LOSS_GM, LOSS_HUBER, LOSS_NONE, LOSS_WELSCH, project_to_SOdn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inter_restatement as ir  # noqa: E402
from inter_restatement import LD  # noqa: E402

DL, XI = 0.25, 1e-11           # Options.driver(): loss_reg and the regulariser
LOSSES = (LOSS_NONE, LOSS_HUBER, LOSS_GM, LOSS_WELSCH)
MIN_PER_REGIME = 5
_CACHE = {}


def ladder_case(d):
    if d not in _CACHE:
        g = synthetic.inter_ladder(d)
        meas = ir.node_measurements(g)
        infos = [og.generate_data_info(a, meas[a]) for a in range(g["num_nodes"])]
        _CACHE[d] = (g, meas, infos)
    return _CACHE[d]


def node_points(d, a):
    """The two points of node a: the ground truth and an extrapolated one."""
    g, _, infos = ladder_case(d)
    info = infos[a]
    Zt = ir.truth_point(g, info, a, synthetic.INTER_LADDER_SPAN)
    Zx = ir.extrapolated_point(np.random.default_rng(1000 + 10 * d + a), Zt, info.n[0], info.n[1], d)
    return {"truth": Zt, "extrapolated": Zx}


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [3, 2])
def test_inter_ladder_reaches_the_edges(d):
    g, meas, infos = ladder_case(d)
    assert [i.n[0] for i in infos] == list(synthetic.INTER_LADDER_SIZES)
    assert [i.n[1] for i in infos] == list(synthetic.INTER_LADDER_NBRS)
    rs = [ir.Restatement(infos[a], d, LOSS_HUBER, DL, XI) for a in range(4)]
    E0 = rs[0].inter
    n0 = infos[0].n[0]
    assert list(rs[0].ninc[:synthetic.INTER_LADDER_TOP + 1]) == list(range(synthetic.INTER_LADDER_TOP + 1))
    assert rs[0].hub == synthetic.INTER_LADDER_HUB and rs[0].ninc[rs[0].hub] == synthetic.INTER_LADDER_HUB_INCIDENCES
    assert E0.m > 2 * 256
    for p in (63, 64, 65, n0 - 1):
        assert rs[0].ninc[p] > 0
    # roles mixed within a pose of node 0; node 2 all head, node 3 all tail
    for p in list(range(2, synthetic.INTER_LADDER_TOP + 1)) + [rs[0].hub]:
        assert np.any(E0.i == p) and np.any(E0.j == p), p
    assert np.all(rs[2].inter.j < infos[2].n[0]) and np.all(rs[2].inter.i >= infos[2].n[0])
    assert np.all(rs[3].inter.i < infos[3].n[0]) and np.all(rs[3].inter.j >= infos[3].n[0])
    pairs = list(zip(E0.i.tolist(), E0.j.tolist()))
    assert len(set(pairs)) < len(pairs)                                         # parallel edges
    assert np.any(g["I"] > g["J"]) and np.any(g["I"] < g["J"])                  # written both ways
    assert np.all((g["tau"] >= 1) & (g["tau"] <= 100) & (g["kappa"] >= 1) & (g["kappa"] <= 100))
    # every regime of every loss, from the reference's own squared residuals at the ground truth (s does not depend on the loss)
    s = []
    for a in range(4):
        Z = node_points(d, a)["truth"]
        T, Y = ir.poses(Z, infos[a].n[0], infos[a].n[1], d)
        s.append(rs[a].residuals(rs[a].inter, T, Y)["s"])
    for a in range(4):
        print("d=%d node %d regimes %s" % (d, a, ir.regime_counts(s[a], DL)))
    c = ir.regime_counts(s[0], DL)      # node 0 holds every kind of edge but the 3 -> 2 ones
    for loss in LOSSES:
        for k, v in c.items():
            assert v >= MIN_PER_REGIME, (loss, k, v)


# ---------------------------------------------------------------------------------------------------------------------
def _ratio(tab, name, got, ref, bound):
    ok, worst = ir.within(got, ref, bound)
    tab[name] = max(tab.get(name, 0.0), worst)
    return ok


def _blocks_of(M, n0, d, rows=None):
    """The (d+1) x (d+1) diagonal block of every pose of a reference-layout matrix (translations first)."""
    n = n0 if rows is None else rows
    M = M.toarray()
    out = np.zeros((n0, d + 1, d + 1))
    for p in range(n0):
        idx = [p] + [n + d * p + k for k in range(d)]
        out[p] = M[np.ix_(idx, idx)]
    return out


def _q_blocks(Q, n0, n1, d):
    Q = Q.toarray()
    out = np.zeros((n0 + n1, d + 1, d + 1))
    o = (d + 1) * n0
    for p in range(n0 + n1):
        idx = [p] + [n0 + d * p + k for k in range(d)] if p < n0 else [o + p - n0] + [o + n1 + d * (p - n0) + k for k in range(d)]
        out[p] = Q[np.ix_(idx, idx)]
    return out


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("d", [3, 2])
def test_oracle_within_the_bounds(d, loss):
    g, meas, infos = ladder_case(d)
    tab = {}
    for a in range(4):
        info = infos[a]
        n0, n1 = info.n
        R0 = (d + 1) * n0
        p = DPGOProblem(a, meas[a], XI, loss, 1e6, DL, preconditioner=0)
        rs = ir.Restatement(info, d, loss, DL, XI)
        for name, Z in node_points(d, a).items():
            rng = np.random.default_rng(7 + a)
            X = Z[:R0]
            GX = p.mat.G @ X
            Zprev = Z + 0.01 * np.abs(Z) * rng.standard_normal(Z.shape)
            old = 10.0 * rng.standard_normal(Z.shape)
            ref = rs.update(Z, Zprev, old, GX, X)
            DfE, fobjE, w = p.evaluate_E(Z)
            assert _ratio(tab, "w", w, ref["w"], ref["dw"]), (a, name)
            assert _ratio(tab, "DfE", DfE, ref["DfE"], ref["d_DfE"]), (a, name)
            assert _ratio(tab, "sum rho", 2 * fobjE, ref["sum_rho"], ref["d_sum_rho"]), (a, name)
            if loss == LOSS_NONE:
                continue    # (the trivial loss has its own surrogate: the robust operators below do not exist for it)
            assert _ratio(tab, "g", p.evaluate_g(Z), ref["g"], ref["d_g"]), (a, name)
            gg, _, Dfobj, _, DfE2, _ = p.evaluate_g_and_f0(Z)
            assert _ratio(tab, "g", gg, ref["g"], ref["d_g"]) and _ratio(tab, "DfE", DfE2, ref["DfE"], ref["d_DfE"])
            assert _ratio(tab, "Dfobj", Dfobj, ref["Df"], ref["d_Df"]), (a, name)
            assert _ratio(tab, "<z, g>", float(np.sum(X * gg)), ref["zg"], ref["d_zg"]), (a, name)
            grad = p.full_tangent_space_projection(X, Dfobj)
            assert _ratio(tab, "|grad F|^2", float(np.sum(grad * grad)), ref["gn"], ref["d_gn"]), (a, name)
            # evaluate_g_and_f: with G = fobjE0 = 0 its fobj is 1/2 fobjE - 1/2 quad
            g3, _, Df3, fobj, _, fobjE3 = p.evaluate_g_and_f(Z, Zprev, 0.0, old, 0.0)
            assert _ratio(tab, "g", g3, ref["g"], ref["d_g"]) and _ratio(tab, "Dfobj", Df3, ref["Df"], ref["d_Df"])
            quad = float(np.sum((Z - Zprev) * (old + 0.5 * (p.mat.Q @ (Z - Zprev)))))
            assert fobj == 0.0 - 0.5 * 0.0 - 0.5 * quad + 0.5 * fobjE3
            assert _ratio(tab, "quad", quad, ref["quad"], ref["d_quad"]), (a, name)
            # the iterate pass at an extrapolated point, and the proximal step on its Df
            for gamma in (0.0, 0.3, 0.999):
                Zp = Z + 0.05 * rng.standard_normal(Z.shape)
                GXc, GXp, Xref = ir.iterate_inputs(rs, rng, Z, Zp, gamma)
                it = rs.iterate(Z, Zp, gamma, GXc, GXp, prox=True)
                Yo = Z + gamma * (Z - Zp)
                # (numpy has no fused multiply-add: its gamma (a - b) rounds once more than the device's, u |gamma (a - b)|)
                assert _ratio(tab, "Y", Yo, it["Y"], it["d_Y"] + ir.U * np.abs(gamma * (Z - Zp))), (a, name, gamma)
                go = p.evaluate_g(Yo)
                # (the oracle evaluates at ITS rounded Y: the same bound, the point's rounding being part of it)
                assert _ratio(tab, "g(Y)", go, it["g"], it["d_g"]), (a, name, gamma)
                Dfo = go + (GXc + gamma * (GXc - GXp))
                assert _ratio(tab, "Df(Y)", Dfo, it["Df"], it["d_Df"] + ir.U * np.abs(gamma * (GXc - GXp))), (a, name, gamma)
                Xo = p.proximal(Yo, Dfo)
                M = np.asarray(it["M"], np.float64)
                sv = np.linalg.svd(M, compute_uv=False)
                assert np.all(sv[:, -1] >= 1e-3 * sv[:, 0]), ("proximal conditioning", a, name)
                Rp = project_to_SOdn(M.reshape(n0 * d, d), d)
                assert _ratio(tab, "proximal R", Xo[n0:], Rp, np.full(Rp.shape, 1e-12)), (a, name, gamma)
                assert _ratio(tab, "proximal t", Xo[:n0], it["prox_t"](Xo[n0:].reshape(n0, d, d)),
                              it["prox_t_bound"](Xo[n0:].reshape(n0, d, d))), (a, name, gamma)
            # the objective: the rho slot is the update pass's, both edge forms agree at orthonormal rotations
            c0 = rs.cost(Z, 0)
            assert _ratio(tab, "cost rho", float(c0[1][0]), ref["sum_rho"], ref["d_sum_rho"] + c0[1][1])
            if name == "truth":
                c1 = rs.cost(Z, 1)
                for q in range(2):
                    assert _ratio(tab, "cost eform", float(c1[q][0]), c0[q][0], c0[q][1] + c1[q][1]), (a, q)
        if loss == LOSS_NONE:
            continue
        # Rescale::Dynamic: the decision, and the rescaled surrogate's block-diagonal terms
        pd = DPGOProblem(a, meas[a], XI, loss, 1e6, DL, preconditioner=0, dynamic=True)
        m1 = info.m[1]
        for w, count, maxc in _rescale_cases(np.random.default_rng(50 + a), m1):
            pd.scale = np.ones(m1) * 0.5
            before = pd.scale.copy()
            flag, sc, cnt = ir.rescale_decide(w, before, count, maxc)
            new_count = pd._maybe_rescale(w, count, maxc)
            assert new_count == cnt and np.array_equal(pd.scale, sc) and flag == (0 if cnt == count + 1 else 1)
        scale = np.random.default_rng(60 + a).uniform(0.01, 1.0, m1)
        pd.update_quadratic_mat(scale)
        bl = rs.blocks(scale, dynamic=True)
        assert _ratio(tab, "D blocks", _blocks_of(pd.mat.D, n0, d), bl["D"], bl["dD"])
        assert _ratio(tab, "G blocks", _blocks_of(pd.mat.G, n0, d), bl["Gd"], bl["dGd"])
        assert _ratio(tab, "H blocks", _blocks_of(pd.mat.H, n0, d), bl["H"], bl["dH"])
        assert _ratio(tab, "Q blocks", _q_blocks(pd.mat.Q, n0, n1, d), bl["Q"], bl["dQ"])
    for k, v in tab.items():
        print("d=%d loss=%d oracle/bound worst ratio %-12s %.3g" % (d, loss, k, v))


def _rescale_cases(rng, m1):
    """(weights, counter, max counter): against scales of 0.5 everywhere."""
    eq = np.full(m1, 0.5)
    above = eq.copy()
    above[-1] = np.nextafter(0.5, 1.0)      # (the last edge: beyond index 256 on node 0)
    low = rng.uniform(0.0, 0.5, m1)
    low[0], low[-1] = 1e-4, 0.5             # clamps at 0.01 ...
    high = rng.uniform(0.5, 1.0, m1)        # ... and at 1
    return [(eq, 0, 5), (above, 0, 5), (eq, 5, 5), (eq, 4, 5), (low, 0, 5), (low, 5, 5), (high, 1, 5)]


# ---------------------------------------------------------------------------------------------------------------------
def _battery(rs, Z, inp, mut=None):
    """Every quantity the GPU tests compare, as {name: (value, bound)}, from the restatement (or a mutant of it)."""
    d, n0, n1 = rs.d, rs.n0, rs.n1
    out = {}
    nbr = inp["Znbr_rows"]
    rows = rs.lazy_rows(nbr, inp["recv"], inp["nsrc"], mut)
    out["lazy rows"] = (rows, np.zeros(rows.shape))
    up = rs.update(Z, inp["Zprev"], inp["old"], inp["GX"], Z[:(d + 1) * n0], scale=inp["scale"], dynamic=True, mut=mut)
    for k in ("w", "rho"):
        out[k] = (up[k], up["d" + k])
    for k in ("DfE", "g", "sum_rho", "quad", "zg", "Df", "gn"):
        out[k] = (up[k], up["d_" + k])
    it = rs.iterate(Z, inp["Zp"], inp["gamma"], inp["GXc"], inp["GXp"], prox=True, gamma_other=inp["gamma_other"], mut=mut)
    for k in ("Y", "g", "zg", "Df"):
        out["it " + k] = (it[k], it["d_" + k])
    Rp = project_to_SOdn(np.asarray(it["M"], np.float64).reshape(n0 * d, d), d)
    Xout = np.vstack([np.asarray(it["prox_t"](Rp.reshape(n0, d, d)), np.float64), Rp])
    xr = rs.xref_after(inp["Xref"], Xout, n0, mut)
    out["Xref"] = (xr, np.full(xr.shape, 1e-12))
    bl = rs.blocks(inp["scale"], True, mut)
    for k in ("D", "Q", "H"):
        out[k + " blocks"] = (bl[k], bl["d" + k])
    for q, (w, count, maxc) in enumerate(inp["rescale"]):
        flag, sc, cnt = ir.rescale_decide(w, np.full(len(w), 0.5), count, maxc, mut)
        out["rescale %d" % q] = (np.concatenate([[flag, cnt], sc]), np.zeros(2 + len(sc)))
    return out


@pytest.mark.parametrize("mut", ir.MUTANTS)
def test_every_mutant_violates_a_bound(mut):
    d, a = 3, 0
    loss = LOSS_GM if mut.startswith("gm") else LOSS_HUBER
    g, meas, infos = ladder_case(d)
    info = infos[a]
    n0, n1 = info.n
    rs = ir.Restatement(info, d, loss, DL, XI)
    Z = node_points(d, a)["truth"]
    rng = np.random.default_rng(99)
    Zp = Z + 0.05 * rng.standard_normal(Z.shape)
    gamma = 0.3
    GXc, GXp, Xref = ir.iterate_inputs(rs, rng, Z, Zp, gamma)
    T, Y = ir.poses(Z, n0, n1, d)
    nbr = np.asarray(np.concatenate([T[n0:, None, :], Y[n0:]], axis=1), np.float64).reshape(n1, -1)
    nsrc = np.where(np.arange(n1) % 3 == 0, -1, np.arange(n1)[::-1]).astype(np.int32)
    inp = dict(Zprev=Z + 0.01 * np.abs(Z) * rng.standard_normal(Z.shape), old=10.0 * rng.standard_normal(Z.shape),
               GX=50.0 * rng.standard_normal(((d + 1) * n0, d)), Zp=Zp, gamma=gamma, gamma_other=0.999, GXc=GXc, GXp=GXp, Xref=Xref,
               Znbr_rows=nbr + 1.0, recv=nbr, nsrc=nsrc, scale=rng.uniform(0.01, 1.0, info.m[1]),
               rescale=_rescale_cases(rng, info.m[1]))
    base = _battery(rs, Z, inp)
    bad = _battery(rs, Z, inp, mut)
    caught = []
    for k, (ref, bound) in base.items():
        ok, worst = ir.within(bad[k][0], np.asarray(ref, LD), bound)
        if not ok:
            caught.append((k, worst))
    print("mutant %-18s caught by %s" % (mut, ", ".join("%s (x%.3g)" % c for c in caught)))
    assert caught, mut
