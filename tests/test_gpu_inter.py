"""The robust inter-edge pass (k_inter) and the objective (k_cost) operator by operator: every output of every variant of
launch_inter_update / launch_inter_iterate / launch_cost, enqueued as the iteration enqueues it (NodeGroup.debug_inter_update,
debug_inter_iterate, debug_cost), against the extended-precision restatement (tests/inter_restatement.py) at its derived
forward bounds -- per edge for the weights, per entry for the vectors, the sums at theirs -- on synthetic.inter_ladder (poses
with 0 .. 40 and 300 incidences, mixed roles, nodes of 1, 64, 65 and 70 poses, 1, 63, 64, 65 neighbour rows, residuals in every
regime of every loss), at the ground truth and at an extrapolated point, for every node, under the node's own mask and the
whole group's.  Variants that are the same arithmetic must agree bit for bit.

Paths reached: both modes; Huber, Geman-McClure, Welsch (the trivial loss never runs k_inter: its objective runs k_cost, in both
edge forms); quad; the halo copy from Znbr (Z's neighbour rows hold NaN: nobody may read them); the lazy unpack (recv / nsrc /
osrc, with delivered and undelivered rows); the fused Dfobj and |grad F|^2 against k_tangent_full; the fused extrapolation against
k_extrapolate; Df from the kept products; the fused proximal half step against k_proximal; gamma by value and from device
memory, different per node (0, 0.3, 0.999); the prefetched record chain at every length 0 .. 40 and 300.

Measured on the MI355X (worst error / bound ratio over all cases; pytest -s prints them): see DESIGN.md, "Operator tests of the
inter-edge pass".
"""
import os
import sys

import numpy as np
import pytest

import dpgo_amd
from dpgo_amd import synthetic
from oracle.problem import LOSS_GM, LOSS_HUBER, LOSS_NONE, LOSS_WELSCH, project_to_SOdn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inter_restatement as ir  # noqa: E402
import test_inter_restatement_host as host  # noqa: E402  (the graph, the points and the constants; none of its tests is imported)

pytestmark = pytest.mark.gpu

ROBUST = (LOSS_HUBER, LOSS_GM, LOSS_WELSCH)
GAMMAS = (0.0, 0.3, 0.999)
_GROUPS = {}
_RATIOS = {}


def device_group(d, loss, **opts):
    key = (d, loss, tuple(sorted(opts.items())))
    if key not in _GROUPS:
        _GROUPS.clear()    # (one group at a time on the device)
        g, _, _ = host.ladder_case(d)
        G = dpgo_amd.graph_from_edges(g["d"], g["num_poses"], g["I"], g["J"], g["R"], g["t"], g["kappa"], g["tau"], g["num_nodes"])
        opt = dpgo_amd.Options.driver(loss, True, **opts)
        assert opt.loss_reg == host.DL and opt.regularizer == host.XI
        grp = dpgo_amd.NodeGroup(G, range(g["num_nodes"]), opt)
        assert [tuple(s[:2]) for s in grp.sizes] == list(zip(synthetic.INTER_LADDER_SIZES, synthetic.INTER_LADDER_NBRS))
        _GROUPS[key] = grp
    return _GROUPS[key]


def check(tab, name, got, ref, bound, where):
    ok, worst = ir.within(got, ref, bound)
    tab[name] = max(tab.get(name, 0.0), worst)
    if not ok:
        err = np.abs(np.asarray(got, ir.LD) - ref)
        bad = np.argwhere(np.atleast_1d(err > bound))
        raise AssertionError("%s %s: %d entries beyond their bound, worst ratio %.3g, first at %s" % (name, where, len(bad), worst, bad[0]))


def report(tab, title):
    for k, v in tab.items():
        print("%s device/bound worst ratio %-14s %.3g" % (title, k, v))


def same(a, b, what):
    assert np.array_equal(a, b, equal_nan=True), what


def update_inputs(rng, Z, n0, d):
    R0 = (d + 1) * n0
    return dict(Zprev=Z + 0.01 * np.abs(Z) * rng.standard_normal(Z.shape), old=10.0 * rng.standard_normal(Z.shape),
                GX=50.0 * rng.standard_normal((R0, d)), X=np.array(Z[:R0]))


@pytest.mark.parametrize("loss", ROBUST)
@pytest.mark.parametrize("d", [3, 2])
def test_update_pass(d, loss):
    g, _, infos = host.ladder_case(d)
    grp = device_group(d, loss)
    tab = {}
    for a in range(g["num_nodes"]):
        info = infos[a]
        n0, n1 = info.n
        own = (d + 1) * n0
        rs = ir.Restatement(info, d, loss, host.DL, host.XI)
        for name, Z in host.node_points(d, a).items():
            rng = np.random.default_rng(7 + a)
            x = update_inputs(rng, Z, n0, d)
            ref = rs.update(Z, x["Zprev"], x["old"], x["GX"], x["X"])
            if name == "truth":
                c = ir.regime_counts(ref["s"], host.DL)
                assert a != 0 or min(c.values()) >= host.MIN_PER_REGIME, c
            outs = {}
            for whole in (False, True):
                where = (a, name, "all" if whole else "own")
                o = grp.debug_inter_update(a, Z, x["Zprev"], x["old"], x["GX"], x["X"], whole=whole)
                outs[whole] = o
                assert not np.any(np.isnan(o["DfE"])) and not np.any(np.isnan(o["g"]))
                check(tab, "w", o["w"], ref["w"], ref["dw"], where)
                check(tab, "DfE", o["DfE"], ref["DfE"], ref["d_DfE"], where)
                check(tab, "g", o["g"], ref["g"], ref["d_g"], where)
                check(tab, "Dfobj", o["Df"], ref["Df"], ref["d_Df"], where)
                check(tab, "sum rho", o["sums"][0], ref["sum_rho"], ref["d_sum_rho"], where)
                check(tab, "quad", o["sums"][1], ref["quad"], ref["d_quad"], where)
                check(tab, "<z, g>", o["sums"][2], ref["zg"], ref["d_zg"], where)
                check(tab, "|grad F|^2", o["sums"][4], ref["gn"], ref["d_gn"], where)
                same(o["Z_after"], Z, ("plain pass changed Z", where))
            base = outs[False]
            for k in ("DfE", "g", "w", "Df", "sums"):
                same(base[k], outs[True][k], ("own mask against :all", a, name, k))
            # the halo copy: neighbour rows from Znbr (Z's hold NaN), copied into Z on the way
            halo = grp.debug_inter_update(a, Z, x["Zprev"], x["old"], x["GX"], x["X"], Znbr=Z, sentinel=np.nan)
            for k in ("DfE", "g", "w", "Df", "sums"):
                same(base[k], halo[k], ("halo against plain", a, name, k))
            same(halo["Z_after"], Z, ("halo copy into Z", a, name))
            same(halo["Znbr_after"], Z, ("halo left Znbr", a, name))
            # the lazy unpack: two rows in three are delivered (in reversed order in the buffer), their Znbr rows hold NaN
            nsrc = np.where(np.arange(n1) % 3 == 0, -1, np.arange(n1)[::-1]).astype(np.int32)
            T, Y = ir.poses(Z, n0, n1, d)
            recv_T, recv_Y = np.full((n1, d), 7.0), np.full((n1, d, d), 7.0)
            Tn, Yn = np.array(T, np.float64), np.array(Y, np.float64)
            for r in range(n1):
                if nsrc[r] >= 0:
                    recv_T[nsrc[r]], recv_Y[nsrc[r]] = Tn[n0 + r], Yn[n0 + r]
                    Tn[n0 + r], Yn[n0 + r] = np.nan, np.nan
            Znbr = np.asarray(ir.stack(Tn, Yn, n0, n1), np.float64)
            recv = np.vstack([recv_T, recv_Y.reshape(n1 * d, d)])
            rows = rs.lazy_rows(np.concatenate([Tn[n0:, None, :], Yn[n0:]], axis=1).reshape(n1, -1), np.concatenate(
                [recv_T[:, None, :], recv_Y], axis=1).reshape(n1, -1), nsrc)
            same(rows, np.concatenate([np.asarray(T, np.float64)[n0:, None, :], np.asarray(Y, np.float64)[n0:]], axis=1).reshape(n1, -1),
                 "the restatement's lazy rows are Z's")
            for whole in (False, True):
                lazy = grp.debug_inter_update(a, Z, x["Zprev"], x["old"], x["GX"], x["X"], Znbr=Znbr, recv=recv, nsrc=nsrc,
                                              sentinel=np.nan, whole=whole)
                for k in ("DfE", "g", "w", "Df", "sums"):
                    same(halo[k], lazy[k], ("lazy against halo", a, name, k, whole))
                same(lazy["Z_after"], Z, ("lazy: rows written to Z", a, name))
                expect = np.array(Z)
                same(lazy["Znbr_after"][own:], expect[own:], ("lazy: delivered rows written to Znbr", a, name))
            # the shapes without quad / Dfobj: the same arithmetic for what they share; Dfobj by k_tangent_full: the same bits
            first = grp.debug_inter_update(a, Z)
            for k in ("DfE", "g", "w"):
                same(base[k], first[k], ("first-iteration shape", a, name, k))
            assert first["sums"][0] == base["sums"][0] and first["sums"][2] == base["sums"][2] and first["sums"][1] == 0.0
            unf = grp.debug_inter_update(a, Z, x["Zprev"], x["old"], x["GX"], x["X"], fused_Df=False)
            for k in ("DfE", "g", "w", "Df", "sums"):
                same(base[k], unf[k], ("fused Dfobj against k_tangent_full", a, name, k))
    report(tab, "update d=%d loss=%d" % (d, loss))
    _RATIOS[("update", d, loss)] = tab


@pytest.mark.parametrize("loss", ROBUST)
@pytest.mark.parametrize("d", [3, 2])
def test_iterate_pass(d, loss):
    g, _, infos = host.ladder_case(d)
    grp = device_group(d, loss)
    L = g["num_nodes"]
    tab = {}
    for a in range(L):
        info = infos[a]
        n0, n1 = info.n
        own = (d + 1) * n0
        rs = ir.Restatement(info, d, loss, host.DL, host.XI)
        for name, Z in host.node_points(d, a).items():
            rng = np.random.default_rng(70 + a)
            for shift in range(3):
                gam = np.array([GAMMAS[(b + shift) % 3] for b in range(L)])
                gamma = float(gam[a])
                Zp = Z + 0.05 * rng.standard_normal(Z.shape)
                GXc, GXp, Xref = ir.iterate_inputs(rs, rng, Z, Zp, gamma)
                ref = rs.iterate(Z, Zp, gamma, GXc, GXp, prox=True)
                M = np.asarray(ref["M"], np.float64)
                sv = np.linalg.svd(M, compute_uv=False)
                assert np.all(sv[:, -1] >= 1e-3 * sv[:, 0]), ("proximal conditioning", a, name)
                Rp = project_to_SOdn(M.reshape(n0 * d, d), d)
                where = (a, name, gamma)
                run = lambda **kw: grp.debug_inter_iterate(a, Z, Zp, gam, GXc, GXp, Xref, **kw)
                fused = run()                               # fused extrapolation, Df from the kept products
                check(tab, "Y", fused["Y"][:own], ref["Y"][:own], ref["d_Y"][:own], where)
                check(tab, "g(Y)", fused["g"], ref["g"], ref["d_g"], where)
                check(tab, "Df(Y)", fused["Df"], ref["Df"], ref["d_Df"], where)
                check(tab, "<Y, g>", fused["sums"][0], ref["zg"], ref["d_zg"], where)
                prox = run(prox=True)                       # ... and the proximal half step on it
                same(prox["g"], fused["g"], ("fused proximal: g", where))
                same(prox["Y"][:own], fused["Y"][:own], ("fused proximal: Y", where))
                assert prox["sums"][0] == fused["sums"][0]
                check(tab, "proximal R", prox["Xout"][n0:], Rp, np.full(Rp.shape, 1e-12), where)
                Rd = prox["Xout"][n0:].reshape(n0, d, d)
                check(tab, "proximal t", prox["Xout"][:n0], ref["prox_t"](Rd), ref["prox_t_bound"](Rd), where)
                same(prox["Xref_after"], rs.xref_after(Xref, prox["Xout"], n0), ("Xref after the proximal step", where))
                dd = np.asarray(prox["Xout"], ir.LD) - np.asarray(Xref, ir.LD)
                sq = float(np.sum(dd * dd))
                # |Xout - Xref|^2 from the device's own Xout: (d+1) d subtractions and fused multiply-adds per pose, the reduction
                assert abs(prox["sums"][1] - sq) <= (ir.gam((d + 1) * d + 2) + n0 * ir.U) * sq, ("|Xout - Xref|^2", where)
                # the un-fused launches (k_extrapolate over all rows, the pass on Y, k_proximal): the same bits
                unf = run(fused=False, prox=True)
                check(tab, "Y", unf["Y"], ref["Y"], ref["d_Y"], where)
                same(unf["Y"][:own], fused["Y"][:own], ("fused extrapolation against k_extrapolate", where))
                for k in ("g", "Df"):
                    same(unf[k], fused[k], ("fused pass against un-fused launches", k, where))
                for k in ("Xout", "Xref_after", "sums"):
                    same(unf[k], prox[k], ("fused proximal step against k_proximal", k, where))
                # gamma from device memory (the by-value ones are wrong on purpose), and the whole group's mask
                for kw in (dict(gamma_dev=True), dict(whole=True), dict(gamma_dev=True, whole=True, prox=True)):
                    o = run(**kw)
                    for k in ("g", "Df", "sums") if not kw.get("prox") else ("g", "Xout", "Xref_after", "sums"):
                        same(o[k], (prox if kw.get("prox") else fused)[k], ("variant", kw, k, where))
                    same(o["Y"][:own], fused["Y"][:own], ("variant", kw, "Y", where))
    report(tab, "iterate d=%d loss=%d" % (d, loss))
    _RATIOS[("iterate", d, loss)] = tab


@pytest.mark.parametrize("loss", (LOSS_NONE,) + ROBUST)
@pytest.mark.parametrize("d", [3, 2])
def test_cost(d, loss):
    g, _, infos = host.ladder_case(d)
    grp = device_group(d, loss)
    tab = {}
    for a in range(g["num_nodes"]):
        info = infos[a]
        rs = ir.Restatement(info, d, loss, host.DL, host.XI)
        for name, Z in host.node_points(d, a).items():
            ref0 = rs.cost(Z, 0)
            c0 = grp.debug_cost(a, Z, eform=False)
            same(c0, grp.debug_cost(a, Z, eform=False, whole=True), ("cost: own mask against :all", a, name))
            for q in range(2):
                check(tab, "cost slot %d" % q, c0[q], ref0[q][0], ref0[q][1], (a, name))
            ref1 = rs.cost(Z, 1)
            c1 = grp.debug_cost(a, Z, eform=True)
            for q in range(2):
                check(tab, "cost eform slot %d" % q, c1[q], ref1[q][0], ref1[q][1], (a, name))
            if name == "truth":    # the two edge forms agree at orthonormal rotations
                for q in range(2):
                    check(tab, "eform 1 against 0", c1[q], ir.LD(c0[q]), ref0[q][1] + ref1[q][1], (a, name))
            if loss != LOSS_NONE:  # the rho slot is slot 0 of the update pass
                up = grp.debug_inter_update(a, Z)
                ref = rs.update(Z)
                check(tab, "rho slot against update", c0[1], ir.LD(up["sums"][0]), ref["d_sum_rho"] + ref0[1][1], (a, name))
    report(tab, "cost d=%d loss=%d" % (d, loss))


def test_groups_released():
    _GROUPS.clear()
