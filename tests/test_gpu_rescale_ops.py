"""Rescale::Dynamic on the device operator by operator (k_rescale_decide, k_rescale_apply, and the refactorisation and repack
behind them: NodeGroup.debug_rescale runs launch_rescale_decide and rescale_device() as update() does).

  decide  against the oracle's _maybe_rescale and the restatement's rescale_decide, exactly (one product and two comparisons per
          edge in fp64): w == scale on every edge; one edge one ulp above its scale beyond index 256 of the node's edges (the second
          trip of the strided loops); the counter at max_count and at max_count - 1; the clamps at 0.01 and 1; a node outside the
          set (scales, counter and operators unchanged bit for bit, flag 0).
  apply   a group built with rescale = 1; after a rescale to random scales in [0.01, 1] the operators that read what
          k_rescale_apply rewrote -- G (the diagonal blocks inside the interleaved rounds, the t-column copy), solve_tt (the
          diagonal of G_tt the factorisation reads), proximal (T, N, V), retract -- against the oracle's rescaled matrices
          (tests/test_gpu_operators.py: Ref with `scale`) at test_gpu_operators.py's bounds (G's with the assembly term its
          _prod_bound leaves out: assembly_term_G), and g and the quad slot of the update
          pass (D; Q on own and neighbour rows) against the restatement's at its bounds.  A flagged and an unflagged node in one
          launch, and a second rescale on top of the first.
  shapes  the iterate pass of a dynamically rescaled group (no kept products): fused extrapolation and the plain pass on an
          extrapolated Y agree bit for bit and lie within the restatement's bounds.
"""
import os
import sys

import numpy as np
import pytest

import dpgo_amd
from oracle.problem import DPGOProblem, LOSS_HUBER, project_to_SOdn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inter_restatement as ir  # noqa: E402
import test_gpu_inter as gi  # noqa: E402  (device_group, check, same; none of its tests is imported)
import test_gpu_operators as ops  # noqa: E402  (Ref, its inputs and bounds; none of its tests is imported)
import test_inter_restatement_host as host  # noqa: E402

pytestmark = pytest.mark.gpu

LOSS = LOSS_HUBER
MAXC = 5


def dynamic_group(d):
    return gi.device_group(d, LOSS, rescale=dpgo_amd.RESCALE_DYNAMIC, max_rescale_count=MAXC)


def node_slices(grp):
    off = grp.debug_edge_offsets()
    return [slice(int(off[a]), int(off[a + 1])) for a in range(len(off) - 1)]


def expect_decide(meas, w, scale, count, maxc, nodes, sl):
    """Per node: (flag, scales, counter) by the restatement, cross-checked with the oracle's _maybe_rescale."""
    out = []
    for a in range(len(sl)):
        if a not in nodes:
            out.append((0, scale[sl[a]].copy(), int(count[a])))
            continue
        flag, sc, cnt = ir.rescale_decide(w[sl[a]], scale[sl[a]], int(count[a]), maxc)
        p = object.__new__(DPGOProblem)      # (the test and the clamp only: no matrices)
        p.scale = scale[sl[a]].copy()
        p.update_quadratic_mat = lambda s, p=p: setattr(p, "scale", np.asarray(s, np.float64).copy())
        assert p._maybe_rescale(w[sl[a]], int(count[a]), maxc) == cnt and np.array_equal(p.scale, sc)
        out.append((flag, sc, cnt))
    return out


@pytest.mark.parametrize("d", [3, 2])
def test_rescale_decide(d):
    g, meas, infos = host.ladder_case(d)
    grp = dynamic_group(d)
    sl = node_slices(grp)
    L, m = len(sl), sl[-1].stop
    assert [s.stop - s.start for s in sl] == [i.m[1] for i in infos] and sl[0].stop - sl[0].start > 2 * 256
    rng = np.random.default_rng(5)
    half = np.full(m, 0.5)
    above0 = half.copy()
    above0[sl[0].stop - 1] = np.nextafter(0.5, 1.0)          # node 0's last edge, beyond index 256 of its edges
    low = rng.uniform(0.0, 0.5, m)
    high = rng.uniform(0.5, 1.0, m)
    for s in sl:
        low[s.start], low[s.stop - 1] = 1e-4, 0.5            # clamped at 0.01; equal to its scale
        high[s.stop - 1] = 0.9                               # clamped at 1
    every = list(range(L))
    cases = [
        ("w == scale on every edge", half, [0] * L, every),
        ("one edge one ulp above", above0, [0] * L, every),
        ("count == max_count / max_count - 1", half, [MAXC, MAXC - 1, MAXC + 1, 0], every),
        ("clamp at 0.01, by the counter", low, [MAXC] * L, every),
        ("below everywhere, no rescale", low, [1] * L, every),
        ("clamp at 1", high, [0] * L, every),
        ("nodes outside the set", high, [MAXC, MAXC, 0, 0], [0, 2]),
    ]
    for what, w, count, nodes in cases:
        G_before = {a: grp.debug_apply(a, "G", np.random.default_rng(a).standard_normal(((d + 1) * infos[a].n[0], d)),
                                       (d + 1) * infos[a].n[0]) for a in range(L)}
        count = np.asarray(count, np.int32)
        exp = expect_decide(meas, w, half, count, MAXC, nodes, sl)
        o = grp.debug_rescale(w, half, count, MAXC, nodes)
        assert o["rescaled"] == sum(e[0] for e in exp), what
        for a in range(L):
            flag, sc, cnt = exp[a]
            assert o["flags"][a] == flag and o["host_flags"][a] == float(flag), (what, a)
            gi.same(o["scale"][sl[a]], sc, (what, a, "scales"))
            assert o["count"][a] == cnt, (what, a, o["count"][a], cnt)
            G_after = grp.debug_apply(a, "G", np.random.default_rng(a).standard_normal(((d + 1) * infos[a].n[0], d)),
                                      (d + 1) * infos[a].n[0])
            if not flag:
                gi.same(G_after, G_before[a], (what, a, "an unflagged node's operator changed"))
    assert exp[1][0] == 0 and exp[3][0] == 0 and exp[0][0] == 1     # (the last case: nodes 1 and 3 outside the set)


def assembly_term_G(bl, X, n0, d):
    """What test_gpu_operators._prod_bound leaves out.  It charges the assembly of an entry of G with k u |G_rc| -- right where the
    terms of an entry share a sign.  On inter_ladder they do not: a pose with dozens of incidences sums tau t_r t_c (and tau t_r) of
    either sign, |G_rc| is far below the sum of |terms|, and two fp64 assemblies in different orders (the oracle's, the
    library's) differ by k u sum |terms|.  Measured: the library's HOST-assembled G of node 3 (d = 3) against the oracle's misses
    _prod_bound by 1.82 x at row 97 on the `mixed` input, on a CPU, with Static and Dynamic rescale alike, before any kernel has
    run.  The term: both assemblies' entrywise bound on the diagonal blocks (the restatement's dGd = gamma_{k+5} sum |terms|,
    inter_restatement.blocks) carried through |X|.  Off-diagonal blocks hold one edge's terms (or a parallel pair's): no such sum."""
    dG = np.asarray(bl["dGd"], np.float64)
    zm = np.concatenate([np.abs(X[:n0])[:, None, :], np.abs(X[n0:]).reshape(n0, d, d)], axis=1)
    e = 2 * np.einsum("prk,pkc->prc", dG, zm)
    return np.vstack([e[:, 0], e[:, 1:].reshape(n0 * d, d)])


def check_rescaled_ops(ref, x, out, bl, tab):
    """test_gpu_operators.check_ops' statements for G, solve_tt, retract and proximal, at its bounds (G's with the assembly term
    of assembly_term_G; the worst ratio against the bound WITHOUT it is recorded too)."""
    d, n0 = ref.d, ref.n0
    U = ops.U
    for k in ("Y", "const", "mixed"):
        err = np.abs(out["G/" + k] - ref.G @ x[k])
        bound = ops._prod_bound(ref.G, x[k], terms=ref.terms)
        tab["G (_prod_bound alone)"] = max(tab.get("G (_prod_bound alone)", 0.0), float((err / np.maximum(bound, 1e-300)).max()))
        bound = bound + assembly_term_G(bl, x[k], n0, d)
        tab["G"] = max(tab.get("G", 0.0), float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound), ("G", k, err.max(), (err / np.maximum(bound, 1e-300)).max())
    for k in ("Y", "mixed"):
        ref.check_solve(ref.Gtt, ref.p.L, ref.kappa_tt, x[k][:n0], out["solve_tt/" + k][:n0], "solve_tt/" + k)
    R = x["Y"][n0:]
    T = out["retract"]
    Rp = project_to_SOdn(R + x["Ydot"][n0:], d)
    assert np.abs(T[n0:] - Rp).max() <= 1e-12
    tref = ref.p.recover_translations(T[n0:], x["g"])
    e_t = ref.tdot_bound(ops._prod_bound(ref.GtR, T[n0:], x["g"][:n0], ref.terms[:n0]), tref)
    assert np.linalg.norm(T[:n0] - tref) <= e_t, ("retract t", np.linalg.norm(T[:n0] - tref), e_t)
    Z, Df = x["Z"], x["Dfp"]
    t0, R0z = Z[:n0], Z[n0:n0 + d * n0]
    M = -Df[n0:] + ref.N.T @ Df[:n0] + ref.V @ R0z
    Rp = project_to_SOdn(M, d)
    tp = t0 - ref.N @ (Rp - R0z) - ref.T[:, None] * Df[:n0]
    assert np.array_equal(ref.p.proximal(Z, Df), np.vstack([tp, Rp]))
    sv = np.linalg.svd(M.reshape(n0, d, d), compute_uv=False)
    assert np.all(sv[:, -1] >= 1e-3 * sv[:, 0]), ("proximal conditioning", (sv[:, -1] / sv[:, 0]).min())
    X = out["proximal"]
    tab["proximal R / 1e-12"] = max(tab.get("proximal R / 1e-12", 0.0), float(np.abs(X[n0:] - Rp).max() / 1e-12))
    assert np.abs(X[n0:] - Rp).max() <= 1e-12, ("proximal R", np.abs(X[n0:] - Rp).max())
    aN = abs(ref.N)
    tb = 2 * (d + 2) * U * (np.abs(t0) + aN @ np.abs(X[n0:] - R0z) + np.abs(ref.T[:, None] * Df[:n0])) \
        + np.asarray(aN.sum(axis=1)) * 1e-12
    tab["proximal t"] = max(tab.get("proximal t", 0.0), float((np.abs(X[:n0] - tp) / tb).max()))
    assert np.all(np.abs(X[:n0] - tp) <= tb), ("proximal t", (np.abs(X[:n0] - tp) / tb).max())


def run_rescaled_ops(grp, a, suffix, ref, x):
    n0, d = ref.n0, ref.d
    R0 = (d + 1) * n0
    op = lambda name, X, rows: grp.debug_apply(a, name + suffix, X, rows)
    out = {}
    for k in ("Y", "const", "mixed"):
        out["G/" + k] = op("G", x[k], R0)
    for k in ("Y", "mixed"):
        out["solve_tt/" + k] = op("solve_tt", x[k], R0)
    out["retract"] = op("retract", np.vstack([x["Y"], x["Ydot"], x["g"]]), R0)
    out["proximal"] = op("proximal", np.vstack([x["Z"], x["Dfp"]]), R0)
    return out


def check_all_nodes(grp, d, scale, sl, tab, what):
    g, meas, infos = host.ladder_case(d)
    opt = grp.get_options()
    for a in range(len(sl)):
        sc = scale[sl[a]]
        ref = ops.Ref(meas[a], a, LOSS, opt, 0.0, precon_rr=False, scale=sc)
        x = ops._inputs(np.random.default_rng(300 + a), ref)
        rs = ir.Restatement(infos[a], d, LOSS, host.DL, host.XI)
        bl = rs.blocks(sc, True)
        outs = {}
        for suffix in ("", ":all"):
            outs[suffix] = run_rescaled_ops(grp, a, suffix, ref, x)
            check_rescaled_ops(ref, x, outs[suffix], bl, tab)
        for k in ("G/Y", "G/const", "G/mixed", "proximal"):
            gi.same(outs[""][k], outs[":all"][k], (what, a, k))
        # D, and Q on own and neighbour rows: g and the quad slot of the update pass
        for name, Z in host.node_points(d, a).items():
            xi = gi.update_inputs(np.random.default_rng(7 + a), Z, infos[a].n[0], d)
            r = rs.update(Z, xi["Zprev"], xi["old"], scale=sc, dynamic=True)
            o = grp.debug_inter_update(a, Z, xi["Zprev"], xi["old"])
            gi.check(tab, "g (rescaled D)", o["g"], r["g"], r["d_g"], (what, a, name))
            gi.check(tab, "quad (rescaled Q)", o["sums"][1], r["quad"], r["d_quad"], (what, a, name))
            gi.check(tab, "<z, g>", o["sums"][2], r["zg"], r["d_zg"], (what, a, name))


@pytest.mark.parametrize("d", [3, 2])
def test_rescale_apply(d):
    g, meas, infos = host.ladder_case(d)
    gi._GROUPS.clear()     # (a group as built: all scales one)
    grp = dynamic_group(d)
    sl = node_slices(grp)
    L, m = len(sl), sl[-1].stop
    rng = np.random.default_rng(21)
    tab = {}
    ones = np.ones(m)
    # a group as built: all scales one
    check_all_nodes(grp, d, ones, sl, tab, "as built")
    # first rescale: nodes 0, 1, 2 by their counters to random scales in [0.01, 1]; node 3's weights stay below its scales
    target = rng.uniform(0.01, 1.0, m)
    w = target / 1.25
    count = np.array([MAXC, MAXC, MAXC, 0], np.int32)
    o = grp.debug_rescale(w, ones, count, MAXC, range(L))
    assert list(o["flags"]) == [1, 1, 1, 0] and o["rescaled"] == 3
    scale = o["scale"].copy()
    for a in range(L):
        gi.same(scale[sl[a]], np.clip(1.25 * w[sl[a]], 0.01, 1.0) if a < 3 else ones[sl[a]], ("first rescale", a))
    assert scale[:sl[2].stop].min() >= 0.01 and scale[:sl[2].stop].max() <= 1.0 and np.ptp(scale[sl[0]]) > 0.9
    check_all_nodes(grp, d, scale, sl, tab, "first rescale")
    # a second one on top: nodes 1 and 3 by a weight above its scale, nodes 0 and 2 left alone
    w2 = np.minimum(scale, rng.uniform(0.008, 0.8, m))
    for a in (1, 3):
        w2[sl[a].stop - 1] = np.nextafter(scale[sl[a].stop - 1], 2.0)
    o2 = grp.debug_rescale(w2, scale, np.zeros(L, np.int32), MAXC, range(L))
    assert list(o2["flags"]) == [0, 1, 0, 1] and list(o2["count"]) == [1, 0, 1, 0]
    scale2 = o2["scale"].copy()
    for a in range(L):
        gi.same(scale2[sl[a]], np.clip(1.25 * w2[sl[a]], 0.01, 1.0) if a in (1, 3) else scale[sl[a]], ("second rescale", a))
    check_all_nodes(grp, d, scale2, sl, tab, "second rescale")
    gi.report(tab, "rescale d=%d" % d)


@pytest.mark.parametrize("d", [3, 2])
def test_iterate_shapes_of_a_dynamic_group(d):
    """No kept products with Dynamic rescale: the fused extrapolation (then a product with G of its own) and the plain pass on
    an extrapolated Y."""
    g, meas, infos = host.ladder_case(d)
    gi._GROUPS.clear()     # (a group as built: all scales one)
    grp = dynamic_group(d)
    L = g["num_nodes"]
    tab = {}
    for a in range(L):
        n0 = infos[a].n[0]
        own = (d + 1) * n0
        rs = ir.Restatement(infos[a], d, LOSS, host.DL, host.XI)
        for name, Z in host.node_points(d, a).items():
            rng = np.random.default_rng(90 + a)
            gam = np.array([gi.GAMMAS[(b + a) % 3] for b in range(L)])
            Zp = Z + 0.05 * rng.standard_normal(Z.shape)
            ref = rs.iterate(Z, Zp, float(gam[a]), dynamic=True)
            fused = grp.debug_inter_iterate(a, Z, Zp, gam)
            plain = grp.debug_inter_iterate(a, Z, Zp, gam, fused=False)
            gi.check(tab, "Y", plain["Y"], ref["Y"], ref["d_Y"], (a, name))
            gi.check(tab, "g(Y)", fused["g"], ref["g"], ref["d_g"], (a, name))
            gi.check(tab, "<Y, g>", fused["sums"][0], ref["zg"], ref["d_zg"], (a, name))
            gi.same(fused["Y"][:own], plain["Y"][:own], ("fused extrapolation against k_extrapolate", a, name))
            gi.same(fused["g"], plain["g"], ("fused against plain", a, name))
            assert fused["sums"][0] == plain["sums"][0]
            for kw in (dict(whole=True), dict(gamma_dev=True)):
                o = grp.debug_inter_iterate(a, Z, Zp, gam, **kw)
                gi.same(o["g"], fused["g"], (kw, a, name))
    gi.report(tab, "dynamic iterate d=%d" % d)


def test_groups_released():
    gi._GROUPS.clear()
