"""Host side of the edge reliability and the candidate gate on the full information matrices (dpgo_amd/csrc/ml_rely.h): the host
twin of the kernels (dpgo_amd.ml_rely_edge_debug) against the long-double restatement (tests/ml_rely_restatement.py), the
constants of the rounding bounds, the restatement against what it claims -- the redundancy identity at a point that is NOT a
minimum of F_ml, the textbook forms of both statistics, graphs re-solved without one edge -- injected faults against the margins,
and the C ABI.  No GPU.

The inputs are tests/ml_inputs.py's with their seeded Omega_e (anisotropic, translation and rotation coupled, one edge scaled by
1e4) at the ISOTROPIC model's polished point (tests/test_ml_host.py: iso_point), where the gradient of F_ml does not vanish;
the re-solved graphs start from the maximum-likelihood refinement's final point (trajectory).  Sigma is the long-double inverse
of the restated anchored H = sum J' Omega J, anchor 0.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_restatement as cr  # noqa: E402
import ml_inputs as mi  # noqa: E402
import ml_rely_restatement as mrr  # noqa: E402
import ml_restatement as mr  # noqa: E402
import test_ml_host as tmh  # noqa: E402  (the whole-call inputs, their points and trajectories; none of its tests is imported)

import dpgo_amd  # noqa: E402

LD, U = mrr.LD, mrr.U
INPUTS = ["tinyGrid3D", "smallGrid3D", "grid2", "ladder2"]
# The constants of the rounding bounds (ml_rely_restatement.margins, rel_margin), one per field: the largest gap between the
# fp64 and the long-double restatement over INPUTS at their isotropic polished points, both signs, in units of the derived bound,
# times the project's margin of 4, rounded up to a power of two (test_constants_of_the_rounding_bounds prints the gaps and
# holds these).  The GPU tests use them and no others.
CONSTANTS = {"rel": 0.5, "d2": 1.0, "redundancy": 4.0, "redundancy_trans": 2.0, "d2_own": 1.0, "influence": 0.5, "r_loo": 0.5}
_pt = {}


def point(fixtures_dir, name, which="iso"):
    """dict(E, X, d, dof, N, per (long-double edges_all), Sigma (long double, anchor 0), h = sqrt(diag H), edges
    (ml_rely_restatement.edge_inputs)) at the isotropic polished point or at the refinement's final one."""
    key = (name, which)
    if key not in _pt:
        E, X = tmh.iso_point(fixtures_dir, name)
        if which == "ml":
            X = tmh.trajectory(fixtures_dir, name)["X"]
        per = mr.edges_all(E, X, LD)
        H = mr.assemble(E, X, 0, LD, per_edge=per)[2]
        lam = np.linalg.eigvalsh(np.asarray(H, np.float64))
        assert lam[0] > 0
        Sigma = mrr.inverse(H)
        _pt[key] = dict(E=E, X=X, d=E["d"], dof=cr.dof_of(E["d"]), N=E["N"], per=per, Sigma=Sigma,
                        h=np.sqrt(np.diag(np.asarray(H, np.float64))), edges=mrr.edge_inputs(E, X, Sigma, 0, per))
    return _pt[key]


def fp64_inputs(P):
    """(J (n, 2, dof, dof), joint (n, 3, dof, dof), Om, r) of every edge, rounded to fp64: what the hooks are given."""
    dof = P["dof"]
    J = np.stack([np.stack([np.asarray(x["Ji"], np.float64), np.asarray(x["Jj"], np.float64)]) for x in P["edges"]])
    joint = np.stack([np.stack([np.asarray(x["Sj"], np.float64)[:dof, :dof], np.asarray(x["Sj"], np.float64)[:dof, dof:],
                                np.asarray(x["Sj"], np.float64)[dof:, dof:]]) for x in P["edges"]])
    Om = np.stack([np.asarray(x["Om"], np.float64) for x in P["edges"]])
    r = np.stack([np.asarray(x["r"], np.float64) for x in P["edges"]])
    return J, joint, Om, r


def compare(d, sign, lib_rel, lib_rec, J, joint, Om, r, constants=None):
    """One edge of a hook's output against the long-double restatement on the same fp64 inputs: (rel's worst error / bound,
    the record's, the restated record, whether the flag was rounding's to decide, whether the flags agree).  Where the flags
    differ only the entries that do not depend on the flag are compared."""
    constants = constants or CONSTANTS
    dof = cr.dof_of(d)
    Sj = mrr.joint_matrix(joint)
    rel = mrr.mirrored(mrr.rel_of(J[0], J[1], Sj))   # (the lower triangle, written to both places: ml_rely.h)
    b_rel = constants["rel"] * mrr.mirrored(mrr.rel_margin(J[0], J[1], Sj))
    e_rel = np.abs(np.asarray(lib_rel, LD) - rel).astype(np.float64)
    assert np.all(e_rel[b_rel == 0] == 0)
    w_rel = float((e_rel[b_rel > 0] / b_rel[b_rel > 0]).max()) if np.any(b_rel > 0) else 0.0
    ref = mrr.record(rel, Om, r, d, sign)
    bnd, bpiv = mrr.bound(ref, d, constants, m_rel=b_rel)
    same = int(lib_rec[1]) == ref["flag"]
    idx = np.arange(mrr.width(d, sign))
    if not same:
        idx = np.array([2, 3, 4] + list(range(6, 6 + dof))) if sign < 0 else np.arange(2, 2 + dof)
    idx = idx[idx != 1]
    err = np.abs(np.asarray(lib_rec, LD) - mrr.vector(ref, d)).astype(np.float64)[idx]
    w = float(np.max(np.where(err == 0, 0.0, err / (bnd[idx] + 1e-300))))
    return w_rel, w, ref, mrr.decided(ref, bpiv), same


# ---------------------------------------------------------------------------------------------------------------
# (a) the host twin against the long-double restatement, and the constants
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sign", [-1, 1])
@pytest.mark.parametrize("name", INPUTS)
def test_host_twin_against_the_restatement(fixtures_dir, name, sign):
    P = point(fixtures_dir, name)
    d, dof = P["d"], P["dof"]
    J, joint, Om, r = fp64_inputs(P)
    rel, rec = dpgo_amd.ml_rely_edge_debug(d, J, joint, Om, r, sign=sign)
    assert rec.shape == (len(J), mrr.width(d, sign))
    worst_rel = worst = 0.0
    flagged = undecided = 0
    for e in range(len(J)):
        assert np.array_equal(rel[e], rel[e].T)
        wr, w, ref, dec, same = compare(d, sign, rel[e], rec[e], J[e], joint[e], Om[e], r[e])
        worst_rel, worst = max(worst_rel, wr), max(worst, w)
        if dec:
            assert same, (e, rec[e][1], ref["flag"], ref["pivots"])
        else:
            undecided += 1
        off = 2 if sign > 0 else 6
        assert np.array_equal(rec[e][off:off + dof], r[e])
        if rec[e][1] == 1:
            flagged += 1
            assert rec[e][0] == 0 and (sign > 0 or (rec[e][5] == 0 and not rec[e][6 + dof:].any() and rec[e][4] > 0))
    print("%s, sign %+d: %d edges, rel %.3g and records %.3g of their bounds, %d flagged, %d flags left to rounding"
          % (name, sign, len(J), worst_rel, worst, flagged, undecided))
    assert worst_rel <= 1.0 and worst <= 1.0
    if sign > 0:
        assert flagged == 0   # I + A is positive definite whatever the point


def test_constants_of_the_rounding_bounds(fixtures_dir):
    """The largest gap between the fp64 and the long-double restatement of each field over the inputs, in units of its derived
    bound; times 4, rounded up to a power of two, it is the recorded constant.  rel: both from the same fp64 J and joint; the
    records: both from the same fp64 rel, Omega and r, so that the gap is this arithmetic's alone."""
    worst = {k: 0.0 for k in CONSTANTS}
    for name in INPUTS:
        P = point(fixtures_dir, name)
        d = P["d"]
        J, joint, Om, r = fp64_inputs(P)
        for e in range(len(J)):
            Sj = mrr.joint_matrix(joint[e])
            rel64 = mrr.rel_of(J[e][0], J[e][1], np.asarray(Sj, np.float64), np.float64)
            b = mrr.rel_margin(J[e][0], J[e][1], Sj)
            err = np.abs(np.asarray(rel64, LD) - mrr.rel_of(J[e][0], J[e][1], Sj)).astype(np.float64)
            if np.any(b > 0):
                worst["rel"] = max(worst["rel"], float((err[b > 0] / b[b > 0]).max()))
            for sign in (-1, 1):
                ref = mrr.record(rel64, Om[e], r[e], d, sign)
                got = mrr.record(rel64, Om[e], r[e], d, sign, dtype=np.float64)
                if ref["flag"] != 0 or got["flag"] != 0:
                    continue
                m = mrr.margins(ref, d)[0]
                err = np.abs(mrr.vector(got, d) - mrr.vector(ref, d)).astype(np.float64)
                for i, f in enumerate(mrr.fields(d, sign)):
                    if f and m[i] > 0:
                        worst[f] = max(worst[f], err[i] / m[i])
    for k, v in worst.items():
        c = 2.0 ** np.ceil(np.log2(4 * v)) if v > 0 else 0.0
        print("%s: worst gap %.3g of the bound, times 4 and rounded up: %g (recorded %g)" % (k, v, c, CONSTANTS[k]))
    for k, v in worst.items():
        assert 2.0 ** np.ceil(np.log2(4 * v)) == CONSTANTS[k], (k, v)


# ---------------------------------------------------------------------------------------------------------------
# (b) the restatement against what it claims
# ---------------------------------------------------------------------------------------------------------------
def edge_bound_inputs(P, x):
    """(m_rel, m_r) of an edge whose rel comes from an fp64 factorisation of H and exact J: what the rounding of Sigma's
    computation moves rel by, plus rel's own rounding."""
    return (mrr.rel_margin_sigma(x["Ji"], x["Jj"], P["Sigma"], P["h"], x["p"], x["q"], 0) +
            CONSTANTS["rel"] * mrr.rel_margin(x["Ji"], x["Jj"], x["Sj"])), None


@pytest.mark.parametrize("name", INPUTS)
def test_redundancies_sum_to_the_degrees_of_freedom_at_any_point(fixtures_dir, name):
    """sum_e tr(Omega_e J_e Sigma J_e^T) = tr(Sigma H) = dof (N - 1): the identity of the Gauss-Newton Hessian, at the isotropic
    polished point, where F_ml is not stationary and the residuals are not small.  The bound is what an fp64 evaluation is held
    to -- the sum of the edges' redundancy bounds for exact Sigma, plus what the rounding of Sigma's computation moves the sum
    by (ml_rely_restatement.sum_margin_sigma); the long-double evaluation is held to it a fortiori."""
    P = point(fixtures_dir, name)
    d, dof, m = P["d"], P["dof"], len(P["edges"])
    total, bnd = LD(0), 0.0
    for x in P["edges"]:
        rec = mrr.record(x["rel"], x["Om"], x["r"], d)
        total += rec["redundancy"]
        bnd += mrr.bound(rec, d, CONSTANTS, CONSTANTS["rel"] * mrr.rel_margin(x["Ji"], x["Jj"], x["Sj"]))[0][2]
    bnd += mrr.sum_margin_sigma(P["Sigma"], P["h"], 0, dof)
    g = np.linalg.norm(np.asarray(mr.assemble(P["E"], P["X"], 0, LD, per_edge=P["per"])[1], np.float64))
    want = dof * (m - P["N"] + 1)
    print("%s: sum of redundancies %.15g, dof (m - N + 1) = %d, apart %.3g, bound %.3g; |g_ml| = %.3g at this point"
          % (name, float(total), want, abs(float(total - want)), bnd, g))
    assert g > 1e-3 and abs(float(total - want)) <= bnd


@pytest.mark.parametrize("name", ["smallGrid3D", "grid2"])
def test_whitened_forms_are_the_textbook_statistics(fixtures_dir, name):
    """d2 of sign + is r' (rel + Omega^-1)^-1 r and d2_loo is r' (Omega^-1 - rel)^-1 r, both in long double with Omega
    inverted explicitly, within the fp64 bound of d2 (the two long-double evaluations differ by far less)."""
    P = point(fixtures_dir, name)
    worst, n = 0.0, 0
    for x in P["edges"]:
        for sign in (-1, 1):
            rec = mrr.record(x["rel"], x["Om"], x["r"], P["d"], sign)
            if rec["flag"] != 0:
                continue
            b = mrr.bound(rec, P["d"], CONSTANTS)[0][0]
            worst = max(worst, abs(float(rec["d2"] - mrr.classical(x["rel"], x["Om"], x["r"], sign))) / b)
            n += 1
    print("%s: %d statistics, whitened against textbook form at %.3g of the fp64 bound" % (name, n, worst))
    assert n >= len(P["edges"]) and worst <= 1.0


def loo_edges(P):
    """Three edges the leave-one-out test can tell the quantities apart on: flag 0, redundancy <= 0.8 dof (an edge the rest of
    the graph does not fully determine: d2_loo and d2_own differ by the factor the redundancy sets), and of those the three with the
    largest d2_own, whose re-solved graph moves the most."""
    rows = []
    for x in P["edges"]:
        rec = mrr.record(x["rel"], x["Om"], x["r"], P["d"])
        if rec["flag"] == 0 and float(rec["redundancy"]) <= 0.8 * P["dof"]:
            rows.append((float(rec["d2_own"]), x["e"]))
    return [e for _, e in sorted(rows, reverse=True)[:3]]


@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("name", ["smallGrid3D", "grid2"])
def test_leave_one_out_against_the_resolved_graph(fixtures_dir, name, k):
    """The graph without edge e, refined again (ml_restatement.polish_full) from the full graph's point: twice the drop of the
    optimum is nearer d2_loo than d2_own, and the edge's residual at the new point nearer r_loo than r.  First-order statements
    of the Gauss-Newton model: no tolerance beyond the two orderings.  Measured (edge: 2 dF*, d2_loo, d2_own; |r_loo - r2|,
    |r - r2|):
        smallGrid3D   see DESIGN section 31
        grid2         see DESIGN section 31"""
    P = point(fixtures_dir, name, "ml")
    E, X, d = P["E"], P["X"], P["d"]
    e = loo_edges(P)[k]
    x = P["edges"][e]
    rec = mrr.record(x["rel"], x["Om"], x["r"], d)
    keep = np.arange(len(E["I"])) != e
    Ee = dict(E, **{key: E[key][keep] for key in ("I", "J", "R", "t", "kappa", "tau", "Om")})
    res = mr.polish_full(Ee, X, anchor=0, max_steps=40)
    assert res["outcome"] == tmh.nr.CONVERGED
    dF2 = 2 * float(mr.objective(E, X, LD) - mr.objective(Ee, res["X"], LD))
    Pz = mr.poses_of(res["X"], d)
    r2 = np.asarray(mr.edge(d, E["R"][e], E["t"][e], Pz[x["p"]], Pz[x["q"]], LD)[0], np.float64)
    d2_loo, d2_own = float(rec["d2"]), float(rec["d2_own"])
    r, r_loo = np.asarray(rec["r"], np.float64), np.asarray(rec["r_loo"], np.float64)
    print("%s edge %d (redundancy %.3f): 2 dF* %.6g, d2_loo %.6g, d2_own %.6g; |r_loo - r2| %.3g, |r - r2| %.3g, |r2| %.3g"
          % (name, e, float(rec["redundancy"]), dF2, d2_loo, d2_own, np.linalg.norm(r_loo - r2), np.linalg.norm(r - r2),
             np.linalg.norm(r2)))
    assert abs(d2_loo - dF2) < abs(d2_own - dF2)
    assert np.linalg.norm(r_loo - r2) < np.linalg.norm(r - r2)


# ---------------------------------------------------------------------------------------------------------------
# (c) injected faults
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fault", mrr.FAULTS)
def test_an_injected_fault_is_caught_by_a_margin(fixtures_dir, fault):
    """The restated step with one mistake, on every edge of smallGrid3D, against the bounds an fp64 result is held to (the
    factorisation's part included): the entry the mistake touches leaves its bound on the edges that can show it -- every edge but
    those at the anchor for S_pq transposed (zero there), every edge whose Omega is not diagonal for the two faults that
    need one (every fifth edge is Omega_iso, ml_inputs.information), every edge for the sign and the whitening's transpose."""
    P = point(fixtures_dir, "smallGrid3D")
    d, dof = P["d"], P["dof"]
    field = dict(sign=0, l_transposed=0, transpose=0, diag_omega=0, trace=2)[fault]
    Ef = mrr.edge_inputs(P["E"], P["X"], P["Sigma"], 0, P["per"], fault=fault) if fault == "transpose" else P["edges"]
    caught = able = 0
    for x, xf in zip(P["edges"], Ef):
        ref = mrr.record(x["rel"], x["Om"], x["r"], d)
        bad = mrr.record(xf["rel"], x["Om"], x["r"], d, fault=None if fault == "transpose" else fault)
        m = mrr.bound(ref, d, CONSTANTS, *edge_bound_inputs(P, x))[0]
        err = np.abs(mrr.vector(bad, d) - mrr.vector(ref, d)).astype(np.float64)
        diagonal = not np.any(np.asarray(x["Om"], np.float64) - np.diag(np.diag(np.asarray(x["Om"], np.float64))))
        can = not (fault == "transpose" and 0 in (x["p"], x["q"])) and not (fault in ("diag_omega", "l_transposed") and diagonal)
        able += can
        caught += bool(can and (err[field] > m[field] or bad["flag"] != ref["flag"]))
    print("%s: caught on %d of the %d edges that can show it (%d edges)" % (fault, caught, able, len(Ef)))
    assert able >= len(Ef) // 2 and caught == able


# ---------------------------------------------------------------------------------------------------------------
# (d) C ABI
# ---------------------------------------------------------------------------------------------------------------
def test_ml_rely_abi():
    L = dpgo_amd.lib()
    root = os.path.join(os.path.dirname(dpgo_amd.__file__), "..")
    header = open(os.path.join(root, "include", "dpgo_amd.h")).read()
    for sym in ("dpgo_group_ml_edge_reliability", "dpgo_group_ml_pair_gate", "dpgo_debug_ml_rely_edge_host", "dpgo_debug_ml_rely_edge"):
        assert sym + "(" in header and sym in dpgo_amd.SYMBOLS and hasattr(L, sym)
    for name in ("ml_edge_reliability", "ml_pair_gate"):
        assert callable(getattr(dpgo_amd.NodeGroup, name))
    assert callable(dpgo_amd.ml_rely_edge_debug)
    facade = open(os.path.join(root, "include", "dpgo_amd.hpp")).read()
    assert "ml_edge_reliability(" in facade and "ml_pair_gate(" in facade
    X = np.zeros((8, 3), order="F")
    dp = X.ctypes.data_as(C.POINTER(C.c_double))
    r, pr_ = dpgo_amd.RelyResult(), dpgo_amd.PairsResult()
    G = dpgo_amd.graph_from_edges(2, 2, [0], [1], [np.eye(2)], [np.zeros(2)], [1.0], [1.0], 1)
    # no group, no graph, no point, no output, no result
    assert L.dpgo_group_ml_edge_reliability(None, G._h, dp, 8, 0, 0, 0, None, 0, dp, None, None, C.byref(r)) == -1
    assert L.dpgo_group_ml_pair_gate(None, G._h, dp, 8, 0, 0, None, 0, dp, dp, dp, dp, dp, dp, C.byref(pr_)) == -1
    # the hooks: null arrays, a dimension that is neither 2 nor 3, a sign that is not +-1, a negative count, an Omega that is
    # not positive definite
    dof = 6
    J, joint, Om, rr_ = np.zeros((1, 2, dof, dof)), np.zeros((1, 3, dof, dof)), np.eye(dof)[None].copy(), np.zeros((1, dof))
    rel, rec = np.zeros((1, dof, dof)), np.zeros((1, 6 + 2 * dof))
    p = [a.ctypes.data_as(C.POINTER(C.c_double)) for a in (J, joint, Om, rr_, rel, rec)]
    assert L.dpgo_debug_ml_rely_edge_host(3, 1, -1, *p) == 0 and rec[0, 2] == dof and rec[0, 1] == 0
    for k in range(6):
        q = list(p)
        q[k] = None
        assert L.dpgo_debug_ml_rely_edge_host(3, 1, -1, *q) == -1
    assert L.dpgo_debug_ml_rely_edge_host(4, 1, -1, *p) == -1 and L.dpgo_debug_ml_rely_edge_host(3, 1, 0, *p) == -1
    assert L.dpgo_debug_ml_rely_edge_host(3, 1, 2, *p) == -1 and L.dpgo_debug_ml_rely_edge_host(3, -1, 1, *p) == -1
    assert L.dpgo_debug_ml_rely_edge_host(3, 0, 1, *p) == 0
    Om[0, 2, 2] = -1.0
    assert L.dpgo_debug_ml_rely_edge_host(3, 1, -1, *p) == -1
    with pytest.raises(ValueError):
        dpgo_amd.ml_rely_edge_debug(3, np.zeros((2, 2, 6, 6)), np.zeros((1, 3, 6, 6)), np.zeros((2, 6, 6)), np.zeros((2, 6)))
    with pytest.raises(RuntimeError):
        dpgo_amd.ml_rely_edge_debug(3, J, joint, Om, rr_)
