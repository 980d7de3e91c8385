"""One device Steihaug-Toint CG (NodeGroup.debug_stpcg: a refinement round's CG and nothing after it, through TntRun's own
pieces) against oracle.tnt.stpcg driven with the oracle's operators: DPGOProblem.hessian_vector_product, the preconditioner
(RegularizedCholesky with the shift formed from the device's lambda_max as test_gpu_operators.Ref does, Jacobi, or none) and
the gradient from tangent_proj.

Cases: the six nodes of synthetic.ladder(3) / ladder(2) at random rotations (negative curvature at the first steps), once with
the one-pose node at its oracle-refined point (it fails the gradient test: active = 0, s = 0); the three 60-pose nodes of
synthetic.grid(6, 6, 5, 700) at the oracle's point after 2 and after 6 trust-region iterations, over radii, iteration limits,
preconditioners, both starts, the whole group and the subset {0, 2}.  The coverage the oracle's verdicts must show is asserted
from the oracle alone (test_oracle_coverage).

A case is kept only where every comparison the oracle takes has relative margin >= 1e-6 (at most one case in ten may go);
without a preconditioner a case the oracle takes past 12 steps is left out.

Per node: cg_it, the exit kind (stop_ord's parity, h_M_norm == Delta) and `active` are the oracle's; the gradient is within
the projection's and the product's rounding bounds; h_M_norm within 1e-12 on interior stops.

s against the oracle's s.  No closed bound exists for k steps of CG, so the oracle itself is measured: it is run five more
times with every H p and P r perturbed entrywise by relative 1e-12 noise, and ten times the largest deviation seen is
allowed (the factor covers five samples).  What test_gpu_operators.check_ops proves for `hess` and `precon` at these sizes,
its `tol` relative to the result at the first CG direction of these cases (HESS_TOL_SEEN, PRECON_TOL_SEEN below;
test_operator_bounds_are_as_recorded re-derives them):
    hess     lattice nodes 8.6e-13 .. 3.4e-12;  ladder nodes 3.2e-12 .. 3.7e-10 (the largest on the one-pose node and on the
             81-pose node, whose 10 kappa u solve term dominates: kappa_1(G_tt) = 1.4e3)
    precon   7.0e-15 .. 1.5e-12
So 1e-12 is that envelope on the lattice and for the preconditioner, and is TIGHTER than the proven bound for `hess` on the
ladder, where the CG ends at its first or second step.
The noise leaves one input of the CG alone: the gradient it starts from, which the device has to the bound asserted below
(gb, the Frobenius norm of the per-block bounds).  Without a preconditioner a CG that ends at its first step returns
s = -(Delta / |grad|) grad whatever H p was, and the measured deviation is exactly 0; to first order the gradient's error
moves that s by at most 2 |s| gb / |grad|, which is added to the tolerance of every case.

Without a reference run: H s as returned is the device's own `hess` applied to the returned s, within that operator's bound
summed over the steps (|c_k| tol(p_k)) plus the accumulations' rounding; without a preconditioner |s| = Delta to 1e-12 on
every boundary, curvature or kernel exit; the model value <grad, s> + 1/2 <s, H s> is negative and within the tolerance of s
times (|grad| + |H s|) of the oracle's.
"""
import math
import os

import numpy as np
import pytest

from oracle import g2o as og
from oracle import tnt as otnt
from oracle.problem import LOSS_NONE, project_to_SOdn, tangent_proj

U = 2.0 ** -53
MIN_MARGIN = 1e-6
NOISE = 1e-12
HESS_TOL_SEEN = {"lattice": (8.6e-13, 3.4e-12), "ladder": (3.2e-12, 3.7e-10)}
PRECON_TOL_SEEN = (7.0e-15, 1.5e-12)
PRECON_NONE, PRECON_JACOBI, PRECON_CHOL = 0, 1, 3
LATTICE = (6, 6, 5, 700)


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's side (no device but for lambda_max)

def _measurements(g):
    z = np.zeros(len(g["I"]), np.int64)
    return og.Measurements(z, g["I"], z, g["J"], g["R"], g["t"], g["kappa"], g["tau"])


class Node:
    """The oracle's operators of one node at a point"""

    def __init__(self, ref, precon):
        self.ref, self.p, self.precon = ref, ref.p, precon
        self.d, self.n0 = ref.d, ref.n0
        self.jac = 1.0 / ref.GRR.diagonal() if precon == PRECON_JACOBI else None

    def at(self, R, g):
        """the point [t recovered ; R] and the operators there"""
        self.g = g
        self.Y = np.vstack([self.p.recover_translations(R, g), R])
        self.nabla = g + self.ref.G @ self.Y
        self.grad = tangent_proj(R, self.nabla[self.n0:], self.d)
        return self

    def H(self, v):
        return self.p.hessian_vector_product(self.Y, self.nabla[self.n0:], v)

    def P(self, v):
        R = self.Y[self.n0:]
        if self.precon == PRECON_CHOL:
            return tangent_proj(R, self.ref.Lrr.solve(v), self.d)
        if self.precon == PRECON_JACOBI:
            return tangent_proj(R, self.jac[:, None] * v, self.d)
        return v


def _inner(a, b):
    return float(np.sum(a * b))


def run_oracle(node, Delta, opt, rng=None):
    """oracle.tnt.stpcg on the node's operators (rng: every H p and P r perturbed by relative NOISE).  Returns a dict: s,
    h_M_norm, cg_it, exit, margin (the smallest relative margin of its comparisons), active, dirs (the p_k handed to H) and
    coefs (the c_k of s = sum c_k p_k)."""
    def noisy(x):
        return x if rng is None else x * (1.0 + NOISE * rng.standard_normal(x.shape))
    dirs, dec, trace = [], [], []

    def H(v):
        dirs.append(v.copy())
        return noisy(node.H(v))
    P = None if node.precon == PRECON_NONE else (lambda v: noisy(node.P(v)))
    gn = math.sqrt(_inner(node.grad, node.grad))
    pg = node.grad if P is None else node.P(node.grad)
    pgn = math.sqrt(_inner(pg, pg))
    margin = min(abs(gn - opt.grad_norm_tol) / max(gn, opt.grad_norm_tol),
                 abs(pgn - opt.preconditioned_grad_norm_tol) / max(pgn, opt.preconditioned_grad_norm_tol))
    if gn < opt.grad_norm_tol or pgn < opt.preconditioned_grad_norm_tol:
        return dict(s=np.zeros_like(node.grad), h_M_norm=0.0, cg_it=0, exit="inactive", margin=margin, active=0, dirs=[], coefs=[])
    with np.errstate(all="ignore"):
        s, hM, it = otnt.stpcg(node.grad, H, _inner, Delta, opt.max_tCG_iterations, opt.STPCG_kappa, opt.STPCG_theta, P,
                               trace=trace, decisions=dec)
    kind = [x[2] for x in dec if x[0] == "exit"][0]
    for what, _, a, b, scale in dec:
        if what != "exit" and np.isfinite(a) and np.isfinite(b):
            margin = min(margin, abs(a - b) / scale if scale > 0 else 0.0)
    coefs = [al for al, _ in trace]
    if len(dirs) > len(coefs):   # the last step, to the boundary: s = sum alpha_k p_k + sigma p_last
        rest = s - sum(c * p for c, p in zip(coefs, dirs))
        coefs.append(_inner(rest, dirs[-1]) / _inner(dirs[-1], dirs[-1]))
    return dict(s=s, h_M_norm=hM, cg_it=it, exit=kind, margin=margin, active=1, dirs=dirs, coefs=coefs)


def envelope(node, Delta, opt, base, seed):
    """the largest |s' - s| over five perturbed reruns of the oracle (inf if one of them decides differently)"""
    rng = np.random.default_rng(seed)
    dev = 0.0
    for _ in range(5):
        o = run_oracle(node, Delta, opt, rng)
        if (o["cg_it"], o["exit"]) != (base["cg_it"], base["exit"]):
            return math.inf
        dev = max(dev, float(np.linalg.norm(o["s"] - base["s"])))
    return dev


def oracle_refine(node, R0, g, iterations, opt):
    """the rotations after `iterations` trust-region iterations of the oracle from R0 (every other stopping test off)"""
    p, n0 = node.p, node.n0
    cache = {}

    def QM(Y):
        cache["nabla"] = p.reduced_Euclidean_gradient_G(Y, g)
        return p.reduced_tangent_space_projection(Y, cache["nabla"]), (lambda Yc, v: p.hessian_vector_product(Yc, cache["nabla"], v))
    prm = otnt.TNTParams()
    prm.max_iterations = prm.max_iterations_accepted = iterations
    prm.gradient_tolerance = prm.preconditioned_gradient_tolerance = 0.0
    prm.relative_decrease_tolerance = prm.stepsize_tolerance = prm.Delta_tolerance = 0.0
    prm.max_TPCG_iterations, prm.kappa_fgr, prm.theta = opt.max_tCG_iterations, opt.STPCG_kappa, opt.STPCG_theta

    def precon(Y, v):
        node.Y = Y
        return node.P(v)
    x0 = np.vstack([p.recover_translations(R0, g), R0])
    with np.errstate(all="ignore"):
        res = otnt.tnt(lambda Y: p.evaluate_G(Y, g, 0.0), QM, lambda Y, a, b: _inner(a, b), lambda Y, v: p.retract(Y, v, g), x0,
                       None if node.precon == PRECON_NONE else precon, prm)
    return res["x"][n0:], res


# ---------------------------------------------------------------------------------------------------------------------
# graphs, groups (one per graph and preconditioner) and the oracle's nodes

_GRAPHS, _GROUPS = {}, {}


def graph(name):
    from dpgo_amd import synthetic
    if name not in _GRAPHS:
        g = synthetic.grid(*LATTICE) if name == "lattice" else synthetic.ladder(int(name[-1]))
        nn = 3 if name == "lattice" else g["num_nodes"]
        _, meas, _ = og.partition_measurements(g["num_poses"], _measurements(g), nn)
        _GRAPHS[name] = (g, nn, meas)
    return _GRAPHS[name]


def options(precon, max_it=1000):
    import dpgo_amd
    return dpgo_amd.Options.driver(LOSS_NONE, True, preconditioner=precon, max_tCG_iterations=max_it)


def group(name, precon):
    """(the device group, the oracle's Node per node), the shift of the oracle's preconditioner from the device's lambda_max"""
    import dpgo_amd
    from test_gpu_operators import Ref, _device_graph
    key = (name, precon)
    if key not in _GROUPS:
        g, nn, meas = graph(name)
        opt = options(precon)
        grp = dpgo_amd.NodeGroup(_device_graph(g, nn), range(nn), opt)
        nodes = []
        for a in range(nn):
            lam = float(grp.debug_apply(a, "lambda_max", np.zeros((1, grp.d)), 1)[0, 0]) if precon == PRECON_CHOL else 0.0
            nodes.append(Node(Ref(meas[a], a, LOSS_NONE, opt, lam, precon_rr=precon == PRECON_CHOL), precon))
        _GROUPS[key] = (grp, nodes)
    return _GROUPS[key]


def set_limit(grp, precon, max_it):
    opt = options(precon, max_it)
    assert grp.set_options(opt) == 0
    return opt


# ---------------------------------------------------------------------------------------------------------------------
# the points

def ladder_point(nodes, c, seed):
    rng = np.random.default_rng(seed)
    out = []
    for nd in nodes:
        R = project_to_SOdn(rng.standard_normal((nd.d * nd.n0, nd.d)), nd.d)
        out.append((R, c * rng.standard_normal(((nd.d + 1) * nd.n0, nd.d))))
    return out


_LATTICE_POINTS = {}


def lattice_point(nodes, iterations, precon):
    """the oracle's point after `iterations` trust-region iterations from identity rotations, g = 0.1 randn"""
    key = (iterations, precon)
    if key not in _LATTICE_POINTS:
        rng = np.random.default_rng(11)
        opt = options(precon)
        out = []
        for nd in nodes:
            g = 0.1 * rng.standard_normal(((nd.d + 1) * nd.n0, nd.d))
            R, _ = oracle_refine(nd, np.tile(np.eye(nd.d), (nd.n0, 1)), g, iterations, opt)
            out.append((R, g))
        _LATTICE_POINTS[key] = out
    return _LATTICE_POINTS[key]


# ---------------------------------------------------------------------------------------------------------------------
# one run: the device against the oracle

STATS = dict(kept=0, dropped=0, skipped=0, exits=[])
_ORACLE = {}


def oracle_case(name, precon, max_it, Delta, a, tag, node, opt):
    """(the oracle's run of node a at the point `tag`, which `node` is set to; its envelope) -- computed once: the runs that
    differ in the start or in the subset only share it, and so does test_oracle_coverage"""
    import zlib
    key = (name, precon, max_it, Delta, a, tag)
    if key not in _ORACLE:
        o = run_oracle(node, Delta, opt)
        far = precon == PRECON_NONE and o["cg_it"] > 12
        seed = zlib.crc32(repr(key).encode())
        _ORACLE[key] = (o, envelope(node, Delta, opt, o, seed) if o["active"] and not far else 0.0)
    return _ORACLE[key]


def hess_tol(nd, v):
    """test_gpu_operators.check_ops' bound on |hess_dev(v) - hess_oracle(v)| (Frobenius)"""
    from test_gpu_operators import _block_norms, _prod_bound
    ref, d, n0 = nd.ref, nd.d, nd.n0
    tdot = -ref.p.L.solve(ref.GtR @ v)
    e_t = ref.tdot_bound(_prod_bound(ref.GtR, v, terms=ref.terms[:n0]), tdot)
    sbd = float(np.sum(_block_norms(v, d) * _block_norms(nd.nabla[n0:], d)))
    mag = np.linalg.norm(abs(ref.GRt) @ np.abs(tdot)) + np.linalg.norm(abs(ref.GRR) @ np.abs(v)) + sbd
    return ref.GRt_norm * e_t + 2 * (ref.kmax + 3 * d + 2) * d * U * mag


def precon_tol(nd, v):
    """... and on |precon_dev(v) - precon_oracle(v)|"""
    from test_gpu_operators import _proj_bound
    ref, d = nd.ref, nd.d
    if nd.precon == PRECON_JACOBI:
        w = nd.jac[:, None] * v
        e = (ref.kmax + 3) * U * np.linalg.norm(w)
    else:
        w = ref.Lrr.solve(v)
        e = 10 * ref.kappa_rr * U * np.linalg.norm(w)
    return e + np.linalg.norm(_proj_bound(w, d))


def hess_norm(nd):
    """an upper bound on |H|_2 at the node's point"""
    from test_gpu_operators import _block_norms, _norm1
    ref = nd.ref
    return _norm1(ref.GRR) + ref.GRt_norm ** 2 * ref.inv_tt + float(_block_norms(nd.nabla[nd.n0:], nd.d).max())


def check_run(name, precon, max_it, points, tag, Delta, subset, device_start, fill=7.25):
    """One debug_stpcg run of the nodes `subset` at `points` (tag: what names them) against the oracle, node by node.  Returns what the oracle did per node, or
    None when the case is dropped (margins) or left out (no preconditioner, past 12 steps)."""
    from test_gpu_operators import _block_norms, _proj_bound, _prod_bound
    grp, nodes = group(name, precon)
    opt = set_limit(grp, precon, max_it)
    L = len(nodes)
    for nd, (R, g) in zip(nodes, points):
        nd.at(R, g)
    orc, env = {}, {}
    for a in subset:
        orc[a], env[a] = oracle_case(name, precon, max_it, Delta, a, tag, nodes[a], opt)
    if precon == PRECON_NONE and any(o["cg_it"] > 12 for o in orc.values()):
        STATS["skipped"] += 1
        return None
    if min(o["margin"] for o in orc.values()) < MIN_MARGIN or any(math.isinf(e) for e in env.values()):
        STATS["dropped"] += 1
        return None
    STATS["kept"] += 1
    STATS["exits"].append([(orc[a]["exit"], orc[a]["cg_it"]) for a in subset])
    out = grp.debug_stpcg(subset, [np.vstack([nd.Y, nd.g]) for nd in nodes], [Delta] * L, device_start, fill)
    for a in range(L):
        nd, o = nodes[a], out[a]
        d, n0 = nd.d, nd.n0
        what = (name, precon, max_it, Delta, tuple(subset), device_start, a)
        if a not in subset:   # its rows of the work vectors come back as they were written
            assert all(np.all(o[k] == fill) for k in ("s", "hs", "grad")), what
            assert o["active"] == 0 and np.all(o["sums"] == 0)
            continue
        ref = orc[a]
        # ---- the gradient, and the start sums against the returned vectors
        assert np.all(o["grad"][:n0] == 0) and np.all(o["s"][:n0] == 0) and np.all(o["hs"][:n0] == 0), what
        nb = _prod_bound(nd.ref.G, nd.Y, nd.g, nd.ref.terms)[n0:]
        dg = _block_norms(o["grad"][n0:] - nd.grad, d)
        gbound = _proj_bound(nd.nabla[n0:], d) + _block_norms(nb, d)
        assert np.all(dg <= gbound), (what, "grad", dg.max())
        g2 = _inner(o["grad"], o["grad"])
        assert abs(o["sums"][0] - g2) <= 1e-13 * g2, (what, "|grad|^2")
        # ---- the decisions
        assert o["active"] == ref["active"], (what, "active", ref["margin"])
        if not ref["active"]:
            assert np.all(o["s"] == 0) and np.all(o["hs"] == 0) and o["cg_it"] == 0, what
            continue
        assert o["cg_it"] == ref["cg_it"], (what, "cg_it", o["cg_it"], ref["cg_it"], ref["exit"], ref["margin"])
        edge = ref["exit"] in ("boundary", "curvature", "kernel")
        assert o["stop_ord"] == 2 * ref["cg_it"] + (1 if edge else 0), (what, "stop_ord", o["stop_ord"], ref["exit"])
        assert (o["h_M_norm"] == Delta) == edge and o["live"] == 0 and o["Delta"] == Delta, (what, o["h_M_norm"])
        if ref["exit"] == "limit":
            assert o["cg_it"] == max_it
        if not edge:
            assert abs(o["h_M_norm"] - ref["h_M_norm"]) <= 1e-12 * ref["h_M_norm"], (what, "h_M_norm", o["h_M_norm"], ref["h_M_norm"])
        # ---- s against the oracle's, within ten times what the oracle's own perturbation moves it
        s, hs = o["s"][n0:], o["hs"][n0:]
        tol_s = 10 * env[a] + 2 * float(np.linalg.norm(ref["s"])) * float(np.linalg.norm(gbound)) / math.sqrt(_inner(nd.grad, nd.grad))
        err = float(np.linalg.norm(s - ref["s"]))
        assert err <= tol_s, (what, "s: device error %.3e, the oracle's deviation under 1e-12 noise %.3e, |s| %.3e, exit %s after %d"
                              % (err, env[a], np.linalg.norm(ref["s"]), ref["exit"], ref["cg_it"]))
        # ---- H s as returned against the device's own Hessian product of the returned s
        R0 = (d + 1) * n0
        Hs = grp.debug_apply(a, "hess", np.vstack([nd.Y, nd.nabla, o["s"], np.zeros_like(nd.Y)]), R0 + 4)[n0:R0]
        mags = [(abs(c), np.linalg.norm(p), np.linalg.norm(nd.H(p))) for c, p in zip(ref["coefs"], ref["dirs"])]
        k = len(mags)
        bound = hess_tol(nd, s) + sum(c * hess_tol(nd, p) for c, p in zip(np.abs(ref["coefs"]), ref["dirs"])) \
            + (k + 1) * U * sum(c * (hp + hess_norm(nd) * pn) for c, pn, hp in mags)
        dh = float(np.linalg.norm(hs - Hs))
        assert dh <= bound, (what, "H s", dh, bound)
        # ---- on the boundary |s| = Delta (identity metric)
        if precon == PRECON_NONE and edge:
            assert abs(np.linalg.norm(s) - Delta) <= 1e-12 * Delta, (what, np.linalg.norm(s))
        # ---- the model value
        m_dev = _inner(o["grad"][n0:], s) + 0.5 * _inner(s, hs)
        Hs_ref = nd.H(ref["s"])
        m_ref = _inner(nd.grad, ref["s"]) + 0.5 * _inner(ref["s"], Hs_ref)
        assert m_dev < 0, (what, m_dev)
        assert abs(m_dev - m_ref) <= tol_s * (np.linalg.norm(nd.grad) + np.linalg.norm(Hs_ref)) + 1e-13 * abs(m_ref), (what, m_dev, m_ref)
    return orc


# ---------------------------------------------------------------------------------------------------------------------
# the cases

LADDER_CASES = [(d, c, Delta, precon) for d in (3, 2) for c in (1.0, 100.0) for Delta in (1.0, 1e3)
                for precon in (PRECON_CHOL, PRECON_NONE)]
LATTICE_CASES = [(its, precon) for its in (2, 6) for precon in (PRECON_CHOL, PRECON_NONE)] + [(6, PRECON_JACOBI)]
LATTICE_DELTAS = (1e-2, 0.1, 1.0, 1e3)
LATTICE_LIMITS = (2, 1000)


def lattice_runs(its, precon):
    for Delta in LATTICE_DELTAS:
        for max_it in LATTICE_LIMITS:
            for device_start in (True, False):
                for subset in ([0, 1, 2], [0, 2]):
                    yield Delta, max_it, device_start, subset


@pytest.mark.gpu
@pytest.mark.parametrize("d,c,Delta,precon", LADDER_CASES)
def test_ladder(d, c, Delta, precon):
    name = "ladder%d" % d
    _, nodes = group(name, precon)
    pts = ladder_point(nodes, c, seed=1000 + d)
    k = LADDER_CASES.index((d, c, Delta, precon))
    check_run(name, precon, 1000, pts, ("random", c), Delta, list(range(len(nodes))), device_start=bool(k % 2))
    check_run(name, precon, 2, pts, ("random", c), Delta, list(range(len(nodes))), device_start=not k % 2)


@pytest.mark.gpu
@pytest.mark.parametrize("d,precon", [(2, PRECON_CHOL), (2, PRECON_NONE), (3, PRECON_NONE)])
@pytest.mark.parametrize("device_start", [True, False])
def test_ladder_converged_node(d, precon, device_start):
    """The one-pose node at its oracle-refined point fails the gradient test: active = 0, s = 0, in the same launches as five
    nodes that iterate."""
    name = "ladder%d" % d
    grp, nodes = group(name, precon)
    pts = ladder_point(nodes, 1.0, seed=2000 + d)
    one = [nd.n0 for nd in nodes].index(1)
    R, g = pts[one]
    opt = options(precon)
    for its in (3, 4, 5, 6, 8, 10):
        Rr, res = oracle_refine(nodes[one], R, g, its, opt)
        if res["gradfx_norm"] < 1e-6:
            break
    assert res["gradfx_norm"] < 1e-6, res["gradfx_norm"]   # (a thousandth of grad_norm_tol)
    pts[one] = (Rr, g)
    orc = check_run(name, precon, 1000, pts, "converged", 1.0, list(range(len(nodes))), device_start)
    assert orc is not None and orc[one]["exit"] == "inactive" and sum(o["active"] for o in orc.values()) == len(nodes) - 1


@pytest.mark.gpu
@pytest.mark.parametrize("its,precon", LATTICE_CASES)
def test_lattice(its, precon):
    _, nodes = group("lattice", precon)
    pts = lattice_point(nodes, its, precon)
    for Delta, max_it, device_start, subset in lattice_runs(its, precon):
        check_run("lattice", precon, max_it, pts, its, Delta, subset, device_start)


def coverage(exits):
    """exits: per kept run, [(exit, cg_it) per node]"""
    flat = [e for run in exits for e in run]
    return {
        "target after 3 or more steps": any(k == "target" and it >= 3 for k, it in flat),
        "iteration limit": any(k == "limit" for k, it in flat),
        "boundary at step 0": any(k == "boundary" and it == 0 for k, it in flat),
        "boundary after 2 or more steps": any(k == "boundary" and it >= 2 for k, it in flat),
        "curvature at step 0": any(k == "curvature" and it == 0 for k, it in flat),
        "curvature at step 1 or later": any(k == "curvature" and it >= 1 for k, it in flat),
        "three nodes, three different steps": any(len(run) == 3 and len({2 * it + (k in ("boundary", "curvature", "kernel"))
                                                                           for k, it in run}) == 3 for run in exits),
    }


@pytest.mark.gpu
def test_oracle_coverage():
    """From the oracle's verdicts alone, over every case of this file (the preconditioner's shift needs the device's
    lambda_max, hence the mark): each exit the device code has is taken by a kept case, and at most one case in ten was dropped
    for its margins (a comparison closer than 1e-6, or one that the 1e-12 noise turns: <r, P r> of a residual at rounding
    level, whose sign decides whether its square root is NaN)."""
    exits, kept, dropped = [], 0, 0

    def count(name, nodes, pts, tag, precon, max_it, Delta, subset):
        nonlocal kept, dropped
        opt = options(precon, max_it)
        for nd, (R, g) in zip(nodes, pts):
            nd.at(R, g)
        cases = [oracle_case(name, precon, max_it, Delta, a, tag, nodes[a], opt) for a in subset]
        if precon == PRECON_NONE and any(o["cg_it"] > 12 for o, _ in cases):
            return
        if min(o["margin"] for o, _ in cases) < MIN_MARGIN or any(math.isinf(e) for _, e in cases):
            dropped += 1
            return
        kept += 1
        exits.append([(o["exit"], o["cg_it"]) for o, _ in cases])
    for d, c, Delta, precon in LADDER_CASES:
        _, nodes = group("ladder%d" % d, precon)
        pts = ladder_point(nodes, c, seed=1000 + d)
        for max_it in (1000, 2):
            count("ladder%d" % d, nodes, pts, ("random", c), precon, max_it, Delta, list(range(len(nodes))))
    for its, precon in LATTICE_CASES:
        _, nodes = group("lattice", precon)
        pts = lattice_point(nodes, its, precon)
        for Delta in LATTICE_DELTAS:
            for max_it in LATTICE_LIMITS:
                for subset in ([0, 1, 2], [0, 2]):
                    count("lattice", nodes, pts, its, precon, max_it, Delta, subset)
    cov = coverage(exits)
    assert all(cov.values()), cov
    assert dropped * 10 <= kept + dropped, (kept, dropped)


@pytest.mark.gpu
def test_operator_bounds_are_as_recorded():
    """check_ops' bounds for `hess` and `precon`, relative to the result, at the points and first directions of these cases:
    the ranges the docstring sets beside the 1e-12 noise (within a factor of two: lambda_max is the device's)."""
    for name, its in (("lattice", 2), ("lattice", 6), ("ladder3", None), ("ladder2", None)):
        _, nodes = group(name, PRECON_CHOL)
        pts = lattice_point(nodes, its, PRECON_CHOL) if its else ladder_point(nodes, 1.0, seed=1000 + int(name[-1]))
        lo, hi = HESS_TOL_SEEN[name[:-1] if its is None else name]
        for nd, (R, g) in zip(nodes, pts):
            nd.at(R, g)
            v = -nd.P(nd.grad)
            h = hess_tol(nd, v) / np.linalg.norm(nd.H(v))
            q = precon_tol(nd, nd.grad) / np.linalg.norm(nd.P(nd.grad))
            assert 0.5 * lo <= h <= 2 * hi, (name, its, nd.n0, h)
            assert 0.5 * PRECON_TOL_SEEN[0] <= q <= 2 * PRECON_TOL_SEEN[1], (name, its, nd.n0, q)


@pytest.mark.gpu
def test_groups_released():
    _GROUPS.clear()


# ---------------------------------------------------------------------------------------------------------------------
# the switches: child processes one after another (the switches are read once per process)

CHILD = """
import sys, numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import test_gpu_stpcg as T
out = {}
for tag, name, its, Delta in (("lattice", "lattice", 6, 1e3), ("ladder", "ladder2", None, 1e3)):
    grp, nodes = T.group(name, T.PRECON_CHOL)
    pts = T.lattice_point(nodes, its, T.PRECON_CHOL) if its else T.ladder_point(nodes, 1.0, seed=1002)
    for nd, (R, g) in zip(nodes, pts):
        nd.at(R, g)
    for device_start in (False, True):
        res = grp.debug_stpcg(list(range(len(nodes))), [np.vstack([nd.Y, nd.g]) for nd in nodes], [Delta] * len(nodes), device_start)
        for a, o in enumerate(res):
            for k, v in o.items():
                out["%%s/%%d/%%d/%%s" %% (tag, device_start, a, k)] = np.asarray(v)
np.savez(sys.argv[1], **out)
"""


@pytest.mark.gpu
def test_switches_do_not_change_a_bit(tmp_path):
    """DPGO_CG_GRAPH = 0 / 1, DPGO_FUSED = 0 / 1, host and device start: eight runs of one lattice and one ladder case, every
    output bit-identical (DESIGN 3.3's guarantee for run_tnt, here for its CG alone)."""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = CHILD % (os.path.dirname(here), here)
    runs = {}
    for cg_graph in ("0", "1"):
        for fused in ("0", "1"):
            path = str(tmp_path / ("g%sf%s.npz" % (cg_graph, fused)))
            subprocess.check_call([sys.executable, "-c", code, path], env=dict(os.environ, DPGO_CG_GRAPH=cg_graph, DPGO_FUSED=fused))
            runs[(cg_graph, fused)] = dict(np.load(path))
    base = runs[("0", "0")]
    steps = 0
    for key, r in runs.items():
        for name, v in base.items():
            tag, mode, a, field = name.split("/")
            for other in (name, "%s/%d/%s/%s" % (tag, 1 - int(mode), a, field)):   # the same switches, and the other start
                assert np.array_equal(v, r[other], equal_nan=True), (key, name, other)
            if field == "cg_it":
                steps = max(steps, int(v))
    assert steps >= 5   # (the lattice nodes take 5 to 9 steps at this radius: the replayed CG steps were reached)
