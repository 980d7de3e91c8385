"""Host side of the maximum-likelihood refinement (dpgo_amd/csrc/ml.h): the graph's memory of Omega (loader, from_edges with
info, filter_edges, scale_edges, Omega_iso), the numpy restatement (tests/ml_restatement.py) against central differences, the
host twin of the kernels (dpgo_amd.ml_edge_debug) against the long-double restatement, the constants of the rounding bounds,
the margins of the Levenberg-Marquardt trajectories the GPU tests replay, and the argument checks of the C ABI.  No GPU.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_restatement as cr  # noqa: E402
import ml_inputs as mi  # noqa: E402
import ml_restatement as mr  # noqa: E402
import newton_restatement as nr  # noqa: E402
import test_polish_host as tph  # noqa: E402  (its start points; none of its tests is imported)

import dpgo_amd  # noqa: E402

U = 2.0 ** -53
LD = cr.LD

# The constants of the rounding bounds (ml_restatement.edge_bounds / sum_bounds), one per output: the largest gap between the
# fp64 and the long-double restatement over INPUTS in units of the derived bound, times the project's margin of 4, rounded up
# to a power of two (test_constants_of_the_rounding_bounds prints the gaps and holds these).  The GPU tests use them and no others.
CONSTANTS = {"r": 2.0, "wr": 2.0, "chi2": 1.0, "Ji": 2.0, "Jj": 2.0, "grad": 1.0, "blocks": 1.0, "F": 0.125, "g": 0.5, "H": 1.0}
# The whole-call inputs: where their isotropic polish starts (test_polish_host.start_point), and the refinement's max_steps.
# Gauss-Newton converges linearly where the residuals at the minimum are large, and the seeded Omega_e make them so on
# tinyGrid3D (92 steps).  The d = 2 ladder's measurements are random: its angle residuals reach 3.1398 at the isotropic point,
# F_ml jumps where one of them wraps, and the refinement cannot converge; its first steps are still a trajectory to replay.
# The d = 2 refinement that converges is ml_inputs.grid2's (consistent measurements, moderate noise), from its chordal point.
WHOLE = {"tinyGrid3D": (100, 100), "smallGrid3D": (200, 20), "ladder2": (300, 6), "grid2": ("chordal", 30)}


def graph_of(E, nn=1, info=True):
    return dpgo_amd.graph_from_edges(E["d"], E["N"], E["I"], E["J"], E["R"], E["t"], E["kappa"], E["tau"], nn,
                                     info=E["Om"] if info else None)


def chordal_point(E):
    from oracle import g2o as og
    from oracle.star import chordal_initialization
    z = np.zeros(len(E["I"]), np.int64)
    return chordal_initialization(E["N"], og.Measurements(z, E["I"], z, E["J"], E["R"], E["t"], E["kappa"], E["tau"]))


_iso = {}


def iso_point(fixtures_dir, name):
    """(E, X_iso): a whole-call input and the isotropic model's polished point (newton_restatement.polish from
    test_polish_host's start), from which the maximum-likelihood refinement starts."""
    if name not in _iso:
        if name == "grid2":
            from oracle import g2o as og
            from oracle.hash import Options as OOptions
            from oracle.problem import LOSS_NONE
            from oracle.star import GlobalProblem
            E = mi.grid2()
            z = np.zeros(len(E["I"]), np.int64)
            mm = og.Measurements(z, E["I"], z, E["J"], E["R"], E["t"], E["kappa"], E["tau"])
            gp, X = GlobalProblem(E["N"], mm, 1, OOptions.driver(LOSS_NONE, True)), chordal_point(E)
        else:
            gp, X = tph.start_point(fixtures_dir, name, WHOLE[name][0])
            E = mi.ladder(2) if name == "ladder2" else mi.fixture(fixtures_dir, name)
        Xp, outcome = nr.polish(gp.M, X, E["d"], anchor=0)[:2]
        assert outcome == nr.CONVERGED
        _iso[name] = (E, Xp)
    return _iso[name]


def ops_inputs(fixtures_dir):
    """(name, E, X) of the inputs the constants are measured on and the host twin is held on."""
    out = []
    for name in ("tinyGrid3D", "smallGrid3D"):
        E = mi.fixture(fixtures_dir, name)
        out.append((name, E, chordal_point(E)))
    for d in (2, 3):
        E = mi.ladder(d)
        out.append(("ladder%d" % d, E, chordal_point(E)))
        out.append(("noise_free%d" % d,) + mi.noise_free(d))
        for m in (1, 65):
            E, X, _ = mi.chain(d, m)
            out.append(("chain%d_%d" % (d, m), E, X))
    return out


# ---------------------------------------------------------------------------------------------------------------
# the graph keeps Omega
# ---------------------------------------------------------------------------------------------------------------
SE2 = [(0, 1, 1.0, 0.5, 0.1, [9, 2, 1, 6, -1, 5]), (1, 2, 1.0, -0.5, -0.2, [4, 1, 0, 3, 0, 7]), (0, 2, 2.0, 0.0, 0.0, [8, 0, 0, 8, 0, 2])]
# 21 numbers: rows of the upper triangle, I11 .. I16, I22 .. I26, I33 .. I36, I44 .. I46, I55 I56, I66
SE3 = [(0, 1, [1.0, 0.0, 0.5], [0.0, 0.0, 0.0, 1.0], [9, 1, 2, 1, 0, -1, 8, 1, 0, 2, 0, 7, 0, 0, 1, 6, 1, 0, 5, 1, 4]),
       (1, 2, [0.0, 1.0, 0.0], [0.0, 0.0, 0.5, 0.5], [5, 0, 1, 0, 0, 0, 6, 0, 1, 0, 0, 7, 0, 0, 1, 3, 1, 1, 4, 0, 5]),
       (0, 2, [1.0, 1.0, 0.5], [0.0, 0.0, 0.0, 1.0], [4, 0, 0, 0, 0, 0, 4, 0, 0, 0, 0, 4, 0, 0, 0, 2, 0, 0, 2, 0, 2])]


def write_g2o(path, d):
    with open(path, "w") as f:
        for e in (SE2 if d == 2 else SE3):
            if d == 2:
                f.write("EDGE_SE2 %d %d %r %r %r %s\n" % (e[0], e[1], e[2], e[3], e[4], " ".join(str(x) for x in e[5])))
            else:
                f.write("EDGE_SE3:QUAT %d %d %s %s %s\n" % (e[0], e[1], " ".join(repr(x) for x in e[2]),
                                                           " ".join(repr(x) for x in e[3]), " ".join(str(x) for x in e[4])))


def trace_inv3(a):
    """graph.cpp's formula; on the integer matrices above every product and sum is exact, so the bits do not depend on
    whether a compiler fuses them."""
    c00 = a[1, 1] * a[2, 2] - a[1, 2] * a[2, 1]
    c11 = a[0, 0] * a[2, 2] - a[0, 2] * a[2, 0]
    c22 = a[0, 0] * a[1, 1] - a[0, 1] * a[1, 0]
    det = a[0, 0] * c00 - a[0, 1] * (a[1, 0] * a[2, 2] - a[1, 2] * a[2, 0]) + a[0, 2] * (a[1, 0] * a[2, 1] - a[1, 1] * a[2, 0])
    return (c00 + c11 + c22) / det


@pytest.mark.parametrize("d", [2, 3])
def test_loader_keeps_the_information_matrix(tmp_path, d):
    path = str(tmp_path / "aniso.g2o")
    write_g2o(path, d)
    G = dpgo_amd.read_g2o(path, 1)
    Om, has = G.edge_information()
    assert has and Om.shape == (3, cr.dof_of(d), cr.dof_of(d))
    kap, tau = G.edges()[4:]
    if d == 2:
        # edge 0 by hand: I11 I12 I13 I22 I23 I33 = 9 2 1 6 -1 5
        assert np.array_equal(Om[0], np.array([[9.0, 2, 1], [2, 6, -1], [1, -1, 5]]))
        for e, rec in enumerate(SE2):
            i11, i12, _, i22, _, i33 = [float(x) for x in rec[5]]
            assert kap[e] == i33 and tau[e] == 2.0 / ((i11 + i22) / (i11 * i22 - i12 * i12))
    else:
        # edge 0 by hand, row by row of the upper triangle
        want = np.array([[9.0, 1, 2, 1, 0, -1], [1, 8, 1, 0, 2, 0], [2, 1, 7, 0, 0, 1], [1, 0, 0, 6, 1, 0], [0, 2, 0, 1, 5, 1],
                         [-1, 0, 1, 0, 1, 4]])
        assert np.array_equal(Om[0], want)
        for e in range(3):
            assert tau[e] == 3.0 / trace_inv3(Om[e][:3, :3]) and kap[e] == 3.0 / (2.0 * trace_inv3(Om[e][3:, 3:]))
    for e in range(3):
        assert np.array_equal(Om[e], Om[e].T)
    # filter_edges and scale_edges carry it along
    Gf = G.filter_edges(np.array([1, 0, 1], np.uint8))
    Of, hf = Gf.edge_information()
    assert hf and np.array_equal(Of, Om[[0, 2]])
    w = np.array([0.5, 2.0, 3.0])
    Gs = G.scale_edges(w)
    Os, hs = Gs.edge_information()
    assert hs and np.array_equal(Os, Om * w[:, None, None])
    assert np.array_equal(Gs.edges()[4], kap * w) and np.array_equal(Gs.edges()[5], tau * w)


@pytest.mark.parametrize("d", [2, 3])
def test_from_edges_info_round_trips_and_a_graph_without_uses_omega_iso(d):
    E, X, _ = mi.chain(d, 65)
    G = graph_of(E)
    Om, has = G.edge_information()
    assert has and np.array_equal(Om, E["Om"])
    for a, b in zip(G.edges(), (E["I"], E["J"], E["R"], E["t"], E["kappa"], E["tau"])):
        assert np.array_equal(a, b)
    keep = (np.arange(65) % 3 != 0).astype(np.uint8)
    assert np.array_equal(G.filter_edges(keep).edge_information()[0], E["Om"][keep.astype(bool)])
    G0 = graph_of(E, info=False)
    O0, h0 = G0.edge_information()
    assert not h0 and np.array_equal(O0, mr.omega_iso(d, E["kappa"], E["tau"]))
    assert not G0.filter_edges(keep).edge_information()[1] and not G0.scale_edges(np.ones(65)).edge_information()[1]
    # ... and evaluates with it
    iso = dict(E, Om=O0)
    ref = mr.edges_all(iso, X, LD)
    got = dpgo_amd.ml_edge_debug(G0, X)
    held = np.arange(65) != 4   # (the edge near pi is not held)
    assert np.all(np.abs(got["chi2"] - ref["chi2"].astype(np.float64))[held] <= CONSTANTS["chi2"] * mr.edge_bounds(iso, X, ref)["chi2"][held])
    with pytest.raises(ValueError):
        dpgo_amd.graph_from_edges(d, E["N"], E["I"], E["J"], E["R"], E["t"], E["kappa"], E["tau"], 1, info=E["Om"][:3])


# ---------------------------------------------------------------------------------------------------------------
# the restatement against central differences
# ---------------------------------------------------------------------------------------------------------------
def central(f, h):
    """(the central difference of f at 0 with step h, its truncation floor): the floor is h^2 / 6 times the third derivative,
    taken from the five-point stencil at H = 1e-2 and doubled for that estimate's own error, as test_polish_host.py takes it."""
    H = 1e-2
    third = np.abs(f(2 * H) - 2 * f(H) + 2 * f(-H) - f(-2 * H)) / (2 * H ** 3)
    return (f(h) - f(-h)) / (2 * h), 2.0 * h * h / 6.0 * third


@pytest.mark.parametrize("d", [2, 3])
def test_restated_jacobians_are_the_central_differences_of_r(d):
    """Ji, Jj of every edge of a 65-edge chain (rotation errors on both sides of the series' threshold, exactly zero, and
    0.1) against central differences of the long-double r along each unknown, h = 1e-5: within 1e-6 of the column's largest
    entry plus the difference's truncation floor plus the fp64 rounding of the retracted pose, U (1 + |t_j - t_i|) / h."""
    E, X, _ = mi.chain(d, 65)
    dof, N, h = cr.dof_of(d), E["N"], 1e-5
    P = mr.poses_of(X, d)
    worst = 0.0
    for e in [0, 1, 2, 3, 32, 33, 64]:
        i, j = int(E["I"][e]), int(E["J"][e])
        r, Ji, Jj, _ = mr.edge(d, E["R"][e], E["t"][e], P[i], P[j])
        for role, J in ((0, Ji), (1, Jj)):
            for a in range(dof):
                def f(s, role=role, a=a):
                    v = np.zeros(dof * N)
                    v[dof * (j if role else i) + a] = s
                    Q = mr.poses_of(cr.retract(X, v, d), d)
                    return mr.edge(d, E["R"][e], E["t"][e], Q[i], Q[j], LD)[0]
                fd, floor = central(f, h)
                tol = 1e-6 * max(np.abs(J[:, a]).max(), 1.0) + floor.astype(np.float64) + U * (1 + np.linalg.norm(P[j][0] - P[i][0])) / h
                err = np.abs(fd.astype(np.float64) - J[:, a])
                worst = max(worst, float((err / tol).max()))
                assert np.all(err <= tol), (e, role, a, err, tol)
    print("d = %d: the worst column at %.3g of its tolerance" % (d, worst))
    assert worst > 0


@pytest.mark.parametrize("name", ["tinyGrid3D", "ladder2"])
def test_restated_gradient_is_the_central_difference_of_F_ml(fixtures_dir, name):
    """g'v against (F_ml(retract(X, h v)) - F_ml(retract(X, -h v))) / 2h, F_ml in long double, five seeded directions, h =
    1e-5, at the chordal point: within 1e-6 |g'v| plus the truncation floor plus the rounding of the retracted points, U |X|_F
    times the edges' gradient terms (no cancellation) / h.  A gradient of the wrong sign has to fail on at least three."""
    E = mi.ladder(2) if name == "ladder2" else mi.fixture(fixtures_dir, name)
    X = chordal_point(E)
    d = E["d"]
    per = mr.edges_all(E, X)
    F, g, H = mr.assemble(E, X, per_edge=per)
    rng = np.random.default_rng(29)
    h, told = 1e-5, 0
    rounding = U * float(np.linalg.norm(X)) * float(np.sqrt((per["grad"] ** 2).sum())) * np.sqrt(len(E["I"])) / h
    for _ in range(5):
        v = rng.standard_normal(len(g))
        v /= np.linalg.norm(v)
        fd, floor = central(lambda s: mr.objective(E, cr.retract(X, s * v, d), LD), h)
        gv = float(g @ v)
        tol = 1e-6 * abs(gv) + float(floor) + rounding
        told += 2 * abs(gv) > tol
        print("%s: g'v %.9g, central difference %.9g, difference %.3g, tolerance %.3g" % (name, gv, float(fd), abs(float(fd) - gv), tol))
        assert abs(float(fd) - gv) <= tol
    assert told >= 3
    # H is the Gauss-Newton matrix: symmetric, positive semidefinite, and 2 F_ml = sum chi2
    assert np.array_equal(H, H.T) or np.abs(H - H.T).max() <= 64 * U * np.abs(H).max()
    assert np.linalg.eigvalsh(0.5 * (H + H.T)).min() >= -1e-9 * np.abs(H).max()
    assert abs(2 * F - per["chi2"].sum()) <= 4 * U * per["chi2"].sum()


def test_omega_iso_matches_the_chordal_objective_to_second_order(fixtures_dir):
    """At the noise-free point plus a small tangent step s v, F_ml with Omega_iso and the project's F = 1/2 <X, M X> agree to
    O(s^4) relative to their O(s^2) value: |Exp(hat w) - I|_F^2 = 2 |w|^2 + O(|w|^4)."""
    for d in (2, 3):
        E, X = mi.noise_free(d)
        from oracle import g2o as og
        from oracle.hash import Options as OOptions
        from oracle.problem import LOSS_NONE
        from oracle.star import GlobalProblem
        z = np.zeros(len(E["I"]), np.int64)
        gp = GlobalProblem(E["N"], og.Measurements(z, E["I"], z, E["J"], E["R"], E["t"], E["kappa"], E["tau"]), 1,
                           OOptions.driver(LOSS_NONE, True))
        v = np.random.default_rng(3).standard_normal(cr.dof_of(d) * E["N"])
        v /= np.linalg.norm(v)
        assert float(mr.objective(E, X)) == 0.0
        for s in (1e-2, 1e-3):
            Z = cr.retract(X, s * v, d)
            Fml, Fc = float(mr.objective(E, Z)), nr.objective(gp.M, Z)
            print("d = %d, s = %g: F_ml %.12g, F %.12g" % (d, s, Fml, Fc))
            assert abs(Fml - Fc) <= 10 * s * s * Fc


# ---------------------------------------------------------------------------------------------------------------
# the host twin and the constants
# ---------------------------------------------------------------------------------------------------------------
def held_edges(E, ref):
    """Edges whose rotation residual is within 1e-3 of pi are not held (ml.h): theta > pi - 1e-3, the kernel's own test."""
    d = E["d"]
    return np.linalg.norm(np.asarray(ref["r"], np.float64)[:, d:], axis=1) <= np.pi - mr.NEAR_PI


def ratios(got, ref, bnd, held):
    out = {}
    for k in ("r", "wr", "chi2", "Ji", "Jj", "grad", "blocks"):
        err = np.abs(np.asarray(got[k], LD) - ref[k]).astype(np.float64)[held]
        b = bnd[k][held]
        assert np.all(err[b == 0] == 0), k   # structural zeros (and the d = 2 rotation entries) are exact
        out[k] = float((err[b > 0] / b[b > 0]).max()) if np.any(b > 0) else 0.0
    return out


def test_host_twin_against_the_long_double_restatement(fixtures_dir):
    for name, E, X in ops_inputs(fixtures_dir):
        ref = mr.edges_all(E, X, LD)
        bnd = mr.edge_bounds(E, X, ref)
        got = dpgo_amd.ml_edge_debug(graph_of(E), X)
        rr = ratios(got, ref, bnd, held_edges(E, ref))
        print(name, " ".join("%s %.3g" % kv for kv in rr.items()))
        for k, v in rr.items():
            assert v <= CONSTANTS[k], (name, k, v)
        assert got["near_pi"] == ref["near_pi"]
        if name.startswith("noise_free"):
            assert not got["r"].any() and not got["chi2"].any() and not got["grad"].any()
        # the blocks of a symmetric pair have the same bits
        assert np.array_equal(got["blocks"][:, 1], np.transpose(got["blocks"][:, 2], (0, 2, 1)))
        for ab in (0, 3):
            assert np.array_equal(got["blocks"][:, ab], np.transpose(got["blocks"][:, ab], (0, 2, 1)))


def test_constants_of_the_rounding_bounds(fixtures_dir):
    """The largest gap between the fp64 and the long-double restatement of each output over the inputs, in units of its derived
    bound; times 4, rounded up to a power of two, it is the recorded constant."""
    worst = {k: 0.0 for k in CONSTANTS}
    for name, E, X in ops_inputs(fixtures_dir):
        ref = mr.edges_all(E, X, LD)
        bnd = mr.edge_bounds(E, X, ref)
        got = mr.edges_all(E, X)
        held = held_edges(E, ref)
        for k, v in ratios(got, ref, bnd, held).items():
            worst[k] = max(worst[k], v)
        if not held.all():
            continue   # (the sums of a graph with an edge near pi are not held either)
        for anchor in (None, 0):
            Fr, gr, Hr = mr.assemble(E, X, anchor, LD, per_edge=ref)
            F, g, H = mr.assemble(E, X, anchor, per_edge=got)
            bF, bg, bH = mr.sum_bounds(E, E["N"], ref, bnd)
            if bF > 0:
                worst["F"] = max(worst["F"], abs(float(F - Fr)) / bF)
            eg, eH = np.abs(g - gr).astype(np.float64), np.abs(H - Hr).astype(np.float64)
            worst["g"] = max(worst["g"], float((eg[bg > 0] / bg[bg > 0]).max()) if np.any(bg > 0) else 0.0)
            worst["H"] = max(worst["H"], float((eH[bH > 0] / bH[bH > 0]).max()) if np.any(bH > 0) else 0.0)
    for k, v in worst.items():
        c = 2.0 ** np.ceil(np.log2(4 * v)) if v > 0 else 0.0
        print("%s: worst gap %.3g of the bound, times 4 and rounded up: %g (recorded %g)" % (k, v, c, CONSTANTS[k]))
        assert c == CONSTANTS[k], (k, v, c)


# ---------------------------------------------------------------------------------------------------------------
# the trajectories the GPU tests replay
# ---------------------------------------------------------------------------------------------------------------
_traj = {}


def trajectory(fixtures_dir, name):
    if name not in _traj:
        E, X = iso_point(fixtures_dir, name)
        _traj[name] = mr.polish_full(E, X, anchor=0, max_steps=WHOLE[name][1])
    return _traj[name]


@pytest.mark.parametrize("name", list(WHOLE))
def test_trajectory_decisions_sit_away_from_their_alternatives(fixtures_dir, name):
    """Every accept / reject, every change of mu and every convergence decision of the restated refinement from the isotropic
    polished point sits at least 4 x CONSTANT x its rounding bound from the alternative: a condition on the inputs (their
    seed, ml_inputs.SEED), so that the device's trajectory can be held to the restatement's exactly."""
    r = trajectory(fixtures_dir, name)
    print("%s: outcome %d, %d steps, %d factorisations, F_ml %.9g -> %.9g, |g| %.3g -> %.3g" %
          (name, r["outcome"], r["steps"], r["factorisations"], r["F_initial"], r["F_final"], r["grad_initial"], r["grad_final"]))
    assert r["outcome"] == (nr.MAX_STEPS if name == "ladder2" else nr.CONVERGED) and r["steps"] >= 1 and r["indefinite"] == 0
    assert r["F_final"] <= r["F_initial"]
    for kind, dist, bound in r["decisions"]:
        c = CONSTANTS["g"] if kind == "converged" else CONSTANTS["F"]
        print("  %-9s distance %.3g, bound %.3g" % (kind, dist, c * bound))
        assert dist >= 4 * c * bound, (kind, dist, bound)


# ---------------------------------------------------------------------------------------------------------------
# refusals and the C ABI
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 3])
def test_an_information_matrix_that_is_not_spd_is_refused_by_name(capfd, d):
    E, X, _ = mi.chain(d, 65)
    for kind in ("indefinite", "asymmetric"):
        Om = E["Om"].copy()
        if kind == "indefinite":
            Om[37, 0, 0] = -Om[37, 0, 0]
        else:
            Om[37, 0, 1] += 1e-6 * Om[37, 0, 0]
        G = graph_of(dict(E, Om=Om))
        capfd.readouterr()
        with pytest.raises(ValueError):
            dpgo_amd.ml_edge_debug(G, X)
        assert "edge 37" in capfd.readouterr().err


def test_ml_abi():
    L = dpgo_amd.lib()
    # the polish's struct, a long long, two doubles
    assert C.sizeof(dpgo_amd.MlResult) == C.sizeof(dpgo_amd.PolishResult) + 24
    r = dpgo_amd.MlResult()
    assert r.outcome == 0 and r.polish.steps == 0 and r.near_pi == 0
    X = np.zeros((8, 3), order="F")
    dp = X.ctypes.data_as(C.POINTER(C.c_double))
    o = dpgo_amd.PolishOptions()
    cov = dpgo_amd.CovResult()
    nnz = C.c_longlong(0)
    E, Xc, _ = mi.chain(3, 1)
    G = graph_of(E)
    for grp in (None, C.c_void_p(0)):
        assert L.dpgo_group_ml_polish(grp, G._h, dp, 8, C.byref(o), 0, dp, 8, None, 0, C.byref(r)) == -1
        assert L.dpgo_group_ml_covariance(grp, G._h, dp, 8, 0, 0, None, 0, dp, None, C.byref(cov)) == -1
        assert L.dpgo_group_ml_hessian(grp, G._h, dp, 8, 0, None, None, None, 0, C.byref(nnz), None, None) == -1
        assert L.dpgo_group_ml_eval(grp, G._h, dp, 8, None, None, None, None, None, None, None) == -1
    assert L.dpgo_debug_ml_edge_host(None, dp, 8, *[None] * 8) == -1
    assert L.dpgo_debug_ml_edge_host(G._h, dp, 3, *[None] * 8) == -1   # (a short X)
    assert L.dpgo_graph_edge_information(None, None, None) == -1
    assert L.dpgo_group_debug_ml_hessian_guarded(None, G._h, dp, 8, 0, 4, 1.0, dp, dp, 8) == -1
    h = C.c_void_p()
    assert L.dpgo_graph_from_edges_info(3, 2, 1, None, None, None, None, None, None, None, 1, C.byref(h)) == -1
    header = open(os.path.join(os.path.dirname(dpgo_amd.__file__), "..", "include", "dpgo_amd.h")).read()
    for sym in ("dpgo_graph_from_edges_info", "dpgo_graph_edge_information", "dpgo_group_ml_polish", "dpgo_group_ml_covariance",
                "dpgo_group_ml_hessian", "dpgo_group_ml_eval", "dpgo_debug_ml_edge_host", "dpgo_group_debug_ml_hessian_guarded"):
        assert sym + "(" in header and sym in dpgo_amd.SYMBOLS and hasattr(L, sym)
    for name in ("ml_polish", "ml_covariance", "ml_hessian", "ml_eval"):
        assert hasattr(dpgo_amd.NodeGroup, name)
    assert hasattr(dpgo_amd.Graph, "edge_information") and hasattr(dpgo_amd.Graph, "from_edges") and hasattr(dpgo_amd, "ml_edge_debug")
