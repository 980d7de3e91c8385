"""Inputs of the tests of graduated non-convexity on the maximum-likelihood objective (tests/test_ml_gnc_host.py,
tests/test_gpu_ml_gnc*.py): test infrastructure.  `chain` is gnc_inputs.chain's trajectory with loop closures, with these
changes: every edge carries a full information matrix (ml_inputs.information: correlated, condition numbers up to 100, every
fifth edge exactly isotropic, the middle edge scaled by 1e4); every inlier's noise is drawn from N(0, Omega_e^-1) IN THE
RESIDUAL'S OWN COORDINATES,

    R~ = R_i^T R_j Exp(-eps_R),    t~ = R_i^T (t_j - t_i) - R~ eps_t      =>  r_e(ground truth) = (eps_t, eps_R)

so that chi2_e ~ chi2_dof at the ground truth; every closure of the robust set is with probability 0.2 a gross outlier (a
rotation error of norm U(0.5, 1.5), a translation error 3 N(0, 1), through the same two formulas).  The robust set is the
closures, handed over as a robust_set array -- except in the case on 3 nodes, which uses the inter-node rule of edges.h
(robust_set None): every inter-node edge is in the robust set, the two odometry edges between nodes included, and only the
inter-node closures can be outliers.

c2 is the chi2_dof quantile at 0.999: 16.266 (d = 2, dof 3) or 22.458 (d = 3, dof 6); mu_step = 1.4; the inner options are the
polish's defaults.  `reference` hands out the committed restated runs (tests/golden/make_ml_gnc_reference.py).
"""
import os

import numpy as np

import cov_restatement as cr
import edge_restatement as er
import gnc_inputs as gi
import ml_gnc_restatement as mgr
import ml_inputs as mi

from dpgo_amd import synthetic

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
C2 = {2: 16.266, 3: 22.458}
MU_STEP = 1.4
# name: (d, N, closures, nodes, seed, inter-node rule)
CASES = {"m3_24": (3, 24, 30, 1, 31, False), "m2_40": (2, 40, 40, 1, 42, False), "m3_40x3": (3, 40, 40, 3, 23, True)}
RUNS = [("m3_24", mgr.TLS), ("m3_24", mgr.GM), ("m2_40", mgr.TLS), ("m2_40", mgr.GM), ("m3_40x3", mgr.TLS)]
SMALLEST = ("m3_24", mgr.TLS)

_cases, _refs = {}, {}


def chain(d, N, nclos, nn, seed, inter_rule=False, out_frac=0.2):
    """(E of ml_restatement with nn, X, R, outlier): N - 1 odometry edges and nclos closures of gnc_inputs.chain's ground truth.
    R: the robust set (bool per edge); X: the ground truth with 0.01 N added to the translations."""
    rng = np.random.default_rng(seed)
    dof = cr.dof_of(d)
    Rg = synthetic._random_rotations_d(rng, N, d)
    tg = np.cumsum(rng.uniform(-1, 1, (N, d)), axis=0)
    ci = rng.integers(0, N, nclos)
    cj = (ci + rng.integers(2, N - 1, nclos)) % N
    I, J = np.concatenate([np.arange(N - 1), ci]), np.concatenate([np.arange(1, N), cj])
    m = len(I)
    closure = np.arange(m) >= N - 1
    R = er.inter_mask(N, nn, I, J) if inter_rule else closure      # (the inter-node rule takes the odometry edges between nodes too)
    outlier = R & closure & (rng.uniform(size=m) < out_frac)
    kappa, tau = rng.uniform(50, 200, m), rng.uniform(50, 100, m)
    Om = mi.information(d, kappa, tau, seed + 1000)
    Rm, tm = np.zeros((m, d, d)), np.zeros((m, d))
    for e in range(m):
        if outlier[e]:
            er_ = rng.standard_normal(dof - d)
            er_ *= rng.uniform(0.5, 1.5) / np.linalg.norm(er_)
            eps = np.concatenate([3.0 * rng.standard_normal(d), er_])
        else:
            L = np.linalg.cholesky(Om[e])               # Omega = L L^T:  eps = L^-T z  has covariance Omega^-1
            eps = np.linalg.solve(L.T, rng.standard_normal(dof))
        i, j = I[e], J[e]
        Rm[e] = Rg[i].T @ Rg[j] @ mi.rotation(-eps[d:], d)
        tm[e] = Rg[i].T @ (tg[j] - tg[i]) - Rm[e] @ eps[:d]
    X = synthetic.global_X(Rg, tg + 0.01 * rng.standard_normal((N, d)))
    E = dict(d=d, N=N, I=I.astype(np.int32), J=J.astype(np.int32), R=Rm, t=tm, kappa=kappa, tau=tau, Om=Om, nn=nn)
    return E, np.asfortranarray(X), R, outlier


def case(name):
    """(E, the start X, R, the injected outliers, the robust_set argument of the library call: None under the inter-node rule)."""
    if name not in _cases:
        d, N, nclos, nn, seed, inter_rule = CASES[name]
        E, X, R, outlier = chain(d, N, nclos, nn, seed, inter_rule)
        _cases[name] = (E, X, R, outlier, None if inter_rule else R.astype(np.int32))
    return _cases[name]


def pendant(name="m3_24", a=3, b=15, err=3.0):
    """(E, X, R): the case with one more pose, held by two robust edges of the same isotropic Omega whose measurements
    contradict each other symmetrically (the pose's translation from a and from b differ by 2 err along one axis).  Both edges
    are gross outliers of equal chi2, so GNC-TLS drops both AT THE SAME LEVEL: that level's H_w has a zero diagonal block -- a
    rank-deficient level.  (One robust edge alone can never disconnect a pose: a pose held by a single edge fits it exactly.)"""
    E, X, R, _, _ = case(name)
    d, N = E["d"], E["N"]
    P = [(X[p], X[N + d * p:N + d * p + d]) for p in range(N)]
    tn = 0.5 * (P[a][0] + P[b][0])
    Rm, tm = [], []
    for p, sign in ((a, 1.0), (b, -1.0)):
        shift = np.zeros(d)
        shift[0] = sign * err
        Rm.append(np.array(P[p][1]))                      # R_p^T I: the new pose's rotation is the identity
        tm.append(P[p][1] @ (tn + shift - P[p][0]))
    kap, tau = np.array([50.0, 50.0]), np.array([100.0, 100.0])
    Om = np.zeros((2, cr.dof_of(d), cr.dof_of(d)))
    for k in range(cr.dof_of(d)):
        Om[:, k, k] = tau if k < d else 2 * kap
    E2 = dict(E, N=N + 1, I=np.concatenate([E["I"], [a, b]]).astype(np.int32), J=np.concatenate([E["J"], [N, N]]).astype(np.int32),
              R=np.concatenate([E["R"], np.array(Rm)]), t=np.concatenate([E["t"], np.array(tm)]),
              kappa=np.concatenate([E["kappa"], kap]), tau=np.concatenate([E["tau"], tau]), Om=np.concatenate([E["Om"], Om]))
    Rs = [np.array(P[p][1]).T for p in range(N)] + [np.eye(d)]
    return E2, np.asfortranarray(mi.point(d, np.vstack([X[:N], tn[None]]), Rs)), np.concatenate([R, [True, True]])


perturbed = gi.perturbed
SCALARS = gi.SCALARS + ("decision_margin", "theta_max", "near_pi", "near_pi_all")
FLOATS = ("mu_initial", "mu_final", "s_max_initial", "F_initial", "margin", "decision_margin", "theta_max")


def compute(name, kind, polish=None):
    """The restated run from the case's start, with `spread` (D_k: the per-level spread of the four logged F values against the
    run from perturbed(X)), `same_counts` (outcome, levels and every per-level count agree) and `same_steps` (the inner steps
    and outcomes agree too), as gnc_inputs.compute."""
    E, X, R, _, _ = case(name)
    c2 = C2[E["d"]]
    a = mgr.run(E, X, kind, c2, R, mu_step=MU_STEP, polish=polish)
    b = mgr.run(E, perturbed(X), kind, c2, R, mu_step=MU_STEP, polish=polish)
    a["same_counts"] = bool(a["outcome"] == b["outcome"] and a["levels"] == b["levels"] and np.array_equal(a["log"][:, 7:], b["log"][:, 7:]))
    a["same_steps"] = bool(a["same_counts"] and np.array_equal(a["log"][:, 5:7], b["log"][:, 5:7]))
    k = min(a["levels"], b["levels"])
    a["spread"] = np.abs(a["log"][:k, 1:5] - b["log"][:k, 1:5])
    a["theta_max"] = max(a["theta_max"], b["theta_max"])
    return a


def pack(name, kind, run):
    """A run as the arrays of tests/golden/ml_gnc_reference.npz."""
    p = "%s_%d_" % (name, kind)
    return {p + "log": run["log"], p + "w": run["w"], p + "X": run["X"], p + "spread": run["spread"],
            p + "inner": np.array(run["inner"], np.int64), p + "scalars": np.array([float(run[k]) for k in SCALARS]),
            p + "same_counts": np.array(run["same_counts"]), p + "same_steps": np.array(run["same_steps"])}


def reference(name, kind):
    """The committed restated run of (name, kind), in compute()'s fields."""
    key = (name, kind)
    if key not in _refs:
        z = np.load(os.path.join(GOLDEN, "ml_gnc_reference.npz"))
        p = "%s_%d_" % (name, kind)
        r = {k: z[p + k] for k in ("log", "w", "X", "spread")}
        r["inner"] = z[p + "inner"].tolist()
        r["same_counts"], r["same_steps"] = bool(z[p + "same_counts"]), bool(z[p + "same_steps"])
        for k, v in zip(SCALARS, z[p + "scalars"]):
            r[k] = float(v) if k in FLOATS else int(v)
        _refs[key] = r
    return _refs[key]
