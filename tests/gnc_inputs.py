"""Inputs of the tests of graduated non-convexity (tests/test_gnc_host.py, tests/test_gpu_gnc*.py): test infrastructure.
`chain` is a trajectory with loop closures of which a seeded part of the inter-node ones are gross outliers; `case` hands out
(P, X, outlier mask) and `reference` the restated runs, computed once per process and handed out unchanged.

TABLE is what tests/gnc_restatement.run gives on the four inputs with c2 = 4, mu_step = 1.4 and the inner options at the
polish's defaults; tests/test_gnc_host.py holds the restatement to it.  In every row exactly the injected outliers are
rejected (w == 0 under TLS, s > c2 under GM) and every inner solve CONVERGED.
"""
import os

import numpy as np

import edge_restatement as er
import gnc_restatement as gr
import robust_restatement as rr

from dpgo_amd import synthetic

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
C2, MU_STEP = 4.0, 1.4
CASES = {"c3_40": (3, 40, 40, 4, 1), "c2_40": (2, 40, 40, 4, 2), "c3_24": (3, 24, 30, 3, 3), "c3_150": (3, 150, 150, 2, 4)}
# name: (edges, in R, outliers, TLS levels, GM levels)
TABLE = {"c3_40": (79, 36, 6, 18, 22), "c2_40": (79, 36, 14, 15, 20), "c3_24": (53, 27, 4, 17, 22), "c3_150": (299, 82, 23, 20, 22)}

_cases, _refs = {}, {}


def chain(d, N, nclos, nn, seed, out_frac=0.3):
    """dict(d, N, I, J, R, t, kappa, tau, X, outlier): N - 1 odometry edges and nclos closures (i, (i + U[2, N-1)) mod N) of a
    ground truth (random rotations, translations a cumulative sum of U(-1, 1)); every inter-node closure is with probability
    out_frac a gross outlier (a random rotation, translation noise 3 N(0, 1)); the rest carries random_graph's noise (I + 0.02 N
    orthonormalised with det +1, translation noise 0.03 N); kappa ~ U(50, 200), tau ~ U(50, 100); X is the ground truth with
    0.01 N added to the translations."""
    rng = np.random.default_rng(seed)
    Rg = synthetic._random_rotations_d(rng, N, d)
    tg = np.cumsum(rng.uniform(-1, 1, (N, d)), axis=0)
    ci = rng.integers(0, N, nclos)
    cj = (ci + rng.integers(2, N - 1, nclos)) % N
    I, J = np.concatenate([np.arange(N - 1), ci]), np.concatenate([np.arange(1, N), cj])
    m = len(I)
    inter = er.inter_mask(N, nn, I, J)
    closure = np.arange(m) >= N - 1
    outlier = closure & inter & (rng.uniform(size=m) < out_frac)
    noise = synthetic._random_rotations_d(rng, m, d)
    small = np.eye(d) + 0.02 * rng.standard_normal((m, d, d))
    Rn = np.where(outlier[:, None, None], noise, small)
    Q = []
    for a in Rn:
        q, r = np.linalg.qr(a)
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, -1] = -q[:, -1]
        Q.append(q)
    R = np.einsum("eji,ejk,ekl->eil", Rg[I], Rg[J], np.stack(Q))
    t = np.einsum("eji,ej->ei", Rg[I], tg[J] - tg[I]) + np.where(outlier[:, None], 3.0, 0.03) * rng.standard_normal((m, d))
    kappa, tau = rng.uniform(50, 200, m), rng.uniform(50, 100, m)
    X = synthetic.global_X(Rg, tg + 0.01 * rng.standard_normal((N, d)))
    return dict(d=d, N=N, I=I, J=J, R=R, t=t, kappa=kappa, tau=tau, X=np.asfortranarray(X), outlier=outlier, nn=nn)


def case(name, out_frac=0.3):
    """(P of robust_restatement, the start X, the injected outliers)."""
    key = (name, out_frac)
    if key not in _cases:
        d, N, nclos, nn, seed = CASES[name]
        g = chain(d, N, nclos, nn, seed, out_frac)
        _cases[key] = (rr.problem(d, N, g["I"], g["J"], g["R"], g["t"], g["kappa"], g["tau"], nn), g["X"], g["outlier"])
    return _cases[key]


def perturbed(X, seed=77):
    """X (1 + 1e-12 xi), xi seeded Gaussians."""
    return np.asfortranarray(X * (1.0 + 1e-12 * np.random.default_rng(seed).standard_normal(X.shape)))


SCALARS = ("outcome", "levels", "steps", "factorisations", "num_outliers", "mu_initial", "mu_final", "s_max_initial", "F_initial",
           "margin")


def compute(name, kind):
    """The restated run from the case's start, with `spread`: D_k, the per-level spread of the four logged F values between that
    run and the run from perturbed(X) -- (levels, 4), columns F_mu(X_{k-1}), F_w(X_{k-1}), F_w(X_k), F_mu(X_k) -- and
    `same_counts`: whether the two runs agree in outcome, levels and every per-level count."""
    P, X, _ = case(name)
    a, b = gr.run(P, X, kind, C2, mu_step=MU_STEP), gr.run(P, perturbed(X), kind, C2, mu_step=MU_STEP)
    # (the counts of the weights, columns 7 ..: the number of inner steps of a level may differ by one where |g| meets its tolerance)
    a["same_counts"] = bool(a["outcome"] == b["outcome"] and a["levels"] == b["levels"] and np.array_equal(a["log"][:, 7:], b["log"][:, 7:]))
    a["same_steps"] = bool(np.array_equal(a["log"][:, 5:7], b["log"][:, 5:7]))
    k = min(a["levels"], b["levels"])
    a["spread"] = np.abs(a["log"][:k, 1:5] - b["log"][:k, 1:5])
    return a


def pack(name, kind, run):
    """A run as the arrays of tests/golden/gnc_reference.npz."""
    p = "%s_%d_" % (name, kind)
    return {p + "log": run["log"], p + "w": run["w"], p + "X": run["X"], p + "spread": run["spread"],
            p + "inner": np.array(run["inner"], np.int64), p + "scalars": np.array([float(run[k]) for k in SCALARS]),
            p + "same_counts": np.array(run["same_counts"]), p + "same_steps": np.array(run["same_steps"])}


def reference(name, kind):
    """The committed restated run of (name, kind), in compute()'s fields (tests/golden/make_gnc_reference.py)."""
    key = (name, kind)
    if key not in _refs:
        z = np.load(os.path.join(GOLDEN, "gnc_reference.npz"))
        p = "%s_%d_" % (name, kind)
        r = {k: z[p + k] for k in ("log", "w", "X", "spread")}
        r["inner"] = z[p + "inner"].tolist()
        r["same_counts"], r["same_steps"] = bool(z[p + "same_counts"]), bool(z[p + "same_steps"])
        for k, v in zip(SCALARS, z[p + "scalars"]):
            r[k] = float(v) if k in ("mu_initial", "mu_final", "s_max_initial", "F_initial", "margin") else int(v)
        _refs[key] = r
    return _refs[key]
