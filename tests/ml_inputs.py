"""Inputs of the maximum-likelihood tests (tests/test_ml_host.py, tests/test_gpu_ml_*.py): the fixtures' and the ladders' edges
with a seeded symmetric positive definite Omega_e attached, a noise-free graph whose every residual is exactly zero, and
chains built for the edge kernel's branches.  numpy only; every input is a dict E = dict(d, N, I, J, R, t, kappa, tau, Om)
(tests/ml_restatement.py) and is built once.
"""
import os

import numpy as np
import scipy.linalg as sla

import cov_restatement as cr
import ml_restatement as mr

SEED = 20261021
_cache = {}


def information(d, kappa, tau, seed):
    """Per edge a dof x dof SPD matrix Q diag(lambda) Q^T: Q a seeded random rotation of the whole residual space (so
    translation and rotation are correlated), lambda log-uniform over a factor of up to 100 above min(tau, 2 kappa).  Every
    fifth edge is exactly Omega_iso = diag(tau I, 2 kappa I); the edge in the middle is scaled by 1e4.  Symmetric to the bit."""
    rng = np.random.default_rng(seed)
    m, dof = len(kappa), cr.dof_of(d)
    Om = mr.omega_iso(d, kappa, tau)
    for e in range(m):
        if e % 5 == 0:
            continue
        Q, Rq = np.linalg.qr(rng.standard_normal((dof, dof)))
        Q = Q * np.sign(np.diag(Rq))
        lam = min(tau[e], 2 * kappa[e]) * 100.0 ** rng.uniform(0, 1, dof)
        lam[0], lam[-1] = lam.min(), lam.min() * 100.0 ** rng.uniform(0.5, 1)   # (condition numbers up to 100, never above)
        A = (Q * lam) @ Q.T
        Om[e] = 0.5 * (A + A.T)
    Om[m // 2] *= 1e4
    return Om


def with_information(d, N, I, J, R, t, kappa, tau, seed=SEED):
    kappa, tau = np.asarray(kappa, np.float64), np.asarray(tau, np.float64)
    return dict(d=d, N=int(N), I=np.asarray(I, np.int32), J=np.asarray(J, np.int32), R=np.asarray(R, np.float64),
                t=np.asarray(t, np.float64), kappa=kappa, tau=tau, Om=information(d, kappa, tau, seed))


def fixture(fixtures_dir, name):
    """A .g2o fixture's edges through the oracle's reader, with `information` attached."""
    from oracle import g2o as og
    if name not in _cache:
        N, mm = og.read_g2o_file(os.path.join(fixtures_dir, name + ".g2o"))
        _cache[name] = with_information(mm.d, N, mm.ipose, mm.jpose, mm.R, mm.t, mm.kappa, mm.tau)
    return _cache[name]


def ladder(d):
    """synthetic.ladder(d) compacted to the poses it uses (the row-degree and shared-block cases: parallel and reversed edges)."""
    from dpgo_amd import synthetic
    key = "ladder%d" % d
    if key not in _cache:
        g = synthetic.ladder(d)
        used = np.unique(np.concatenate([g["I"], g["J"]]))
        new = np.full(g["num_poses"], -1, np.int64)
        new[used] = np.arange(len(used))
        E = with_information(d, len(used), new[g["I"]], new[g["J"]], g["R"], g["t"], g["kappa"], g["tau"])
        E["num_nodes"] = int(g["num_nodes"])
        _cache[key] = E
    return _cache[key]


def rotation(w, d):
    return sla.expm(cr.hat(np.atleast_1d(w), d))


def point(d, t, Rs):
    """The reference layout: row p the translation, rows N + d p ... the rows of Y_p = R_p^T."""
    N = len(t)
    X = np.zeros(((d + 1) * N, d))
    X[:N] = t
    for p in range(N):
        X[N + d * p:N + d * p + d] = Rs[p].T
    return X


def noise_free(d):
    """(E with Omega_iso, X): a 4 x 3 grid of poses whose rotations are quarter turns and whose translations are integers,
    every measurement computed from them -- all of it exact in fp64, so every residual is exactly zero."""
    key = "noise_free%d" % d
    if key not in _cache:
        rng = np.random.default_rng(SEED + d)
        N = 12
        t = rng.integers(-4, 5, (N, d)).astype(np.float64)
        Rs = []
        for p in range(N):
            if d == 2:
                k = int(rng.integers(0, 4))
                Rs.append(np.round(rotation(k * np.pi / 2, 2)))
            else:
                ax, k = int(rng.integers(0, 3)), int(rng.integers(0, 4))
                Rs.append(np.round(rotation(k * np.pi / 2 * np.eye(3)[ax], 3)))
        I, J = [], []
        for p in range(N):
            for q in (p + 1, p + 3):
                if q < N and (q != p + 1 or q % 3 != 0):
                    I.append(p)
                    J.append(q)
        I, J = np.array(I), np.array(J)
        R = np.array([Rs[i].T @ Rs[j] for i, j in zip(I, J)])
        tt = np.array([Rs[i].T @ (t[j] - t[i]) for i, j in zip(I, J)])
        kappa, tau = rng.uniform(5, 50, len(I)), rng.uniform(5, 50, len(I))
        E = dict(d=d, N=N, I=I.astype(np.int32), J=J.astype(np.int32), R=R, t=tt, kappa=kappa, tau=tau,
                 Om=mr.omega_iso(d, kappa, tau))
        _cache[key] = (E, point(d, t, Rs))
    return _cache[key]


THETA_BELOW, THETA_ABOVE = 5e-5, 2e-4   # theta^2 = 2.5e-9 and 4e-8: either side of the series' threshold 1e-8


def chain(d, m):
    """(E, X, near_pi): a chain of m edges over m + 1 seeded random poses for the edge kernel.  The measurement of edge e is the
    true relative pose with a rotation error of norm THETA_BELOW (e = 0 mod 4), THETA_ABOVE (1 mod 4) or 0.1 (the rest) and a
    translation error of 0.1.  m >= 3: the last edge joins two poses with identity rotations and integer translations and is
    exact (theta = 0).  m >= 5: edge 4 has a rotation error of pi - 5e-4 and is the one near_pi counts; its values are not held."""
    key = ("chain", d, m)
    if key not in _cache:
        rng = np.random.default_rng(SEED + 100 * d + m)
        N, dr = m + 1, cr.dof_of(d) - d
        t = rng.uniform(-5, 5, (N, d))
        Rs = [rotation(rng.standard_normal(dr), d) for _ in range(N)]
        if m >= 3:
            Rs[N - 2], Rs[N - 1] = np.eye(d), np.eye(d)
            t[N - 2:] = rng.integers(-4, 5, (2, d))
        I, J = np.arange(m), np.arange(1, m + 1)
        R, tt = np.zeros((m, d, d)), np.zeros((m, d))
        near = 0
        for e in range(m):
            w = rng.standard_normal(dr)
            w *= (THETA_BELOW, THETA_ABOVE, 0.1, 0.1)[e % 4] / np.linalg.norm(w)
            dt = 0.1 * rng.standard_normal(d)
            if m >= 5 and e == 4:
                w *= (np.pi - 5e-4) / np.linalg.norm(w)
                near = 1
            if m >= 3 and e == m - 1:
                w, dt = 0.0 * w, 0.0 * dt
            R[e] = Rs[e].T @ Rs[e + 1] @ rotation(-w, d) if np.any(w) else Rs[e].T @ Rs[e + 1]
            tt[e] = Rs[e].T @ (t[e + 1] - t[e]) - dt
        E = with_information(d, N, I, J, R, tt, rng.uniform(5, 50, m), rng.uniform(5, 50, m), seed=SEED + m)
        _cache[key] = (E, point(d, t, Rs), near)
    return _cache[key]


def grid2():
    """A 6 x 5 grid of SE(2) poses whose measurements are the true relative poses with moderate noise (0.03 rad, 0.05 in
    translation): row and column neighbours, eight seeded closures, every fourth edge written reversed.  A d = 2 input whose
    refinement can converge, which the ladder's random measurements do not allow."""
    key = "grid2"
    if key not in _cache:
        rng = np.random.default_rng(SEED + 22)
        nx, ny = 6, 5
        N = nx * ny
        t = np.array([[float(x), float(y)] for y in range(ny) for x in range(nx)]) + 0.1 * rng.standard_normal((N, 2))
        Rs = [rotation(a, 2) for a in rng.uniform(-np.pi, np.pi, N)]
        pairs = [(y * nx + x, y * nx + x + 1) for y in range(ny) for x in range(nx - 1)]
        pairs += [(y * nx + x, (y + 1) * nx + x) for y in range(ny - 1) for x in range(nx)]
        while len(pairs) < (nx - 1) * ny + nx * (ny - 1) + 8:
            p, q = (int(v) for v in rng.integers(0, N, 2))
            if p != q and (p, q) not in pairs and (q, p) not in pairs:
                pairs.append((p, q))
        pairs = [(q, p) if k % 4 == 3 else (p, q) for k, (p, q) in enumerate(pairs)]
        I, J = np.array([p for p, _ in pairs]), np.array([q for _, q in pairs])
        R = np.array([Rs[i].T @ Rs[j] @ rotation(0.03 * rng.standard_normal(), 2) for i, j in pairs])
        tt = np.array([Rs[i].T @ (t[j] - t[i]) + 0.05 * rng.standard_normal(2) for i, j in pairs])
        _cache[key] = with_information(2, N, I, J, R, tt, rng.uniform(5, 50, len(I)), rng.uniform(5, 50, len(I)), seed=SEED + 23)
    return _cache[key]
