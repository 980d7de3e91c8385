"""Synthetic SE(3) lattice pose graphs (BASELINE.json config 4).

Lattice nx x ny x nz, pose id = x + nx*y + nx*ny*z (z-major, so the reference's contiguous
partition gives every node a slab of whole z-layers).  Edges: all 6-neighbour lattice edges plus
loop closures between lattice points at Chebyshev distance <= 2, drawn without replacement, written
i < j.  Ground truth t = (x, y, z), R = I; translation noise N(0, 0.1^2 I), rotation noise
exp(N(0, 0.05^2 I)); information diag(100,100,100,400,400,400) => tau = 100, kappa = 200
(C++/DPGO/src/DPGO_utils.cpp:107-116); `outlier_frac` of the closures are replaced by uniformly
random rotations / translations inside the bounding box.

The headline instance is grid(50, 50, 40, 400_000): 100 000 poses, 293 500 lattice edges + 106 500
closures = 400 000 edges, seed 20240817 (numpy default_rng -- this module defines the instance).
Data generation only; nothing here is on the timed path.
"""
from __future__ import annotations

import numpy as np

HEADLINE = dict(nx=50, ny=50, nz=40, num_edges=400_000, seed=20240817)


def _exp_so3(w):
    th = np.linalg.norm(w, axis=1)
    k = w / np.maximum(th, 1e-300)[:, None]
    K = np.zeros((len(w), 3, 3))
    K[:, 0, 1], K[:, 0, 2] = -k[:, 2], k[:, 1]
    K[:, 1, 0], K[:, 1, 2] = k[:, 2], -k[:, 0]
    K[:, 2, 0], K[:, 2, 1] = -k[:, 1], k[:, 0]
    s, c = np.sin(th)[:, None, None], np.cos(th)[:, None, None]
    return np.eye(3)[None] + s * K + (1 - c) * (K @ K)


def _random_rotations(rng, n):
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    w, x, y, z = q.T
    R = np.empty((n, 3, 3))
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - w * z); R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y); R[:, 2, 1] = 2 * (y * z + w * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def grid(nx, ny, nz, num_edges=None, seed=20240817, outlier_frac=0.02, sigma_t=0.1, sigma_r=0.05,
         tau=100.0, kappa=200.0):
    """Returns dict(d, num_poses, I, J, R, t, kappa, tau, outlier) for graph_from_edges / the oracle."""
    rng = np.random.default_rng(seed)
    N = nx * ny * nz
    x, y, z = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    pid = (x + nx * y + nx * ny * z)
    lat = []
    lat.append((pid[:-1].ravel(), pid[1:].ravel()))
    lat.append((pid[:, :-1].ravel(), pid[:, 1:].ravel()))
    lat.append((pid[:, :, :-1].ravel(), pid[:, :, 1:].ravel()))
    I = np.concatenate([a for a, _ in lat])
    J = np.concatenate([b for _, b in lat])
    n_lat = len(I)
    n_extra = 0 if num_edges is None else num_edges - n_lat
    assert n_extra >= 0
    seen = set((I * N + J).tolist())
    ei, ej = [], []
    while len(ei) < n_extra:
        k = max(2 * (n_extra - len(ei)), 1024)
        a = rng.integers(0, N, k)
        off = rng.integers(-2, 3, (k, 3))
        ax, ay, az = a % nx, (a // nx) % ny, a // (nx * ny)
        bx, by, bz = ax + off[:, 0], ay + off[:, 1], az + off[:, 2]
        ok = (bx >= 0) & (bx < nx) & (by >= 0) & (by < ny) & (bz >= 0) & (bz < nz) & (np.abs(off).sum(1) > 0)
        b = bx + nx * by + nx * ny * bz
        for u, v in zip(a[ok].tolist(), b[ok].tolist()):
            lo, hi = (u, v) if u < v else (v, u)
            key = lo * N + hi
            if key in seen:
                continue
            seen.add(key)
            ei.append(lo)
            ej.append(hi)
            if len(ei) == n_extra:
                break
    I = np.concatenate([I, np.asarray(ei, np.int64)]).astype(np.int64)
    J = np.concatenate([J, np.asarray(ej, np.int64)]).astype(np.int64)
    M = len(I)
    pos = np.stack([I % nx, (I // nx) % ny, I // (nx * ny)], 1).astype(float)
    posj = np.stack([J % nx, (J // nx) % ny, J // (nx * ny)], 1).astype(float)
    R = _exp_so3(sigma_r * rng.standard_normal((M, 3)))          # R_i = R_j = I
    t = (posj - pos) + sigma_t * rng.standard_normal((M, 3))
    outlier = np.zeros(M, bool)
    if n_extra and outlier_frac > 0:
        n_out = int(round(outlier_frac * n_extra))
        sel = n_lat + rng.choice(n_extra, n_out, replace=False)
        outlier[sel] = True
        R[sel] = _random_rotations(rng, n_out)
        t[sel] = rng.uniform(-1, 1, (n_out, 3)) * np.array([nx, ny, nz])
    return dict(d=3, num_poses=N, I=I, J=J, R=R, t=t, kappa=np.full(M, kappa), tau=np.full(M, tau),
                outlier=outlier)


def write_g2o(path, g):
    """EDGE_SE3:QUAT writer so that the same instance can feed any g2o reader."""
    with open(path, "w") as fh:
        for e in range(len(g["I"])):
            R = g["R"][e]
            w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
            if w > 1e-6:
                q = [(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w]
            else:
                ev, evec = np.linalg.eigh((R + R.T) / 2)
                ax = evec[:, -1]
                q = [ax[0], ax[1], ax[2], 0.0]
            ti, ki = g["tau"][e], 2 * g["kappa"][e]
            info = "%g 0 0 0 0 0 %g 0 0 0 0 %g 0 0 0 %g 0 0 %g 0 %g" % (ti, ti, ti, ki, ki, ki)
            fh.write("EDGE_SE3:QUAT %d %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %s\n" % (
                g["I"][e], g["J"][e], *g["t"][e], *q, info))


LADDER_SIZES = (81, 1, 63, 64, 65, 129)   # own poses of the nodes of ladder(); node 0 holds the ladder itself
LADDER_SPAN = 130                          # ids per node (the contiguous partition); ids a node does not use have no edge
LADDER_TOP = 40


def _random_rotations_d(rng, n, d):
    if d == 3:
        return _random_rotations(rng, n)
    th = rng.uniform(-np.pi, np.pi, n)
    c, s = np.cos(th), np.sin(th)
    return np.stack([np.stack([c, -s], 1), np.stack([s, c], 1)], 1)


def ladder(d=3, seed=7):
    """A 6-node SE(d) graph whose rows cover every length the row kernels split differently (for operator tests).

    Node 0: ladder poses L_k = k (k = 0..40), pose L_k with exactly k distinct intra-node neighbours -- the fillers
    F_0..F_{k-1} (ids 41 + j), so filler F_j has 40 - j of them; L_0 has inter-node edges only.  A pose's block row of G
    has 1 + (distinct intra neighbours) blocks: lengths 1..41, each residue mod 8 and mod 16 at least twice.  Some edges
    are written reversed (head before tail) and some twice (parallel measurements of one pair).
    Nodes 1..5: LADDER_SIZES[1:] own poses (the 64-row segment boundaries), a chain plus random closures, again with
    reversed and parallel edges.  Neighbouring nodes share a few inter-node edges; L_0 and F_0 have some.
    Returns the dict of grid() plus num_nodes."""
    rng = np.random.default_rng(seed)
    nn = len(LADDER_SIZES)
    N = nn * LADDER_SPAN
    I, J = [], []

    def add(i, j):
        I.append(i); J.append(j)

    for k in range(1, LADDER_TOP + 1):
        for j in range(k):
            f = LADDER_TOP + 1 + j
            if (k + j) % 3 == 0:
                add(f, k)          # reversed
            else:
                add(k, f)
            if j == 0 and k % 4 == 0:
                add(k, f)          # parallel
    first = [a * LADDER_SPAN for a in range(nn)]
    for a in range(1, nn):
        n, b = LADDER_SIZES[a], first[a]
        for k in range(n - 1):
            add(b + k + 1, b + k) if k % 5 == 0 else add(b + k, b + k + 1)
        for _ in range(n // 2 if n > 2 else 0):
            u, v = rng.choice(n, 2, replace=False)
            add(b + u, b + v)
            if rng.random() < 0.2:
                add(b + v, b + u)  # parallel, reversed
    # inter-node edges: L_0 and F_0 of the ladder, the single pose of node 1, and a few per neighbouring pair
    add(0, first[1]); add(first[2], 0); add(LADDER_TOP + 1, first[5] + 3)
    add(first[1], first[2] + 5)
    for a in range(nn - 1):
        for _ in range(3):
            u = first[a] + rng.integers(LADDER_SIZES[a])
            v = first[a + 1] + rng.integers(LADDER_SIZES[a + 1])
            add(u, v) if rng.random() < 0.5 else add(v, u)
    I = np.asarray(I, np.int64)
    J = np.asarray(J, np.int64)
    M = len(I)
    R = _random_rotations_d(rng, M, d)
    t = rng.standard_normal((M, d))
    return dict(d=d, num_poses=N, num_nodes=nn, I=I, J=J, R=R, t=t, kappa=rng.uniform(1.0, 100.0, M),
                tau=rng.uniform(1.0, 100.0, M), outlier=np.zeros(M, bool))


INTER_LADDER_SIZES = (70, 1, 64, 65)       # own poses of the nodes of inter_ladder(); node 0 holds the ladder and the hub
INTER_LADDER_NBRS = (65, 1, 63, 64)        # ... and their neighbour rows (n1)
INTER_LADDER_SPAN = 130
INTER_LADDER_TOP = 40
INTER_LADDER_HUB = 41                      # the hub pose of node 0
INTER_LADDER_HUB_INCIDENCES = 300
INTER_LADDER_KINK = 48                     # edges whose noise is set so that s lands within 10 % of `kink` (half on each side)


def _small_rotations_d(rng, sigma, d):
    """exp of a rotation vector (d = 3) / angle (d = 2) with N(0, sigma_e^2) entries, one per entry of sigma."""
    if d == 3:
        return _exp_so3(sigma[:, None] * rng.standard_normal((len(sigma), 3)))
    th = sigma * rng.standard_normal(len(sigma))
    c, s = np.cos(th), np.sin(th)
    return np.stack([np.stack([c, -s], 1), np.stack([s, c], 1)], 1)


def inter_ladder(d=3, seed=11, kink=0.25):
    """A 4-node SE(d) graph whose INTER-node incidence lists cover what the inter-edge kernels split differently (for
    operator tests of the inter-edge pass, the objective and the Dynamic rescale).

    Node 0 (ids 0..69): own pose k <= 40 has exactly k inter-node incidences (0: the empty chain), even ones as the tail of
    an edge into node 2, odd ones as the head of an edge out of node 3 (written reversed: I > J); poses divisible by 4 carry
    one pair twice (parallel edges).  Pose 41 is the hub: 300 incidences, both roles, three of them with the single pose of
    node 1 (both directions and a parallel pair).  Poses 63, 64, 65 and 69 (the 64-row segment boundary and the last own row)
    have one incidence of each role.  Node 0 has well over 256 inter-node edges.
    Node 1: one pose, no intra-node edge, one neighbour row.  Node 2 (64 poses): every inter-node incidence is a head.
    Node 3 (65 poses): every one a tail.  Own sizes INTER_LADDER_SIZES, neighbour rows INTER_LADDER_NBRS.

    Measurements are formed from ground-truth poses (random rotations, translations uniform in [0, 10)^d): R_e = R_i^T R_j
    E_e, t_e = R_i^T (t_j - t_i) + n_e with E_e = exp(N(0, sigma_e^2)), n_e ~ N(0, sigma_e^2 I) and sigma_e log-uniform over
    1e-8 .. 1e1, so that every edge's residual at the ground truth is its own noise.  INTER_LADDER_KINK of the inter-node
    edges instead carry an exact rotation and a translation error of length sqrt(s / tau) with s / kink = 1 -+ [0.001, 0.1]:
    they sit on both sides of the Huber kink of loss_reg = kink.  tau, kappa uniform in [1, 100].
    Returns the dict of grid() plus num_nodes, Rg, tg (the ground truth) and sigma (the per-edge noise level; for the kink
    edges sqrt(s / tau))."""
    rng = np.random.default_rng(seed)
    nn, S = len(INTER_LADDER_SIZES), INTER_LADDER_SPAN
    N = nn * S
    b1, b2, b3 = S, 2 * S, 3 * S
    I, J = [], []

    def add(i, j):
        I.append(i); J.append(j)

    # intra-node chains (every own pose is used; node 1 has none), some reversed
    for a in (0, 2, 3):
        for k in range(INTER_LADDER_SIZES[a] - 1):
            add(a * S + k + 1, a * S + k) if k % 5 == 0 else add(a * S + k, a * S + k + 1)
    n_intra = len(I)

    def incidence(k, j, slot):
        if j % 2 == 0:
            add(k, b2 + slot % 32)        # tail role in node 0, head in node 2
        else:
            add(b3 + slot % 32, k)        # head role in node 0, tail in node 3 (reversed)

    for k in range(1, INTER_LADDER_TOP + 1):
        for j in range(k):
            incidence(k, j, 7 * k + (0 if (k % 4 == 0 and j == 2) else j))
    hub = INTER_LADDER_HUB
    add(b1, hub); add(hub, b1); add(b1, hub)
    for j in range(INTER_LADDER_HUB_INCIDENCES - 3):
        incidence(hub, j, 3 * j + j // 64)
    for k in (63, 64, 65, INTER_LADDER_SIZES[0] - 1):
        incidence(k, 0, k); incidence(k, 1, k)
    # node 3 -> node 2: 18 further poses of node 3 as neighbours of node 2, 20 of node 2 as neighbours of node 3
    for i in range(18):
        add(b3 + 32 + i, b2 + 32 + i)
    add(b3 + 32, b2 + 50); add(b3 + 32, b2 + 51); add(b3 + 33, b2 + 33)   # (the last one parallel)
    I = np.asarray(I, np.int64)
    J = np.asarray(J, np.int64)
    M = len(I)
    Rg = _random_rotations_d(rng, N, d)
    tg = rng.uniform(0.0, 10.0, (N, d))
    tau = rng.uniform(1.0, 100.0, M)
    kappa = rng.uniform(1.0, 100.0, M)
    sigma = 10.0 ** rng.uniform(-8.0, 1.0, M)
    Rt = np.einsum("eba,ebc->eac", Rg[I], Rg[J])
    tt = np.einsum("eba,eb->ea", Rg[I], tg[J] - tg[I])
    R = Rt @ _small_rotations_d(rng, sigma, d)
    t = tt + sigma[:, None] * rng.standard_normal((M, d))
    sel = n_intra + rng.choice(M - n_intra, INTER_LADDER_KINK, replace=False)
    off = rng.uniform(0.001, 0.1, INTER_LADDER_KINK) * np.where(np.arange(INTER_LADDER_KINK) % 2 == 0, 1.0, -1.0)
    dirs = rng.standard_normal((INTER_LADDER_KINK, d))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    sigma[sel] = np.sqrt(kink * (1.0 + off) / tau[sel])
    R[sel] = Rt[sel]
    t[sel] = tt[sel] + sigma[sel, None] * dirs
    return dict(d=d, num_poses=N, num_nodes=nn, I=I, J=J, R=R, t=t, kappa=kappa, tau=tau, outlier=np.zeros(M, bool),
                Rg=Rg, tg=tg, sigma=sigma)


def two_node(m, poses_per_node=256, seed=1, sigma_t=0.05, sigma_r=0.02, outlier_frac=0.1, extent=10.0):
    """A two-node SE(3) graph with m inter-node edges (the PCM test and benchmark instance).  Ground-truth poses:
    random rotations, translations uniform in [0, extent)^3; node 0 holds poses [0, P), node 1 [P, 2P) (the
    contiguous partition with num_nodes = 2).  Edges: an odometry chain inside each node, then m cross edges between
    random poses of the two nodes, every second one written from node 1 to node 0; their relative poses carry
    N(0, sigma_t^2) translation and exp(N(0, sigma_r^2)) rotation noise, and `outlier_frac` of them are random.
    Returns the dict of grid() plus Rg, tg (the ground truth)."""
    rng = np.random.default_rng(seed)
    P = poses_per_node
    N = 2 * P
    Rg = _random_rotations(rng, N)
    tg = rng.uniform(0, extent, (N, 3))
    chain = [(k, k + 1) for k in range(P - 1)] + [(P + k, P + k + 1) for k in range(P - 1)]
    a = rng.integers(0, P, m)
    b = rng.integers(P, N, m)
    flip = (np.arange(m) % 2) == 1
    I = np.concatenate([np.array([c[0] for c in chain]), np.where(flip, b, a)])
    J = np.concatenate([np.array([c[1] for c in chain]), np.where(flip, a, b)])
    M = len(I)
    R = np.einsum("eba,ebc->eac", Rg[I], Rg[J])                       # R_i^T R_j
    t = np.einsum("eba,eb->ea", Rg[I], tg[J] - tg[I])                 # R_i^T (t_j - t_i)
    R = R @ _exp_so3(sigma_r * rng.standard_normal((M, 3)))
    t = t + sigma_t * rng.standard_normal((M, 3))
    outlier = np.zeros(M, bool)
    n_out = int(round(outlier_frac * m))
    if n_out:
        sel = len(chain) + rng.choice(m, n_out, replace=False)
        outlier[sel] = True
        R[sel] = _random_rotations(rng, n_out)
        t[sel] = rng.uniform(-extent, extent, (n_out, 3))
    return dict(d=3, num_poses=N, I=I, J=J, R=R, t=t, kappa=np.full(M, 200.0), tau=np.full(M, 100.0),
                outlier=outlier, Rg=Rg, tg=tg)


def _planar(d, angle):
    """The rotation by `angle` about the first two axes of R^d."""
    R = np.eye(d)
    c, s = np.cos(angle), np.sin(angle)
    R[0, 0], R[0, 1], R[1, 0], R[1, 1] = c, -s, s, c
    return R


def twisted_ring(d=3, n=12, noise=0.02, seed=1, twist=1):
    """A single loop of n poses and a start that winds once too often around it (the staircase's test instance).

    Ground truth: pose k at angle 2 pi k / n on a circle of radius n / 2 pi in the plane of the first two axes, heading
    rotated by the same angle about them.  Edges k -> (k + 1) mod n with kappa = tau = 10.  Per edge, in edge order, from
    default_rng(seed): the rotation noise first -- d = 2: one normal times `noise` as an angle; d = 3: three normals times
    `noise` as a rotation vector -- applied on the right of the true relative rotation, then d normals times `noise` added
    to the true relative translation.  The start has the true translations and the rotations R_k Rot(twist 2 pi k / n):
    `twist` extra turns of the heading along the loop, a local minimum's basin away from the truth.
    Returns (the dict of grid() plus num_nodes = 1, the start in the library's global layout)."""
    rng = np.random.default_rng(seed)
    ang = 2 * np.pi * np.arange(n) / n
    Rg = np.stack([_planar(d, a) for a in ang])
    tg = np.zeros((n, d))
    tg[:, 0], tg[:, 1] = n / (2 * np.pi) * np.cos(ang), n / (2 * np.pi) * np.sin(ang)
    I = np.arange(n, dtype=np.int64)
    J = (I + 1) % n
    R, t = np.empty((n, d, d)), np.empty((n, d))
    for e in range(n):
        Rt = Rg[I[e]].T @ Rg[J[e]]
        tt = Rg[I[e]].T @ (tg[J[e]] - tg[I[e]])
        if d == 2:
            E = _planar(2, noise * rng.standard_normal())
        else:
            E = _exp_so3(noise * rng.standard_normal((1, 3)))[0]
        R[e] = Rt @ E
        t[e] = tt + noise * rng.standard_normal(d)
    g = dict(d=d, num_poses=n, num_nodes=1, I=I, J=J, R=R, t=t, kappa=np.full(n, 10.0), tau=np.full(n, 10.0),
             outlier=np.zeros(n, bool))
    Rs = np.stack([Rg[k] @ _planar(d, twist * ang[k]) for k in range(n)])
    return g, global_X(Rs, tg)


def global_X(R, t):
    """The library's global layout ((d+1)N x d) of poses R (N x d x d), t (N x d): rows [0, N) t_i, rows
    [N + d i, N + d i + d) R_i^T."""
    N, d = t.shape
    X = np.zeros(((d + 1) * N, d))
    X[:N] = t
    X[N:] = np.swapaxes(R, 1, 2).reshape(N * d, d)
    return X
