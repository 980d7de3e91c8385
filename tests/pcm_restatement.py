"""numpy restatement of PCM::update (C++/DPGO/src/PCM.cpp:5-235) with the reference's variable names: the oracle the
PCM tests compare the device against (oracle/ is frozen, so it lives beside the tests).

X is the global iterate ((d+1)N x d): pose i has t_i = X[i] and R_i = X[N + d i : N + d i + d].T (PCM.cpp:128-129).
The q loop of one p is vectorised over q (same formulas, same order of the products)."""
import numpy as np


def measurement_list(alpha, beta, I, J, node_of):
    """PCM.cpp:22-33: the alpha-beta measurements in graph edge order (edge ids)."""
    ni, nj = node_of[I], node_of[J]
    return np.nonzero(((ni == alpha) & (nj == beta)) | ((ni == beta) & (nj == alpha)))[0]


def pose(X, N, d, i):
    t = X[i].copy()
    R = X[N + d * i:N + d * i + d].T.copy()
    return R, t


def roles(alpha, beta, I, J, R, t, node_of, measurements):
    """Per measurement: (alpha pose id, beta pose id, Rij, tij, Rji, tji) -- PCM.cpp:71-117 (first role, p) and
    :140-183 (second role, q); both forms computed from the measurement as the reference does."""
    out = []
    for e in measurements:
        if node_of[I[e]] == alpha and node_of[J[e]] == beta:
            i0, i1 = I[e], J[e]
            tij, Rij = t[e], R[e]                              # :91-92
            tji, Rji = -R[e].T @ t[e], R[e].T                  # :156-157
        else:
            i0, i1 = J[e], I[e]
            tij, Rij = -R[e].T @ t[e], R[e].T                  # :115-116
            tji, Rji = t[e], R[e]                              # :181-182
        out.append((i0, i1, Rij, tij, Rji, tji))
    return out


def pair_error(Ri, ti, Rj, tj, Rij, tij, Rji, tji, kappa=1.0, tau=1.0):
    """PCM.cpp:194-228 for one pair: Ri/ti/Rj/tj are two-element lists [p, q] of the alpha / beta poses."""
    d = len(tij)
    Rii = Ri[1].T @ Ri[0]
    tii = Ri[1].T @ (ti[0] - ti[1])
    Rjj = Rj[0].T @ Rj[1]
    tjj = Rj[0].T @ (tj[1] - tj[0])
    Raj = [Rij, Rij @ Rjj]
    taj = [tij, tij + Rij @ tjj]
    Rai = [None, Raj[1] @ Rji]
    tai = [None, taj[1] + Raj[1] @ tji]
    Rai[0] = Rai[1] @ Rii
    tai[0] = tai[1] + Rai[1] @ tii
    return np.sqrt(kappa * np.sum((Rai[0] - np.eye(d)) ** 2) + tau * np.sum(tai[0] ** 2))


def update(alpha, beta, I, J, R, t, kappa, tau, node_of, X, tolerance=0.2, weighted=False):
    """PCM::update: returns (measurements as edge ids, adjacency matrix (int), error matrix (diagonal 0))."""
    d = R.shape[1]
    N = len(node_of)
    measurements = measurement_list(alpha, beta, I, J, node_of)
    num_m = len(measurements)
    adjacency_matrix = np.zeros((num_m, num_m), int)
    E = np.zeros((num_m, num_m))
    if num_m == 0:
        return measurements, adjacency_matrix, E
    rl = roles(alpha, beta, I, J, R, t, node_of, measurements)
    Ra = np.stack([pose(X, N, d, r[0])[0] for r in rl])
    ta = np.stack([pose(X, N, d, r[0])[1] for r in rl])
    Rb = np.stack([pose(X, N, d, r[1])[0] for r in rl])
    tb = np.stack([pose(X, N, d, r[1])[1] for r in rl])
    RIJ = np.stack([r[2] for r in rl]); TIJ = np.stack([r[3] for r in rl])
    RJI = np.stack([r[4] for r in rl]); TJI = np.stack([r[5] for r in rl])
    kap, ta_ = kappa[measurements], tau[measurements]
    mv = lambda A, v: np.einsum("...ab,...b->...a", A, v)
    for p in range(num_m):
        adjacency_matrix[p, p] = 1
        q = np.arange(p + 1, num_m)
        if len(q) == 0:
            continue
        Ri0, ti0, Rj0, tj0, Rij, tij = Ra[p], ta[p], Rb[p], tb[p], RIJ[p], TIJ[p]
        Ri1, ti1, Rj1, tj1, Rji, tji = Ra[q], ta[q], Rb[q], tb[q], RJI[q], TJI[q]
        if weighted:
            k = 0.5 * (kap[p] + kap[q])
            tu = 0.5 * (ta_[p] + ta_[q])
        else:
            k = tu = 1.0
        Rii = np.swapaxes(Ri1, 1, 2) @ Ri0
        tii = mv(np.swapaxes(Ri1, 1, 2), ti0 - ti1)
        Rjj = Rj0.T @ Rj1
        tjj = mv(Rj0.T, tj1 - tj0)
        Raj1 = Rij @ Rjj
        taj1 = tij + mv(Rij, tjj)
        Rai1 = Raj1 @ Rji
        tai1 = taj1 + mv(Raj1, tji)
        Rai0 = Rai1 @ Rii
        tai0 = tai1 + mv(Rai1, tii)
        error = np.sqrt(k * np.sum((Rai0 - np.eye(d)) ** 2, axis=(1, 2)) + tu * np.sum(tai0 ** 2, axis=1))
        E[p, q] = E[q, p] = error
        adjacency_matrix[p, q] = adjacency_matrix[q, p] = error <= tolerance
    return measurements, adjacency_matrix, E
