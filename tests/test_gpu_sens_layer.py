"""dpgo_amd.torch_layer.pose_graph_solve on the device: backward against NodeGroup.sensitivity contracted the same way, one
finite difference through the whole layer, and the refusal of a solve that did not converge.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import newton_restatement as nr  # noqa: E402
import test_gpu_certify as tc  # noqa: E402
import test_gpu_cert_proof as tp  # noqa: E402  (the ladder's edges; none of its tests is imported)

import dpgo_amd  # noqa: E402
from dpgo_amd.torch_layer import pose_graph_solve  # noqa: E402
from oracle.problem import LOSS_NONE  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def tiny(fixtures_dir):
    G = dpgo_amd.read_g2o(os.path.join(fixtures_dir, "tinyGrid3D.g2o"), 1)
    return G.num_poses, G.edges()


def tensors(edges, grad=True):
    I, J, R, t, kappa, tau = edges
    return I, J, [torch.tensor(v, dtype=torch.float64, requires_grad=grad) for v in (R, t, kappa, tau)]


def weights(N, d, seed=4):
    rng = np.random.default_rng(seed)
    return torch.tensor(rng.standard_normal((N, d))), torch.tensor(rng.standard_normal((N, d, d)))


@pytest.mark.parametrize("nn,anchor", [(1, 0), (2, 8)])
def test_backward_is_the_sensitivity_call_contracted_the_same_way(fixtures_dir, nn, anchor):
    N, edges = tiny(fixtures_dir)
    I, J, (R, t, kappa, tau) = tensors(edges)
    T, Rm = pose_graph_solve(I, J, R, t, kappa, tau, N, 3, num_nodes=nn, anchor=anchor)
    assert T.shape == (N, 3) and Rm.shape == (N, 3, 3) and T.dtype == torch.float64
    WT, WR = weights(N, 3)
    (torch.sum(WT * T) + torch.sum(WR * Rm)).backward()
    # the same by hand: the polished point, the ambient gradient in X's layout (Y_p = R_p^T), one column
    G = dpgo_amd.graph_from_edges(3, N, *edges, nn)
    grp = dpgo_amd.NodeGroup(G, range(nn), dpgo_amd.Options.driver(LOSS_NONE, True, max_iterations=0))
    X, pres, _ = grp.polish(G.chordal_initialization(), anchor=anchor)
    assert pres.outcome == dpgo_amd.POLISH_CONVERGED
    assert np.array_equal(T.detach().numpy(), X[:N]) and np.array_equal(Rm.detach().numpy(), np.swapaxes(X[N:].reshape(N, 3, 3), 1, 2))
    amb = np.zeros_like(X)
    amb[:N] = WT.numpy()
    amb[N:] = np.swapaxes(WR.numpy(), 1, 2).reshape(3 * N, 3)
    res, sens = grp.sensitivity(X, dpgo_amd.tangent_gradient(X, amb), anchor=anchor)
    assert res.outcome == dpgo_amd.SENS_OK
    s = sens[0]
    assert np.array_equal(kappa.grad.numpy(), s[:, 0]) and np.array_equal(tau.grad.numpy(), s[:, 1]) and np.array_equal(t.grad.numpy(), s[:, 2:5])
    gR, Rt = R.grad.numpy(), edges[2]
    # tangent to SO(3) at R~: R~^T gR = (R~^T R~) hat(s) / 2 is skew, and its pairing with the generators gives the eta entries
    # back -- as far as the measured R~ is a rotation: with E = R~^T R~ - I (1e-7 on a g2o file's quaternions) the symmetric part
    # is E K - K E and the pairing is off by <hat(e_k), E K>, K = hat(s) / 2: both within 2 d max|E| max|K| per edge
    A = np.swapaxes(Rt, 1, 2) @ gR
    E = np.abs(np.swapaxes(Rt, 1, 2) @ Rt - np.eye(3)).max(axis=(1, 2))
    tol = (6 * E + 16 * U) * np.abs(s[:, 5:]).max(axis=1)
    assert np.all(np.abs(A + np.swapaxes(A, 1, 2)).max(axis=(1, 2)) <= tol)
    back = np.stack([A[:, 2, 1] - A[:, 1, 2], A[:, 0, 2] - A[:, 2, 0], A[:, 1, 0] - A[:, 0, 1]], axis=1)
    assert np.all(np.abs(back - s[:, 5:]).max(axis=1) <= tol) and np.abs(s).min(axis=0).max() > 0


def test_one_finite_difference_through_the_layer(fixtures_dir):
    """kappa of one edge: L(kappa + h) - L(kappa - h) through two more solves, at two step sizes; |closed - D_{h/2}| is held
    to |D_h - D_{h/2}| plus the floor of the differences, computed below."""
    N, edges = tiny(fixtures_dir)
    I, J, (R, t, kappa, tau) = tensors(edges)
    WT, WR = weights(N, 3)
    loss = lambda T, Rm: torch.sum(WT * T) + torch.sum(WR * Rm)
    loss(*pose_graph_solve(I, J, R, t, kappa, tau, N, 3)).backward()
    e = 6
    closed = float(kappa.grad[e])

    def L(step):
        k = kappa.detach().clone()
        k[e] += step
        with torch.no_grad():
            return float(loss(*pose_graph_solve(I, J, R.detach(), t.detach(), k, tau.detach(), N, 3)))

    h = 2.0 ** -4 * float(kappa[e])
    D = [(L(s) - L(-s)) / (2 * s) for s in (h, h / 2)]
    # the floor: each of the four points is within (1e-9 hmax) / lambda_min(H) of a critical one (the polish's stopping rule
    # over the smallest eigenvalue of the restated anchored Hessian), L moves by at most |c| times that, a difference by twice
    # that over 2 h
    G = dpgo_amd.graph_from_edges(3, N, *edges, 1)
    grp = dpgo_amd.NodeGroup(G, [0], dpgo_amd.Options.driver(LOSS_NONE, True, max_iterations=0))
    X, pres, _ = grp.polish(G.chordal_initialization())
    M = tc.problem(fixtures_dir, "tinyGrid3D")[3].M
    lmin = float(np.linalg.eigvalsh(nr.anchored_hessian(M, X, 3, 0))[0])
    assert lmin > 0
    cnorm = float(np.sqrt(np.sum(WT.numpy() ** 2) + 2 * np.sum(WR.numpy() ** 2)))
    floor = cnorm * (1e-9 * pres.hmax / lmin) / (h / 2)
    print("d L / d kappa_%d: closed %.12g, differences %.12g, %.12g, floor %.3g" % (e, closed, D[0], D[1], floor))
    assert abs(closed - D[1]) <= abs(D[0] - D[1]) + floor
    assert abs(closed) > 10 * (abs(D[0] - D[1]) + floor)


def test_forward_raises_when_the_polish_does_not_converge():
    """The d = 2 ladder from its chordal point needs far more than the polish's 20 steps."""
    g, N, mm, gp, X0, nn = tp.ladder2()
    args = [torch.tensor(np.asarray(g[k], np.float64)) for k in ("R", "t", "kappa", "tau")]
    with pytest.raises(RuntimeError, match="polish"):
        pose_graph_solve(g["I"], g["J"], *args, N, 2, num_nodes=nn)
    with pytest.raises(TypeError):
        pose_graph_solve(g["I"], g["J"], args[0].float(), *args[1:], N, 2)
