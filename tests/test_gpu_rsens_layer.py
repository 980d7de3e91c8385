"""dpgo_amd.torch_layer.pose_graph_solve with a robust loss on the device: backward against NodeGroup.robust_sensitivity
contracted the same way, one finite difference through the whole layer in kappa of an inter-node edge and one in the loss
threshold delta, and the refusals.  tinyGrid3D on 2 nodes (4 inter-node edges) from its chordal point; Huber at delta = 5 has
edges on either side of the kink there, Welsch at delta = 50 is smooth (both chosen on the CPU: robust_restatement.polish_full
converges within the polish's 20 steps and the restated H is positive definite).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import robust_inputs as ri  # noqa: E402
import robust_restatement as rr  # noqa: E402
import test_gpu_cert_proof as tp  # noqa: E402  (the ladder's edges; none of its tests is imported)

import dpgo_amd  # noqa: E402
from dpgo_amd.torch_layer import pose_graph_solve  # noqa: E402
from oracle.problem import LOSS_HUBER, LOSS_NONE, LOSS_WELSCH  # noqa: E402

pytestmark = pytest.mark.gpu

N, D, NN = 9, 3, 2


def tiny():
    P, _ = ri.named("tiny")
    assert P["N"] == N and P["num_nodes"] == NN
    return P, (P["I"], P["J"], P["R"], P["t"], P["kappa"], P["tau"])


def tensors(edges, delta):
    I, J, R, t, kappa, tau = edges
    return I, J, [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (R, t, kappa, tau)], \
        torch.tensor(delta, dtype=torch.float64, requires_grad=True)


def weights(seed=4):
    rng = np.random.default_rng(seed)
    return torch.tensor(rng.standard_normal((N, D))), torch.tensor(rng.standard_normal((N, D, D)))


def to_X(T, Rm):
    return np.concatenate([T.detach().numpy(), np.swapaxes(Rm.detach().numpy(), 1, 2).reshape(D * N, D)])


@pytest.mark.parametrize("loss,delta,anchor", [(LOSS_HUBER, 5.0, 0), (LOSS_WELSCH, 50.0, 8)])
def test_backward_is_the_robust_sensitivity_call_contracted_the_same_way(loss, delta, anchor):
    P, edges = tiny()
    I, J, (R, t, kappa, tau), reg = tensors(edges, delta)
    T, Rm = pose_graph_solve(I, J, R, t, kappa, tau, N, D, num_nodes=NN, anchor=anchor, loss=loss, loss_reg=reg)
    assert T.shape == (N, D) and Rm.shape == (N, D, D) and T.dtype == torch.float64
    WT, WR = weights()
    (torch.sum(WT * T) + torch.sum(WR * Rm)).backward()
    # the same by hand: the robust-polished point, the ambient gradient in X's layout (Y_p = R_p^T), one column
    G = dpgo_amd.graph_from_edges(D, N, *edges, NN)
    grp = dpgo_amd.NodeGroup(G, range(NN), dpgo_amd.Options.driver(LOSS_NONE, True, max_iterations=0))
    X, pres, _, _ = grp.robust_polish(G.chordal_initialization(), loss, delta, anchor=anchor)
    assert pres.outcome == dpgo_amd.POLISH_CONVERGED and np.array_equal(to_X(T, Rm), X)
    amb = np.zeros_like(X)
    amb[:N] = WT.numpy()
    amb[N:] = np.swapaxes(WR.numpy(), 1, 2).reshape(D * N, D)
    res, sens, dreg = grp.robust_sensitivity(X, dpgo_amd.tangent_gradient(X, amb), loss, delta, anchor=anchor)
    assert res.outcome == dpgo_amd.SENS_OK
    s = sens[0]
    assert np.array_equal(kappa.grad.numpy(), s[:, 0]) and np.array_equal(tau.grad.numpy(), s[:, 1]) and np.array_equal(t.grad.numpy(), s[:, 2:5])
    assert reg.grad.shape == reg.shape and float(reg.grad) == dreg[0] and dreg[0] != 0.0
    H = np.zeros((len(s), 3, 3))
    H[:, 0, 1], H[:, 0, 2], H[:, 1, 0], H[:, 1, 2], H[:, 2, 0], H[:, 2, 1] = -s[:, 7], s[:, 6], s[:, 7], -s[:, 5], -s[:, 6], s[:, 5]
    assert np.array_equal(R.grad.numpy(), edges[2] @ H / 2) and np.abs(s[:, :8]).min(axis=0).max() > 0


def restated(P, X, loss, delta):
    """(lambda_min of the restated anchored robust H at X, hmax the polish's scale: the largest diagonal entry)."""
    A = rr.hessian(P, X, loss, delta, 1, 0)
    return float(np.linalg.eigvalsh(A)[0]), float(np.abs(np.diag(A)).max())


def test_one_finite_difference_through_the_layer_in_kappa_of_an_inter_edge():
    """Welsch, delta = 50, the inter-node edge with the largest residual: L(kappa + h) - L(kappa - h) through two more solves,
    at two step sizes; |closed - D_{h/2}| is held to |D_h - D_{h/2}| plus the floor of the differences: each of the four
    points is within (1e-9 hmax) / lambda_min(H) of a critical one (the polish's stopping rule over the smallest eigenvalue of
    the restated anchored robust Hessian), L moves by at most |c| times that, a difference by twice that over 2 h."""
    loss, delta = LOSS_WELSCH, 50.0
    P, edges = tiny()
    I, J, (R, t, kappa, tau), reg = tensors(edges, delta)
    WT, WR = weights()
    Lf = lambda T, Rm: torch.sum(WT * T) + torch.sum(WR * Rm)
    T, Rm = pose_graph_solve(I, J, R, t, kappa, tau, N, D, num_nodes=NN, loss=loss, loss_reg=reg)
    Lf(T, Rm).backward()
    X = to_X(T, Rm)
    s = np.asarray(rr.weights(P, X, loss, delta)[0])
    e = int(np.argmax(np.where(P["inter"], s, -np.inf)))
    closed = float(kappa.grad[e])

    def L(step):
        k = kappa.detach().clone()
        k[e] += step
        with torch.no_grad():
            return float(Lf(*pose_graph_solve(I, J, R.detach(), t.detach(), k, tau.detach(), N, D, num_nodes=NN, loss=loss, loss_reg=reg.detach())))

    h = 2.0 ** -4 * float(kappa[e].detach())
    Dd = [(L(st) - L(-st)) / (2 * st) for st in (h, h / 2)]
    lmin, hmax = restated(P, X, loss, delta)
    assert lmin > 0
    cnorm = float(np.sqrt(np.sum(WT.numpy() ** 2) + 2 * np.sum(WR.numpy() ** 2)))
    floor = cnorm * (1e-9 * hmax / lmin) / (h / 2)
    print("d L / d kappa_%d (inter, s = %.3g): closed %.12g, differences %.12g, %.12g, floor %.3g" % (e, s[e], closed, Dd[0], Dd[1], floor))
    assert abs(closed - Dd[1]) <= abs(Dd[0] - Dd[1]) + floor
    assert abs(closed) > 10 * (abs(Dd[0] - Dd[1]) + floor)


def test_one_finite_difference_through_the_layer_in_delta():
    """Huber, delta = 5: the same rule in the loss threshold, h = 2^-6 delta; no inter edge changes its side of the kink
    between the four points."""
    loss, delta = LOSS_HUBER, 5.0
    P, edges = tiny()
    I, J, (R, t, kappa, tau), reg = tensors(edges, delta)
    WT, WR = weights()
    Lf = lambda T, Rm: torch.sum(WT * T) + torch.sum(WR * Rm)
    T, Rm = pose_graph_solve(I, J, R, t, kappa, tau, N, D, num_nodes=NN, loss=loss, loss_reg=reg)
    Lf(T, Rm).backward()
    X = to_X(T, Rm)
    closed = float(reg.grad)
    side = np.asarray(rr.weights(P, X, loss, delta)[0])[P["inter"]] > delta
    assert side.any() and not side.all()

    def L(step):
        with torch.no_grad():
            dl = torch.tensor(delta + step, dtype=torch.float64)
            out = pose_graph_solve(I, J, R.detach(), t.detach(), kappa.detach(), tau.detach(), N, D, num_nodes=NN, loss=loss, loss_reg=dl)
        assert np.array_equal(np.asarray(rr.weights(P, to_X(*out), loss, delta + step)[0])[P["inter"]] > delta + step, side)
        return float(Lf(*out))

    h = 2.0 ** -6 * delta
    Dd = [(L(st) - L(-st)) / (2 * st) for st in (h, h / 2)]
    lmin, hmax = restated(P, X, loss, delta)
    assert lmin > 0
    cnorm = float(np.sqrt(np.sum(WT.numpy() ** 2) + 2 * np.sum(WR.numpy() ** 2)))
    floor = cnorm * (1e-9 * hmax / lmin) / (h / 2)
    print("d L / d delta: closed %.12g, differences %.12g, %.12g, floor %.3g" % (closed, Dd[0], Dd[1], floor))
    assert abs(closed - Dd[1]) <= abs(Dd[0] - Dd[1]) + floor
    assert abs(closed) > 10 * (abs(Dd[0] - Dd[1]) + floor)


def test_refusals():
    P, edges = tiny()
    args = [torch.tensor(np.asarray(v, np.float64)) for v in edges[2:]]
    reg = torch.tensor(5.0, dtype=torch.float64)
    with pytest.raises(ValueError):
        pose_graph_solve(edges[0], edges[1], *args, N, D, num_nodes=1, loss=LOSS_HUBER, loss_reg=reg)       # no inter-node edge
    with pytest.raises(TypeError):
        pose_graph_solve(edges[0], edges[1], *args, N, D, num_nodes=NN, loss=LOSS_HUBER, loss_reg=5.0)      # not a tensor
    with pytest.raises(TypeError):
        pose_graph_solve(edges[0], edges[1], *args, N, D, num_nodes=NN, loss=LOSS_HUBER, loss_reg=reg.float())
    with pytest.raises(ValueError):
        pose_graph_solve(edges[0], edges[1], *args, N, D, num_nodes=NN, loss=7, loss_reg=reg)
    g, Nl, _, _, _, nn = tp.ladder2()             # the d = 2 ladder from its chordal point needs far more than the polish's 20 steps
    largs = [torch.tensor(np.asarray(g[k], np.float64)) for k in ("R", "t", "kappa", "tau")]
    with pytest.raises(RuntimeError, match="polish"):
        pose_graph_solve(g["I"], g["J"], *largs, Nl, 2, num_nodes=nn, loss=LOSS_HUBER, loss_reg=reg)
    # the trivial loss is the layer of before, loss_reg ignored
    T0, R0 = pose_graph_solve(edges[0], edges[1], *args, N, D, num_nodes=NN)
    T1, R1 = pose_graph_solve(edges[0], edges[1], *args, N, D, num_nodes=NN, loss=LOSS_NONE, loss_reg=None)
    assert torch.equal(T0, T1) and torch.equal(R0, R1)
