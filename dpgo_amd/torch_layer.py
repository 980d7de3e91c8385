"""A differentiable pose-graph solve for PyTorch: the solution of a pose graph as a function of its measurements.

    T, Rm = pose_graph_solve(I, J, R, t, kappa, tau, num_poses, d)

Forward: the graph of the edges (graph_from_edges), a trivial-loss group that hosts every node, the chordal point, and the
Newton polish on the device (NodeGroup.polish) to a critical point X* with pose `anchor` held fixed.  T (num_poses, d) are its
translations, Rm (num_poses, d, d) its rotations.  Backward: implicit differentiation on the device (NodeGroup.sensitivity) --
the incoming (gT, gRm) becomes the tangent gradient of the downstream scalar at X* (tangent_gradient), one adjoint solve on the
factor of the anchored Hessian gives dL/d(kappa_e, tau_e, t~_e, eta_e) of every edge, and those are handed back as gradients:

  * t, kappa, tau: as returned (raw entries).
  * R: the Riemannian gradient R~_e hat(s_e) / 2 with s_e = dL/d eta_e.  It is TANGENT to SO(d) at R~_e: the measured rotations
    are constrained, and only the derivative along R~ <- R~ Exp(hat(eta)) is defined.  <R~ hat(s) / 2, R~ hat(eta)>_F = s . eta,
    so a step R~ <- R~ Exp(-lr hat(s)) (or any retraction of -lr times the gradient) descends; the ambient components normal
    to SO(d) are zero by construction, not computed.

Everything is float64 on the host side of PyTorch; the arithmetic is the library's HIP kernels.  The edge indices I, J and the
sizes are not differentiable.

With loss = LOSS_HUBER, LOSS_GM or LOSS_WELSCH the solve is that of the ROBUST objective (the inter-node edges under the loss, so
num_nodes >= 2): forward is NodeGroup.robust_polish from the chordal point, backward one NodeGroup.robust_sensitivity call on the
true robust Hessian, and loss_reg -- a float64 scalar tensor, the loss threshold delta -- is differentiable too: its gradient
is dL/ddelta.  This is the derivative of the robust solution, not of its quadratic surrogate with frozen weights.
"""
import numpy as np
import torch

import dpgo_amd


def _hat(s, d):
    """(m, d, d) from (m, dof - d)."""
    H = np.zeros((len(s), d, d))
    if d == 2:
        H[:, 0, 1], H[:, 1, 0] = -s[:, 0], s[:, 0]
    else:
        H[:, 0, 1], H[:, 0, 2] = -s[:, 2], s[:, 1]
        H[:, 1, 0], H[:, 1, 2] = s[:, 2], -s[:, 0]
        H[:, 2, 0], H[:, 2, 1] = -s[:, 1], s[:, 0]
    return H


class _PoseGraphSolve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, R, t, kappa, tau, I, J, num_poses, d, num_nodes, anchor):
        for v in (R, t, kappa, tau):
            if v.dtype != torch.float64 or v.device.type != "cpu":
                raise TypeError("pose_graph_solve takes float64 host tensors")
        Rn = R.detach().numpy()
        graph = dpgo_amd.graph_from_edges(d, num_poses, np.asarray(I), np.asarray(J), Rn, t.detach().numpy(),
                                          kappa.detach().numpy(), tau.detach().numpy(), num_nodes)
        group = dpgo_amd.NodeGroup(graph, range(num_nodes), dpgo_amd.Options.driver(dpgo_amd.LOSS_NONE, True, max_iterations=0))
        X, res, _ = group.polish(graph.chordal_initialization(), anchor=anchor)
        if res.outcome != dpgo_amd.POLISH_CONVERGED:
            raise RuntimeError("pose_graph_solve: the Newton polish ended %s after %d steps (|g| = %.3g): no critical point to "
                               "differentiate at" % (dpgo_amd.POLISH_NAMES[res.outcome], res.steps, res.grad_final))
        X = np.array(X)
        ctx.group, ctx.X, ctx.R, ctx.d, ctx.anchor = group, X, np.array(Rn), d, anchor
        T = torch.from_numpy(np.array(X[:num_poses]))
        Rm = torch.from_numpy(np.ascontiguousarray(np.swapaxes(X[num_poses:].reshape(num_poses, d, d), 1, 2)))
        return T, Rm

    @staticmethod
    def backward(ctx, gT, gRm):
        d, X = ctx.d, ctx.X
        N = X.shape[0] // (d + 1)
        G = np.zeros_like(X)
        if gT is not None:
            G[:N] = gT.detach().numpy()
        if gRm is not None:     # X holds Y_p = R_p^T
            G[N:] = np.swapaxes(gRm.detach().numpy(), 1, 2).reshape(N * d, d)
        res, sens = ctx.group.sensitivity(X, dpgo_amd.tangent_gradient(X, G), anchor=ctx.anchor)
        if res.outcome != dpgo_amd.SENS_OK:
            raise RuntimeError("pose_graph_solve: the sensitivities ended %s" % dpgo_amd.SENS_NAMES[res.outcome])
        s = sens[0]
        gR = ctx.R @ _hat(s[:, 2 + d:], d) / 2
        return (torch.from_numpy(gR), torch.from_numpy(np.array(s[:, 2:2 + d])), torch.from_numpy(np.array(s[:, 0])),
                torch.from_numpy(np.array(s[:, 1])), None, None, None, None, None, None)


class _RobustPoseGraphSolve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, R, t, kappa, tau, loss_reg, I, J, num_poses, d, num_nodes, anchor, loss):
        for v in (R, t, kappa, tau, loss_reg):
            if v.dtype != torch.float64 or v.device.type != "cpu":
                raise TypeError("pose_graph_solve takes float64 host tensors")
        if loss_reg.numel() != 1:
            raise TypeError("pose_graph_solve: loss_reg is a scalar tensor")
        delta = float(loss_reg.detach().reshape(()))
        Rn = R.detach().numpy()
        graph = dpgo_amd.graph_from_edges(d, num_poses, np.asarray(I), np.asarray(J), Rn, t.detach().numpy(),
                                          kappa.detach().numpy(), tau.detach().numpy(), num_nodes)
        group = dpgo_amd.NodeGroup(graph, range(num_nodes), dpgo_amd.Options.driver(dpgo_amd.LOSS_NONE, True, max_iterations=0))
        X, res, _, _ = group.robust_polish(graph.chordal_initialization(), loss, delta, anchor=anchor)
        if res.outcome != dpgo_amd.POLISH_CONVERGED:
            raise RuntimeError("pose_graph_solve: the robust Newton polish ended %s after %d steps (|g| = %.3g): no critical point "
                               "to differentiate at" % (dpgo_amd.POLISH_NAMES[res.outcome], res.steps, res.grad_final))
        X = np.array(X)
        ctx.group, ctx.X, ctx.R, ctx.d, ctx.anchor, ctx.loss, ctx.delta = group, X, np.array(Rn), d, anchor, loss, delta
        ctx.reg_shape = loss_reg.shape
        T = torch.from_numpy(np.array(X[:num_poses]))
        Rm = torch.from_numpy(np.ascontiguousarray(np.swapaxes(X[num_poses:].reshape(num_poses, d, d), 1, 2)))
        return T, Rm

    @staticmethod
    def backward(ctx, gT, gRm):
        d, X = ctx.d, ctx.X
        N = X.shape[0] // (d + 1)
        G = np.zeros_like(X)
        if gT is not None:
            G[:N] = gT.detach().numpy()
        if gRm is not None:     # X holds Y_p = R_p^T
            G[N:] = np.swapaxes(gRm.detach().numpy(), 1, 2).reshape(N * d, d)
        res, sens, dreg = ctx.group.robust_sensitivity(X, dpgo_amd.tangent_gradient(X, G), ctx.loss, ctx.delta, anchor=ctx.anchor)
        if res.outcome != dpgo_amd.SENS_OK:
            raise RuntimeError("pose_graph_solve: the robust sensitivities ended %s" % dpgo_amd.SENS_NAMES[res.outcome])
        s = sens[0]
        gR = ctx.R @ _hat(s[:, 2 + d:2 + d + d * (d - 1) // 2], d) / 2
        return (torch.from_numpy(gR), torch.from_numpy(np.array(s[:, 2:2 + d])), torch.from_numpy(np.array(s[:, 0])),
                torch.from_numpy(np.array(s[:, 1])), torch.from_numpy(np.array(dreg[0])).reshape(ctx.reg_shape), None, None, None, None, None,
                None, None)


def pose_graph_solve(I, J, R, t, kappa, tau, num_poses, d, num_nodes=1, anchor=0, loss=dpgo_amd.LOSS_NONE, loss_reg=None):
    """(T (num_poses, d), Rm (num_poses, d, d)): the polished solution of the pose graph with edges (I[e], J[e]) and
    measurements R (m, d, d), t (m, d), kappa (m), tau (m) -- float64 host tensors, differentiable in all four (see the
    module's text for the gradient in R).  loss: LOSS_NONE, or a robust loss on the inter-node edges with loss_reg a float64
    scalar tensor (differentiable) and num_nodes >= 2.  Raises RuntimeError unless the polish converges."""
    if int(loss) == dpgo_amd.LOSS_NONE:
        return _PoseGraphSolve.apply(R, t, kappa, tau, I, J, int(num_poses), int(d), int(num_nodes), int(anchor))
    if int(loss) not in (dpgo_amd.LOSS_HUBER, dpgo_amd.LOSS_GM, dpgo_amd.LOSS_WELSCH):
        raise ValueError("pose_graph_solve: loss is LOSS_NONE, LOSS_HUBER, LOSS_GM or LOSS_WELSCH")
    if not torch.is_tensor(loss_reg):
        raise TypeError("pose_graph_solve: a robust loss takes loss_reg as a float64 scalar tensor")
    if int(num_nodes) < 2:
        raise ValueError("pose_graph_solve: a robust loss acts on the inter-node edges: num_nodes >= 2")
    return _RobustPoseGraphSolve.apply(R, t, kappa, tau, loss_reg, I, J, int(num_poses), int(d), int(num_nodes), int(anchor), int(loss))
