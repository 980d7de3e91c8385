"""The oracle's single operators (oracle/problem.py), pinned on the CPU before the GPU operator tests
(test_gpu_operators.py) lean on them, and the graph generators those tests run on."""
import numpy as np
import pytest
import scipy.sparse as sp

from dpgo_amd import synthetic
from oracle import g2o as og
from oracle.problem import DPGOProblem, LOSS_HUBER, LOSS_NONE, project_to_SOdn, tangent_proj

U = 2.0 ** -53


def measurements(g):
    """The oracle's global measurement list of a synthetic graph (read_g2o_file's layout)."""
    z = np.zeros(len(g["I"]), np.int64)
    return og.Measurements(z, g["I"], z, g["J"], g["R"], g["t"], g["kappa"], g["tau"])


def node_problems(g, num_nodes, loss, **kw):
    _, meas, _ = og.partition_measurements(g["num_poses"], measurements(g), num_nodes)
    return [DPGOProblem(a, meas[a], 1e-11, loss, 1e6, 0.25, **kw) for a in range(num_nodes)]


def random_point(rng, p, tscale=3.0):
    n0, d = p.n[0], p.d
    R = project_to_SOdn(rng.standard_normal((d * n0, d)), d)
    return np.vstack([tscale * rng.standard_normal((n0, d)), R])


def block_row_lengths(G, n0, d):
    """Blocks of (d+1) x (d+1) per pose row of a node's G (reference layout: rows [0, n0) translations, then d per pose)."""
    pose = np.concatenate([np.arange(n0), np.repeat(np.arange(n0), d)])
    C = sp.coo_matrix(G)
    pairs = np.unique(pose[C.row] * n0 + pose[C.col])
    return np.bincount(pairs // n0, minlength=n0)


@pytest.mark.parametrize("loss", [LOSS_NONE, LOSS_HUBER])
@pytest.mark.parametrize("d", [2, 3])
def test_hessian_vector_product_is_the_derivative_of_the_gradient(loss, d):
    """Hess[Rdot] = Proj_R(d/dh grad(R(h))) along R(h) = proj(R + h Rdot), grad the Riemannian gradient of the reduced
    cost (translations recovered at every point): the central difference converges to it as h^2."""
    g = synthetic.ladder(d)
    rng = np.random.default_rng(11)
    for p in node_problems(g, g["num_nodes"], loss)[:3]:
        n0 = p.n[0]
        Y = random_point(rng, p)
        gv = rng.standard_normal(Y.shape)
        R = Y[n0:]
        Rdot = tangent_proj(R, rng.standard_normal(R.shape), d)

        def grad(h):
            Rh = project_to_SOdn(R + h * Rdot, d)
            Yh = np.vstack([p.recover_translations(Rh, gv), Rh])
            return tangent_proj(Rh, p.reduced_Euclidean_gradient_G(Yh, gv), d)

        Y[:n0] = p.recover_translations(R, gv)
        H = p.hessian_vector_product(Y, p.reduced_Euclidean_gradient_G(Y, gv), Rdot)
        scale = np.linalg.norm(H)
        assert scale > 0
        errs = []
        for h in (1e-3, 5e-4):
            fd = tangent_proj(R, (grad(h) - grad(-h)) / (2 * h), d)
            errs.append(np.linalg.norm(fd - H) / scale)
        # O(h^2): halving h divides the error by 4 (3 leaves room for the O(h^4) term and rounding, ~u / h = 2e-13)
        assert errs[1] <= errs[0] / 3, errs
        assert errs[0] < 1e-4, errs


def test_regularized_cholesky_preconditioner_against_a_dense_solve():
    g = synthetic.ladder(3)
    rng = np.random.default_rng(12)
    for p in node_problems(g, g["num_nodes"], LOSS_HUBER, preconditioner=True)[:3]:
        n0, d = p.n[0], p.d
        Y = random_point(rng, p)
        v = rng.standard_normal((d * n0, d))
        A = p.mat.GRR.toarray() + (p.lambda_max / 1e6) * np.eye(d * n0)
        x = np.linalg.solve(A, v)
        ref = tangent_proj(Y[n0:], x, d)
        out = p.precondition(Y, v)
        # both solves are backward stable: forward error <= 2 * 10 kappa_2 u |x| (the projection is a contraction)
        tol = 20 * np.linalg.cond(A) * U * np.linalg.norm(x)
        assert np.linalg.norm(out - ref) <= tol
        # lambda_max: the reference's Spectra tolerance (1e-4) against the dense spectrum
        lam = np.linalg.eigvalsh(p.mat.GRR.toarray())[-1]
        assert abs(p.lambda_max - lam) <= 1e-4 * lam


def test_jacobi_preconditioner_against_the_diagonal():
    g = synthetic.ladder(2)
    rng = np.random.default_rng(13)
    p = node_problems(g, g["num_nodes"], LOSS_NONE, preconditioner=1)[0]
    n0, d = p.n[0], p.d
    Y = random_point(rng, p)
    v = rng.standard_normal((d * n0, d))
    ref = tangent_proj(Y[n0:], v / p.mat.GRR.diagonal()[:, None], d)
    np.testing.assert_allclose(p.precondition(Y, v), ref, rtol=0, atol=1e-14 * np.abs(ref).max())


@pytest.mark.parametrize("d", [2, 3])
def test_ladder_generator_gives_the_rows_it_claims(d):
    g = synthetic.ladder(d)
    nn = g["num_nodes"]
    I, J = g["I"], g["J"]
    pairs = list(zip(I.tolist(), J.tolist()))
    assert len(pairs) > len(set(pairs)), "parallel edges"
    assert any(i > j for i, j in pairs) and any(i < j for i, j in pairs), "edges in both directions"
    _, meas, _ = og.partition_measurements(g["num_poses"], measurements(g), nn)
    top = synthetic.LADDER_TOP
    for a in range(nn):
        info = og.generate_data_info(a, meas[a])
        assert info.n[0] == synthetic.LADDER_SIZES[a]
        assert info.m[1] > 0
    # node 0: pose k (k <= 40) has k distinct intra-node neighbours, L_0 only inter-node edges
    p = node_problems(g, nn, LOSS_NONE)[0]
    lengths = block_row_lengths(p.mat.G, p.n[0], d)
    np.testing.assert_array_equal(lengths[:top + 1], 1 + np.arange(top + 1))
    assert sorted(lengths[top + 1:].tolist()) == list(range(2, top + 2))
    for period in (8, 16):                    # k_bsr's groups of 2 over 4 lanes, k_bsr_tcol's groups of 4
        counts = np.bincount(lengths % period, minlength=period)
        assert counts.min() >= 2, (period, counts)
    intra0 = (meas[0].inode == 0) & (meas[0].jnode == 0)
    assert not np.any(intra0 & ((meas[0].ipose == 0) | (meas[0].jpose == 0)))
    for q in node_problems(g, nn, LOSS_HUBER):
        np.linalg.cholesky(q.mat.Gtt.toarray())   # G_tt positive definite: every node is anchored


def test_lattice_generators_give_the_node_sizes_they_claim():
    for (nx, ny, nz, m), nn, rows in (((50, 50, 40, 400_000), 8, 12_500), ((32, 32, 24, 98_304), 6, 4096)):
        g = synthetic.grid(nx, ny, nz, m, seed=synthetic.HEADLINE["seed"])
        assert g["num_poses"] == nx * ny * nz and len(g["I"]) == m
        node, _ = og.partition_index(g["num_poses"], nn)
        np.testing.assert_array_equal(np.bincount(node), np.full(nn, rows))
        deg = np.bincount(np.concatenate([g["I"], g["J"]]), minlength=g["num_poses"])
        assert deg.min() >= 3
