"""The launches of an update enqueued ahead of the host's decision -- the gated local halo copy (k_copy_indexed), update()'s
product with G and its inter-edge pass under NodeMask{all, go} -- with the gate's word GIVEN (NodeGroup.debug_gated_update,
which enqueues Group::update_continuation, the very sequence speculate_update() enqueues):

  go = 0          every buffer the launches may write is bit for bit what it was: Xk, the X, g, Dfobj and G X of both history
                  places, every partial sum, DfobjE
  go = all ones   the result is bit for bit that of the same launches without a gate
  afterwards      the hook puts everything back: ten further step()s give the X of a run that never called it

The hook is called BETWEEN iterate() and update(), where speculate_update()'s launches run: the buffers are in the roles of the
accepted step, Xk's neighbour rows are still those of the previous iterate, and an open gate changes the destinations of all
three launches -- Xk (the halo copy), G X[iter-1] (the product), g[iter-1], Dfobj[iter-1], DfobjE and the partial sums (the
pass) -- so a closed gate that leaves them alone has held something back.  Behind update() the same launches would only repeat
what update() did (nothing but the partial sums would change); that state is checked for the closed gate as well.

Groups: synthetic.ladder(3) (its measured poses, in 6 nodes) and smallGrid3D in 2 nodes, Huber loss, Static rescale, after three step()s.
"""
import os

import numpy as np
import pytest

COPY, PRODUCT, PASS = ("Xk",), ("GXp",), ("gp", "Dfp", "DfE", "partials")   # the destinations with the accepted step's roles
BUFFERS = {"Xk", "Zc", "Zp", "gc", "gp", "Dfc", "Dfp", "GXc", "GXp", "partials", "DfE"}
ALL_ONES = 0xFFFFFFFFFFFFFFFF


def _driver(which, fixtures_dir):
    import dpgo_amd
    from dpgo_amd import synthetic
    if which == "ladder":
        g = synthetic.ladder(3)       # (its pose ids without an edge dropped: the chordal start needs every pose measured)
        used = np.unique(np.concatenate([g["I"], g["J"]]))
        new = np.full(g["num_poses"], -1, np.int64)
        new[used] = np.arange(len(used))
        G = dpgo_amd.graph_from_edges(g["d"], len(used), new[g["I"]], new[g["J"]], g["R"], g["t"], g["kappa"], g["tau"], g["num_nodes"])
    else:
        G = dpgo_amd.read_g2o(os.path.join(fixtures_dir, "smallGrid3D.g2o"), 2)
    return dpgo_amd.DistPGO(G, dpgo_amd.Options.driver(dpgo_amd.LOSS_HUBER, True), X0=G.chordal_initialization())


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["ladder", "smallGrid3D"])
def test_gated_launches_fall_through_or_run(which, fixtures_dir):
    plain, hooked = _driver(which, fixtures_dir), _driver(which, fixtures_dir)
    for drv in (plain, hooked):
        for _ in range(3):
            assert drv.step() == 0
    # behind update(): a closed gate
    closed = hooked.group.debug_gated_update(0)
    assert set(closed) == BUFFERS
    assert all(r["untouched"] and r["same_as_ungated"] is None for r in closed.values()), closed
    # between iterate() and update()
    assert plain.group.iterate() == 0 and hooked.group.iterate() == 0
    closed = hooked.group.debug_gated_update(0)
    assert set(closed) == BUFFERS and all(r["untouched"] for r in closed.values()), closed
    opened = hooked.group.debug_gated_update(ALL_ONES)
    assert all(r["same_as_ungated"] for r in opened.values()), opened
    assert not any(opened[k]["untouched"] for k in COPY + PRODUCT + PASS), opened
    assert all(opened[k]["untouched"] for k in ("gc", "Dfc", "GXc", "Zc")), opened      # (X[iter]'s side: no role in these launches)
    again = hooked.group.debug_gated_update(0)     # every launch reads the word anew
    assert all(r["untouched"] for r in again.values()), again
    for drv in (plain, hooked):
        assert drv.group.communicate_local() == 0 and drv.group.update() == 0
    for _ in range(10):
        assert plain.step() == 0 and hooked.step() == 0
    assert np.array_equal(plain.X(), hooked.X())
