"""The boundary exchange between two groups of one process, wired as connect_torch does (pack_sent into one device buffer,
set_recv_layout, unpack_recv) without torch.distributed, with Huber so that the unpack is lazy (Group::set_pending_recv:
the next update()'s inter-edge pass reads the neighbour rows out of the receive buffer through a digest of the lists).

torus3D, 8 nodes: group A = nodes 0-3, group B = nodes 4-7, against one group holding all 8."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import dpgo_amd
from oracle.problem import LOSS_HUBER

pytestmark = pytest.mark.gpu

ITERS = 10
HALF = 5
NN = 8


class DevArray:
    """n doubles of device memory (the HIP runtime the library itself is linked against)."""
    _hip = None

    def __init__(self, n, fill=0.0):
        if DevArray._hip is None:
            dpgo_amd.lib()
            DevArray._hip = ctypes.CDLL("libamdhip64.so.7")   # (already loaded with the library: the same runtime)
        self.n = n
        self.ptr = ctypes.c_void_p()
        assert self._hip.hipMalloc(ctypes.byref(self.ptr), ctypes.c_size_t(8 * max(n, 1))) == 0
        self.upload(np.full(n, fill))

    def upload(self, a, off=0):
        a = np.ascontiguousarray(a, np.float64)
        assert self._hip.hipMemcpy(ctypes.c_void_p(self.ptr.value + 8 * off), a.ctypes.data_as(ctypes.c_void_p),
                                   ctypes.c_size_t(8 * a.size), 1) == 0   # hipMemcpyHostToDevice

    def copy_from(self, src, n, off=0):
        assert self._hip.hipMemcpy(ctypes.c_void_p(self.ptr.value + 8 * off), src.ptr, ctypes.c_size_t(8 * n), 3) == 0   # DeviceToDevice

    def __del__(self):
        if self.ptr.value:
            self._hip.hipDeviceSynchronize()
            self._hip.hipFree(self.ptr)
            self.ptr = ctypes.c_void_p()


def _graph(fixtures_dir):
    G = dpgo_amd.read_g2o(os.path.join(fixtures_dir, "torus3D.g2o"), NN)
    return G, G.chordal_initialization()


def _gather(groups, X):
    for g in groups:
        assert g.scatter_global(X) == 0
    return X.copy()


def run_single(G, X0):
    opt = dpgo_amd.Options.driver(LOSS_HUBER, True)
    grp = dpgo_amd.NodeGroup(G, range(NN), opt)
    X = np.zeros(X0.shape, order="F")
    assert grp.initialize_global(X0) == 0 and grp.update() == 0
    out = []
    for _ in range(ITERS):
        assert grp.iterate() == 0 and grp.communicate_local() == 0 and grp.update() == 0
        out.append(_gather([grp], X))
    return np.array(out)


class Split:
    """Groups A and B and the exchange between them: the send buffers, and a gathered buffer laid out as set_recv_layout
    was told (slot of key k of rank position r = r * stride + k)."""

    def __init__(self, G, X0):
        opt = dpgo_amd.Options.driver(LOSS_HUBER, True)
        self.groups = [dpgo_amd.NodeGroup(G, range(0, 4), opt), dpgo_amd.NodeGroup(G, range(4, 8), opt)]
        self.keys = [g.sent_keys() for g in self.groups]
        self.RS = (G.d + 1) * G.d
        self.nsent = [len(k[0]) for k in self.keys]
        assert min(self.nsent) > 0
        self.sends = [DevArray(n * self.RS) for n in self.nsent]
        self.X = np.zeros(X0.shape, order="F")
        self.layout(0, False)
        for g in self.groups:
            assert g.initialize_global(X0) == 0
        for g in self.groups:
            assert g.update() == 0

    def layout(self, extra, reverse):
        """set_recv_layout of both groups with stride max(sent) + extra, the ranks listed in reverse order if asked, and a
        fresh gathered buffer for it."""
        self.stride = max(self.nsent) + extra
        self.order = [1, 0] if reverse else [0, 1]
        for g in self.groups:
            assert g.set_recv_layout(self.stride, [self.keys[r] for r in self.order]) == 0
        self.gathered = DevArray(2 * self.stride * self.RS, np.nan)   # (slots nobody fills stay NaN)

    def pack_unpack(self):
        for g, s in zip(self.groups, self.sends):
            assert g.communicate_local() == 0 and g.pack_sent(s.ptr.value) == 0
        for g in self.groups:
            assert g.sync() == 0
        for pos, r in enumerate(self.order):   # the all-gather: rank r's records at slot pos * stride
            self.gathered.copy_from(self.sends[r], self.nsent[r] * self.RS, pos * self.stride * self.RS)
        for g in self.groups:
            assert g.unpack_recv(self.gathered.ptr.value) == 0

    def iterate(self):
        for g in self.groups:
            assert g.iterate() == 0

    def update(self):
        for g in self.groups:
            assert g.update() == 0
        return _gather(self.groups, self.X)

    def step(self):
        self.iterate()
        self.pack_unpack()
        return self.update()


def run_split(G, X0, relayout=None):
    """ITERS iterations; relayout: None, "before" (set_recv_layout again before the exchange of iteration HALF), "after"
    (after its unpack, no update between) or "after_sync" (the same with a sync() between the two calls)."""
    s = Split(G, X0)
    out = []
    for it in range(ITERS):
        if it == HALF and relayout == "before":
            s.layout(5, True)
        if it == HALF and relayout in ("after", "after_sync"):
            s.iterate()
            s.pack_unpack()
            if relayout == "after_sync":
                for g in s.groups:
                    assert g.sync() == 0
            keep = s.gathered              # (the pending unpack reads it: it must outlive the update)
            s.layout(5, True)
            out.append(s.update())
            del keep
            continue
        out.append(s.step())
    return np.array(out)


@pytest.fixture(scope="module")
def runs(fixtures_dir):
    G, X0 = _graph(fixtures_dir)
    return G, X0, run_single(G, X0), run_split(G, X0)


def test_split_groups_follow_the_single_group(runs):
    """(a) the exchange through set_recv_layout / unpack_recv is exact: the trajectory of the single group."""
    _, _, one, two = runs
    for it in range(ITERS):
        err = np.abs(two[it] - one[it]).max()
        assert err <= 1e-10 * np.abs(one[it]).max(), (it, err)


def test_second_recv_layout_midway_changes_nothing(runs):
    """(b) set_recv_layout again halfway (stride + 5, the ranks in reverse order, a fresh buffer): the same bits.  The lists
    are re-uploaded at the size they had, so very likely at the address they had: the lazy unpack's digest must not be
    taken for the old one's."""
    G, X0, _, two = runs
    b = run_split(G, X0, "before")
    for it in range(ITERS):
        assert np.array_equal(b[it], two[it]), it


def test_initialize_after_an_unconsumed_unpack(runs):
    """(c) unpack_recv, then initialize_global(X0), then update(): as if the unpack had never been (initialize() syncs, and
    sync() flushes the pending unpack before the rows are overwritten)."""
    G, X0, _, _ = runs
    s = Split(G, X0)
    s.pack_unpack()
    for g in s.groups:
        assert g.initialize_global(X0) == 0
    out = [s.update()]
    for _ in range(2):
        out.append(s.step())
    ref = Split(G, X0)
    for g in ref.groups:
        assert g.initialize_global(X0) == 0
    out_ref = [ref.update()] + [ref.step() for _ in range(2)]
    for it in range(3):
        assert np.array_equal(out[it], out_ref[it]), it


def test_recv_layout_between_unpack_and_update(runs):
    """(d) unpack_recv, then set_recv_layout(new) with no update between: the unpack lands as the old lay-out described it --
    the bits of the same sequence with a sync() (which flushes it) between the two calls, and of the run without either."""
    G, X0, _, two = runs
    d = run_split(G, X0, "after")
    ds = run_split(G, X0, "after_sync")
    for it in range(ITERS):
        assert np.array_equal(d[it], ds[it]), it
        assert np.array_equal(d[it], two[it]), it


def test_second_recv_layout_without_the_lazy_unpack(runs, tmp_path):
    """(e) (b) with DPGO_LAZY_UNPACK=0 (read once per process: a child) -- the plain unpack kernel -- gives the same bits."""
    _, _, _, two = runs
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    out = tmp_path / "b.npy"
    code = ("import sys; sys.path[:0] = [%r, %r]; import numpy as np; import test_gpu_recv_layout as t; from conftest import FIXTURES; "
            "G, X0 = t._graph(FIXTURES); np.save(%r, t.run_split(G, X0, 'before'))" % (root, here, str(out)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, cwd=root,
                       env=dict(os.environ, DPGO_LAZY_UNPACK="0"))
    assert r.returncode == 0, r.stderr[-3000:]
    e = np.load(str(out))
    for it in range(ITERS):
        assert np.array_equal(e[it], two[it]), it
