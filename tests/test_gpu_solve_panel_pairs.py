"""The paired panel layout of the device multifrontal solve (dpgo_amd/csrc/spd_panel.h; kernels.hip: stream_load,
k_pack_panels; spd_solve.cpp: upload, repack) against the plain one: DPGO_SPD_PANEL_PAIRS=1 and =0 give the same bits.

A lane consumes the same entries in the same order under both layouts -- only where they lie in memory and how many a load
fetches differ -- so every solution is equal bit for bit, and the plan (tile classes, counts, launches) is untouched.

As tests/test_gpu_solve_tiles.py: the library reads its settings once per process, so every (plan, setting) is one child
process (tests/solve_tiles_child.py) that runs all inputs of solve_restatement.INPUTS for d = 3, 2 and dof = 1, d; the
parent compares.  A child is started once and never retried; one that ends by a signal, by its timeout or with an error
fails the module's remaining tests without another child being started.

  default      16-row levels (4 lanes per row, paired), 8-row fused roots (plain under both settings), NT = false
  rows64       64-row tiles everywhere (1 lane per row), 64-row roots
  root16       16-row roots
  stream_once  the non-temporal instantiations
  host_panels  the host packer instead of k_pack_panels
  dynamic      repack() after new values: xkept

The inputs hold the shapes at which a paired layout can go wrong: batch_edges (roots of 7, 8, 9, 16, 17, 24, 25 and leaves of
128, 129, 192, 193: odd reduction lengths and lengths 1 and 7 mod 8), long_root (a second chunk round), narrow_only (a
ragged last pack)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import solve_restatement as sr  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "solve_tiles_child.py")
PLANS = {
    "default": {},
    "rows64": {"DPGO_SPD_FINE_FWD": "0", "DPGO_SPD_FINE_BWD": "0", "DPGO_SPD_FINE_BWD_TALL": "0", "DPGO_SPD_FINE_ROOT": "0",
               "DPGO_SPD_FINE_ROOT8": "0"},
    "root16": {"DPGO_SPD_FINE_ROOT8": "0"},
    "stream_once": {"DPGO_SPD_KEEP_MB": "0"},
    "host_panels": {"DPGO_SPD_DEVICE_PANELS": "0"},
    "dynamic": {},
}
INPUTS = list(sr.INPUTS)
COMBOS = [(3, 1), (3, 3), (2, 1), (2, 2)]

_children = {}
_dead = []   # why no further child is started


@pytest.fixture(scope="module")
def pairs_tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("solve_panel_pairs")


def results(tmp_dir, plan, pairs, timeout=180):
    """{input: {"<d><dof>": {field: array}}} of the child of (plan, DPGO_SPD_PANEL_PAIRS = pairs), started on first use."""
    if (plan, pairs) in _children:
        return _children[plan, pairs]
    if _dead:
        pytest.fail("no further child process is started: " + _dead[0])
    out = os.path.join(str(tmp_dir), "%s_%d.npz" % (plan, pairs))
    cmd = [sys.executable, CHILD, out] + (["dynamic"] if plan == "dynamic" else [])
    env = dict(os.environ, **PLANS[plan], DPGO_SPD_PANEL_PAIRS=str(pairs))
    try:
        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    except subprocess.TimeoutExpired:
        _dead.append("child %r (pairs %d) ran into its timeout of %d s" % (plan, pairs, timeout))
        pytest.fail(_dead[0])
    if p.returncode != 0:
        _dead.append("child %r (pairs %d) ended with status %d:\n%s" % (plan, pairs, p.returncode,
                                                                        p.stderr.decode(errors="replace")[-2000:]))
        pytest.fail(_dead[0])
    r = {}
    npz = np.load(out)
    for key in npz.files:
        a, b, c = key.split("|")
        r.setdefault(a, {}).setdefault(b, {})[c] = npz[key]
    _children[plan, pairs] = r
    return r


@pytest.mark.parametrize("tag", list(PLANS))
def test_same_bits_and_same_plan_under_both_layouts(pairs_tmp, tag):
    plain, paired = results(pairs_tmp, tag, 0), results(pairs_tmp, tag, 1)
    compared = 0
    for name in INPUTS:
        for d, dof in COMBOS:
            a, b = plain[name]["%d%d" % (d, dof)], paired[name]["%d%d" % (d, dof)]
            for k in ("flags", "levels", "counts"):
                assert np.array_equal(a[k], b[k]), (tag, name, d, dof, k)
            assert ("xkept" in a) == ("xkept" in b) == (tag == "dynamic")
            for k in ("x", "xneg") + (("xkept",) if "xkept" in a else ()):
                assert a[k].shape == b[k].shape and np.array_equal(sr.bits(a[k]), sr.bits(b[k])), (tag, name, d, dof, k)
                compared += 1
    assert compared == len(INPUTS) * len(COMBOS) * (3 if tag == "dynamic" else 2)
