"""The device multifrontal solve (spd_solve.cpp: upload, repack, Level::map, fine_root_for, spd_run; kernels.hip: k_spd_level,
k_root_sym, k_root_combine, k_root_syrk, k_pack_panels) tile class by tile class, against an extended-precision solve
(tests/solve_restatement.py) on inputs whose front shapes are chosen.  Inputs, references and the bound are validated on the
host in tests/test_solve_restatement_host.py; here dpgo_amd.SpdSolverDebug runs spd_run itself.

The library reads its settings once per process, so every plan is a child process (tests/solve_tiles_child.py) that runs
all inputs for d = 3, 2 and dof = 1, d and writes what the hook returned to a file; the parent compares.  A child that ends
by a signal, by its timeout or with an error fails the module's remaining tests without another child being started.

  tag            environment                                                    what runs
  default        --                                                             16-row levels, 8-row fused roots, NT = false
  rows64         DPGO_SPD_FINE_FWD=0 _BWD=0 _BWD_TALL=0 _ROOT=0 _ROOT8=0        64-row tiles everywhere
  root16         DPGO_SPD_FINE_ROOT8=0                                          16-row roots (an 8-row fine class is cut)
  root64         DPGO_SPD_FINE_ROOT=0 DPGO_SPD_FINE_ROOT8=0                     64-row roots (a 16-row fine class is cut)
  root16_fine    DPGO_SPD_FINE_ROOT8=3                                          16-row roots, the 8-row class for few live nodes
  root64_fine    DPGO_SPD_FINE_ROOT=3 DPGO_SPD_FINE_ROOT8=0                     64-row roots, the 16-row class for few live nodes
  two_sweeps     DPGO_SPD_FUSE_ROOT=0                                           roots inside the sweeps; in == out
  triangle_1/3/8 DPGO_SPD_ROOT_SYM=1 DPGO_SPD_ROOT_SYM_BLOCKS=1/3/8             k_root_sym + k_root_combine, nb = 1 roots included
  stream_once    DPGO_SPD_KEEP_MB=0                                             the NT = true instantiations
  host_panels    DPGO_SPD_DEVICE_PANELS=0                                       panels packed on the host
  dynamic        keep_numeric                                                   repack(), roots inside the sweeps
  dynamic_fused  keep_numeric, DPGO_SPD_FUSE_ROOT_DYNAMIC=1                     repack() with k_root_syrk again
(root16 / root64 cut a finer class that a threshold of 0 never selects; the two *_fine plans are there to run it.)

Per plan and input: the plan read-back names the class of the table and every launch's tile height and tile counts are
those a restatement of upload() expects (solve_restatement.tile_classes); the solution is within
10 kappa_1 u |x_ref|_1 per column and connected component; every entry of `out` that is not an unknown of a live node keeps
its sentinel bits; a second run has the same bits; scale = -1 gives the negated bits; in place gives the bits of in != out
under two_sweeps / dynamic and is refused wherever a root is fused.  stream_once and host_panels equal default bit for bit
(the host packer copies the same factor: the numeric phase ran on the device in both).
"""
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
ROWS64 = {"DPGO_SPD_FINE_FWD": "0", "DPGO_SPD_FINE_BWD": "0", "DPGO_SPD_FINE_BWD_TALL": "0", "DPGO_SPD_FINE_ROOT": "0",
          "DPGO_SPD_FINE_ROOT8": "0"}
PLANS = {
    "default": {},
    "rows64": ROWS64,
    "root16": {"DPGO_SPD_FINE_ROOT8": "0"},
    "root64": {"DPGO_SPD_FINE_ROOT": "0", "DPGO_SPD_FINE_ROOT8": "0"},
    "root16_fine": {"DPGO_SPD_FINE_ROOT8": "3"},
    "root64_fine": {"DPGO_SPD_FINE_ROOT": "3", "DPGO_SPD_FINE_ROOT8": "0"},
    "two_sweeps": {"DPGO_SPD_FUSE_ROOT": "0"},
    "triangle_1": {"DPGO_SPD_ROOT_SYM": "1", "DPGO_SPD_ROOT_SYM_BLOCKS": "1"},
    "triangle_3": {"DPGO_SPD_ROOT_SYM": "1", "DPGO_SPD_ROOT_SYM_BLOCKS": "3"},
    "triangle_8": {"DPGO_SPD_ROOT_SYM": "1", "DPGO_SPD_ROOT_SYM_BLOCKS": "8"},
    "stream_once": {"DPGO_SPD_KEEP_MB": "0"},
    "host_panels": {"DPGO_SPD_DEVICE_PANELS": "0"},
    "dynamic": {},
    "dynamic_fused": {"DPGO_SPD_FUSE_ROOT_DYNAMIC": "1"},
}
DYNAMIC = ("dynamic", "dynamic_fused")
MASK_PLANS = ("default", "triangle_3", "two_sweeps", "root16_fine", "root64_fine")
INPUTS = list(sr.INPUTS)
COMBOS = [(3, 1), (3, 3), (2, 1), (2, 2)]


def thresholds(plan):
    env = PLANS[plan]
    return {k: int(env.get("DPGO_SPD_" + k.upper(), v)) for k, v in sr.DEFAULT_THRESHOLDS.items()}


# ---------------------------------------------------------------------------------------------------------------
# children: one process per plan, started once, never retried
# ---------------------------------------------------------------------------------------------------------------
_children = {}
_dead = []   # why no further child is started


@pytest.fixture(scope="module")
def tiles_tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("solve_tiles")


def results(tmp_dir, plan, timeout=180):
    """{input: {"<d><dof>": {field: array}}} of the child of `plan` (started on first use)."""
    if plan in _children:
        return _children[plan]
    if _dead:
        pytest.fail("no further child process is started: " + _dead[0])
    out = os.path.join(str(tmp_dir), plan + ".npz")
    cmd = [sys.executable, CHILD, out] + (["dynamic"] if plan in DYNAMIC else [])
    try:
        p = subprocess.run(cmd, env=dict(os.environ, **PLANS[plan]), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    except subprocess.TimeoutExpired:
        _dead.append("child %r ran into its timeout of %d s" % (plan, timeout))
        pytest.fail(_dead[0])
    if p.returncode != 0:
        _dead.append("child %r ended with status %d:\n%s" % (plan, p.returncode, p.stderr.decode(errors="replace")[-2000:]))
        pytest.fail(_dead[0])
    r = {}
    npz = np.load(out)
    for key in npz.files:
        a, b, c = key.split("|")
        r.setdefault(a, {}).setdefault(b, {})[c] = npz[key]
    _children[plan] = r
    return r


def plan_of(run):
    """A run of the child in the shape SpdSolverDebug.plan() returns."""
    fl = run["flags"]
    nf, nb = (int(v) for v in run["nlevels"])
    lv = [dict(rows=int(a[0]), nwide=int(a[1]), nnarrow=int(a[2]), wcount=c[:, 0], ncount=c[:, 1])
          for a, c in zip(run["levels"], run["counts"])]
    w, u = run["w"], run["u"]
    pp, up = np.concatenate([[0], np.cumsum(w)]), np.concatenate([[0], np.cumsum(u)])
    return {"fused_root": bool(fl[0]), "root_sym": bool(fl[1]), "root_rows": int(fl[2]), "root_fine_rows": int(fl[3]),
            "root_fine_below": int(fl[4]), "stream_once": bool(fl[5]), "nnodes": int(fl[6]), "fwd": lv[:nf], "bwd": lv[nf:nf + nb],
            "root": lv[-3], "root_fine": lv[-2], "root_rows_level": lv[-1], "nfronts": len(w), "w": w, "u": u,
            "parent": run["parent"], "height": run["height"], "piv_idx": [run["piv_idx"][pp[s]:pp[s + 1]] for s in range(len(w))],
            "upd_idx": [run["upd_idx"][up[s]:up[s + 1]] for s in range(len(w))]}


def key(d, dof):
    return "%d%d" % (d, dof)


def has_fused_roots(plan):
    return any(sr.is_fused_root(plan, f) for f in range(plan["nfronts"]))


def unknowns_of(name, d, dof, nodes=None):
    """(rows of the record array that hold unknowns of the nodes, mask of all other entries)."""
    inp = sr.build_input(name)
    rows = sr.unknown_rows(inp.n, d, dof)
    live = np.ones(inp.n, bool) if nodes is None else np.isin(inp.nodes, list(nodes))
    other = np.ones(sr.record_shape(inp.n, d, dof), bool)
    other[rows[live]] = False
    return rows, live, other


def check_left_alone(x, name, d, dof, nodes=None, sentinel=sr.SENT_OUT):
    _, _, other = unknowns_of(name, d, dof, nodes)
    assert np.all(sr.bits(x)[other] == sr.bits(np.asarray([sentinel]))[0]), "%s: an entry outside the live unknowns was written" % name


# ---------------------------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(PLANS))
def test_plan_read_back_names_the_class(tiles_tmp, tag):
    r = results(tiles_tmp, tag)
    th = thresholds(tag)
    levels16 = roots = 0
    for name in INPUTS:
        for d, dof in COMBOS:
            plan = plan_of(r[name][key(d, dof)])
            sr.check_input_structure(name, plan)
            tiles = sr.tile_classes(plan, th)   # (asserts every launch's tile height and counts)
            fused = has_fused_roots(plan)
            if name == "gauge":
                assert not plan["fused_root"]   # the root's pivots span more than 1e9: two sweeps under every plan
            elif tag in ("two_sweeps", "dynamic"):
                assert not plan["fused_root"]
            else:
                assert plan["fused_root"] and fused
            assert plan["stream_once"] == (tag == "stream_once")
            assert plan["root_sym"] == (tag.startswith("triangle") and fused)
            levels16 += sum(v["rows"] == 16 and v["nwide"] > 0 for v in plan["fwd"] + plan["bwd"])
            if fused and not plan["root_sym"]:
                roots += 1
                if tag == "root16" and name != "mixed_launch":   # (521 root tiles: 64 rows unless every threshold says otherwise)
                    assert plan["root_rows"] == 16
                if tag in ("rows64", "root64"):
                    assert plan["root_rows"] == 64
                if name == "three_nodes":   # (five 64-row tiles: at or above the *_fine plans' threshold of 3)
                    assert tag != "root16_fine" or plan["root_rows"] == 16
                    assert tag != "root64_fine" or plan["root_rows"] == 64
                    want = {"rows64": (16, 0), "root16": (8, 0), "root64": (16, 0), "root16_fine": (8, 3),
                            "root64_fine": (16, 3)}.get(tag, (0, 0))
                    assert (plan["root_fine_rows"], plan["root_fine_below"]) == (want if tag not in DYNAMIC else (0, 0))
                else:
                    assert plan["root_fine_rows"] == 0   # (one node: no finer class)
            if plan["root_sym"]:
                S = int(PLANS[tag]["DPGO_SPD_ROOT_SYM_BLOCKS"])
                nbs = [(int(plan["w"][f]) + 63) // 64 for f in range(plan["nfronts"]) if sr.is_fused_root(plan, f)]
                assert plan["root"]["nnarrow"] == sum(-(-(i + 1) // S) for nb in nbs for i in range(nb))
                assert plan["root_rows_level"]["nwide"] == sum(nbs)
            if tag == "rows64":
                assert all(v["rows"] == 64 for v in plan["fwd"] + plan["bwd"])
            if tag == "default" and fused:
                assert plan["root_rows"] == (64 if name == "mixed_launch" else 8)
            del tiles
    assert (levels16 == 0) == (tag == "rows64")
    assert roots > 0 or tag in ("two_sweeps", "dynamic") or tag.startswith("triangle")


def test_host_panels_plan_is_the_default_plan(tiles_tmp):
    a, b = results(tiles_tmp, "default"), results(tiles_tmp, "host_panels")
    for name in INPUTS:
        for k in ("flags", "levels", "counts"):
            assert np.array_equal(a[name]["31"][k], b[name]["31"][k]), (name, k)


def test_every_case_the_inputs_were_made_for_occurs(tiles_tmp):
    """The second chunk round, the mixed wide and narrow grid, the ragged narrow pack, the nb = 1 triangle root, three
    nodes that differ at shared levels, and every arm of the streaming loop for 1, 4 and 8 lanes per row."""
    th = thresholds("default")
    d, two, r64 = results(tiles_tmp, "default"), results(tiles_tmp, "two_sweeps"), results(tiles_tmp, "rows64")
    # reductions beyond 8 x 128: fused root (8 lanes per row), and inside both sweeps
    t = sr.tile_classes(plan_of(d["long_root"]["31"]), th)
    assert sr.second_chunk_round(t, "root") and sr.second_chunk_round(t, "fwd") and sr.second_chunk_round(t, "bwd")
    t = sr.tile_classes(plan_of(two["long_root"]["31"]), th)
    assert sum(x[0] == "fwd" and x[4] == 1100 for x in t) and sum(x[0] == "bwd" and x[4] == 1100 for x in t)
    # wide and narrow packs in one grid
    for r in (d, two):
        plan = plan_of(r["mixed_launch"]["31"])
        assert plan["fwd"][0]["nwide"] > 0 and plan["fwd"][0]["nnarrow"] >= sr.MERGE_BELOW
        assert plan["bwd"][-1]["nwide"] > 0 and plan["bwd"][-1]["nnarrow"] >= sr.MERGE_BELOW
    # merged: narrow fronts in the wide class
    plan = plan_of(d["class_edges"]["31"])
    assert plan["fwd"][0]["nnarrow"] == 0 and plan["fwd"][0]["nwide"] > 0
    # a ragged last narrow pack behind full ones
    plan = plan_of(d["narrow_only"]["31"])
    for lev in (plan["fwd"][0], plan["bwd"][-1]):
        assert lev["nwide"] == 0 and lev["ncount"][0] > sr.WAVES and lev["ncount"][0] % sr.WAVES
    # the triangle: one-block roots, and 18 block rows with a ragged last one
    tri = results(tiles_tmp, "triangle_3")
    plan = plan_of(tri["batch_edges"]["31"])
    assert plan["root_sym"] and any(sr.is_fused_root(plan, f) and plan["w"][f] <= 64 for f in range(plan["nfronts"]))
    plan = plan_of(tri["long_root"]["31"])
    assert plan["root_sym"] and 1100 in plan["w"].tolist() and 1100 % 64 == 12
    # three nodes: node 2 has no tile in any sweep level, nodes 0 and 1 differ at the leaf level
    plan = plan_of(d["three_nodes"]["31"])
    for lev in plan["fwd"] + plan["bwd"]:
        assert lev["wcount"][2] + lev["ncount"][2] == 0
    assert plan["fwd"][0]["wcount"][0] != plan["fwd"][0]["wcount"][1] and plan["root"]["wcount"][2] > 0
    # the streaming loop
    seen = set()
    for r, tag in ((d, "default"), (r64, "rows64")):
        for name in INPUTS:
            seen |= sr.stream_cases(sr.tile_classes(plan_of(r[name]["31"]), thresholds(tag)))
    print(sorted(seen))
    for kq in (1, 4, 8):
        for what in ("full", "second", "rest", "rest_only") + (("third",) if kq < 8 else ()):   # (8 lanes: a chunk is 16 loads)
            assert (kq, what) in seen, (kq, what)


# ---------------------------------------------------------------------------------------------------------------
# the solution
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", INPUTS)
@pytest.mark.parametrize("tag", list(PLANS))
def test_solution_within_the_bound(tiles_tmp, tag, name):
    r = results(tiles_tmp, tag)[name]
    for d, dof in COMBOS:
        x = r[key(d, dof)]["x"]
        rows, _, _ = unknowns_of(name, d, dof)
        ratios = sr.solve_ratios(x[rows], name, d, dof)
        print("%s %s d %d dof %d: worst error / bound %.3g" % (tag, name, d, dof, ratios.max()))
        assert np.all(np.isfinite(x[rows])) and ratios.max() <= 1.0, (tag, name, d, dof, ratios.max())


@pytest.mark.parametrize("name", INPUTS)
@pytest.mark.parametrize("tag", list(PLANS))
def test_left_alone_same_bits_twice_scale_and_in_place(tiles_tmp, tag, name):
    r = results(tiles_tmp, tag)[name]
    for d, dof in COMBOS:
        run = r[key(d, dof)]
        x = run["x"]
        check_left_alone(x, name, d, dof)
        assert np.array_equal(sr.bits(run["x2"]), sr.bits(x)), "a second run differs"
        rows, _, _ = unknowns_of(name, d, dof)
        check_left_alone(run["xneg"], name, d, dof)
        assert np.array_equal(sr.bits(-run["xneg"][rows]), sr.bits(x[rows])), "scale = -1 is not the negated scale = +1"
        if has_fused_roots(plan_of(run)):
            assert "refused" in run and "xip" not in run     # spd_run's own error, as a return code
        else:
            check_left_alone(run["xip"], name, d, dof, sentinel=sr.SENT_IN)
            assert np.array_equal(sr.bits(run["xip"][rows]), sr.bits(x[rows])), "in == out differs from in != out"


@pytest.mark.parametrize("tag", ["stream_once", "host_panels"])
def test_same_bits_as_default(tiles_tmp, tag):
    a, b = results(tiles_tmp, "default"), results(tiles_tmp, tag)
    for name in INPUTS:
        for d, dof in COMBOS:
            for k in ("x", "xneg"):
                assert np.array_equal(sr.bits(a[name][key(d, dof)][k]), sr.bits(b[name][key(d, dof)][k])), (name, d, dof, k)


# ---------------------------------------------------------------------------------------------------------------
# masks
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", MASK_PLANS)
def test_masks(tiles_tmp, tag):
    """Every subset of three_nodes' nodes: in mask.v (the roots' class chosen for all nodes), in the device word under
    mask.v = all, and in mask.v with the class chosen for the subset -- which, under the *_fine plans, is the finer one."""
    name = "three_nodes"
    r = results(tiles_tmp, tag)[name]
    fine_seen = coarse_seen = 0
    for d, dof in COMBOS:
        run = r[key(d, dof)]
        plan = plan_of(run)
        x = run["x"]
        for b in range(1, 8):
            nodes = [a for a in range(3) if (b >> a) & 1]
            rows, live, _ = unknowns_of(name, d, dof, nodes)
            for k in ("mv%d" % b, "mw%d" % b):
                check_left_alone(run[k], name, d, dof, nodes)
                assert np.array_equal(sr.bits(run[k][rows[live]]), sr.bits(x[rows[live]])), (tag, k, d, dof)
            live_tiles = sum(int(plan["root"]["wcount"][a]) for a in nodes)
            predicted = (plan["fused_root"] and not plan["root_sym"] and plan["root_fine_rows"] > 0 and live_tiles > 0
                         and live_tiles * plan["root_rows"] // 64 < plan["root_fine_below"])
            assert bool(run["fine%d" % b][0]) == predicted, (tag, b, live_tiles)
            xf = run["mf%d" % b]
            check_left_alone(xf, name, d, dof, nodes)
            if predicted:
                fine_seen += 1
                assert sr.solve_ratios(xf[rows], name, d, dof, nodes=nodes).max() <= 1.0
            else:
                coarse_seen += 1
                assert np.array_equal(sr.bits(xf[rows[live]]), sr.bits(x[rows[live]])), (tag, b, d, dof)
    assert coarse_seen > 0 and (fine_seen > 0) == tag.endswith("_fine")


# ---------------------------------------------------------------------------------------------------------------
# repack
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", INPUTS)
@pytest.mark.parametrize("tag", DYNAMIC)
def test_repack_has_the_bits_of_a_fresh_upload(tiles_tmp, tag, name):
    """refactor(): new values on the device, spd_refactor_device, repack() -- what a Dynamic rescale does to G_tt."""
    r = results(tiles_tmp, tag)[name]
    for d, dof in COMBOS:
        run = r[key(d, dof)]
        rows, _, _ = unknowns_of(name, d, dof)
        check_left_alone(run["xkept"], name, d, dof)
        # (the fresh handle made the same plan: a factor that is re-done keeps the plan of its first upload)
        assert np.array_equal(run["fresh_flags"], run["flags"]) and np.array_equal(run["fresh_levels"], run["levels"])
        assert np.array_equal(sr.bits(run["xkept"]), sr.bits(run["xfresh"])), (tag, name, d, dof)
        ratios = sr.solve_ratios(run["xkept"][rows], name, d, dof, second=True)
        print("%s %s d %d dof %d, second values: worst error / bound %.3g" % (tag, name, d, dof, ratios.max()))
        assert ratios.max() <= 1.0
