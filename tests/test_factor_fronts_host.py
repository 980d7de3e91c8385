"""The multifrontal factor front by front, on the host numeric path (spd.cpp), against an extended-precision Cholesky
(tests/factor_restatement.py): what dpgo_amd.spd_factor_debug returns for inputs whose fronts have chosen shapes.

No GPU: the child process runs under DPGO_SPD_HOST_FACTOR=1.  This validates the reference, the permutation logic, the
bounds and the inputs (the coverage table below is asserted from the symbolic analysis alone), so that on a GPU
(tests/test_gpu_factor_fronts.py, which takes its helpers from here) the only new thing under test is spd_dev.hip.

Bounds (u = 2^-53, kappa_2 from eigvalsh of the input):
  factor   per front, entrywise: |W - W_ref| <= (w + u_rows) u kappa_2(A) max|W_ref,s|  -- the first-order normwise
           perturbation bound of a Cholesky factor and of a product with it, not a sharp constant; the zero upper triangle of
           L11^-1 is part of W_ref and held to the same bound;
  pivots   pivot_min / pivot_max equal min / max diag(L_ref)^2 within n u kappa_2(A), relative.
A condition on the INPUTS, not on the code under test: the plain fp64 restatement and the host path stay at or below 1/10 of
the factor bound on every front (the Laplacian-like family's shift is chosen for it, factor_restatement.SHIFT).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import factor_restatement as fr  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "factor_fronts_child.py")
INPUTS = list(fr.INPUTS)

# ---------------------------------------------------------------------------------------------------------------
# children: one process per elimination path, started once, never retried
# ---------------------------------------------------------------------------------------------------------------
_children = {}
_dead = []   # why no further child is started: a child ended by a signal, by its timeout or with an error


def split(npz):
    """{input or case: {run: {field: array}}} of a child's file."""
    out = {}
    for key in npz.files:
        a, b, c = key.split("|")
        out.setdefault(a, {}).setdefault(b, {})[c] = npz[key]
    return out


def as_result(run, structure):
    """A run of the child in the shape dpgo_amd.spd_factor_debug returns (the structure is that of the input's first run)."""
    res = {k: structure[k] for k in ("w", "u", "parent", "height", "ldw", "ldm", "w_off", "wt_off")}
    res["nfronts"] = int(structure["nfronts"])
    pp = np.concatenate([[0], np.cumsum(res["w"])])
    up = np.concatenate([[0], np.cumsum(res["u"])])
    res["piv_idx"] = [structure["piv_idx"][pp[s]:pp[s + 1]] for s in range(res["nfronts"])]
    res["upd_idx"] = [structure["upd_idx"][up[s]:up[s + 1]] for s in range(res["nfronts"])]
    for k in ("status", "fail_front"):
        res[k] = int(run[k])
    for k in ("pivot_min", "pivot_max"):
        res[k] = float(run[k])
    res["on_device"] = bool(run["on_device"])
    res["W"], res["WT"] = run.get("W"), run.get("WT")
    return res


def child(tag, env, tmp_dir, fails=None, timeout=120):
    """The split results of the child `tag` (started on first use).  A child that ends by a signal, by its timeout or with an
    error fails this and every later request without another process being started."""
    if tag in _children:
        return _children[tag]
    if _dead:
        pytest.fail("no further child process is started: " + _dead[0])
    out = os.path.join(str(tmp_dir), tag + ".npz")
    cmd = [sys.executable, CHILD, out] + ([fails] if fails else [])
    try:
        p = subprocess.run(cmd, env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    except subprocess.TimeoutExpired:
        _dead.append("child %r ran into its timeout of %d s" % (tag, timeout))
        pytest.fail(_dead[0])
    if p.returncode != 0:
        _dead.append("child %r ended with status %d:\n%s" % (tag, p.returncode, p.stderr.decode(errors="replace")[-2000:]))
        pytest.fail(_dead[0])
    r = split(np.load(out))
    r["_output"] = (p.stdout + p.stderr).decode(errors="replace")
    _children[tag] = r
    return r


@pytest.fixture(scope="session")
def fronts_tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("factor_fronts")


def host_results(tmp_dir):
    return child("host", {"DPGO_SPD_HOST_FACTOR": "1"}, tmp_dir)


# ---------------------------------------------------------------------------------------------------------------
# references: one long-double Cholesky per (input, value array), shared by every path
# ---------------------------------------------------------------------------------------------------------------
_refs = {}


def structure(tmp_dir, name):
    return as_result(host_results(tmp_dir)[name]["first"], host_results(tmp_dir)[name]["first"])


def reference(tmp_dir, name, second=False):
    key = (name, second)
    if key not in _refs:
        _refs[key] = fr.Reference(fr.build_input(name, second)[0], structure(tmp_dir, name))
        assert _refs[key].kstar < 0, "the reference does not find %s positive definite" % name
    return _refs[key]


# ---------------------------------------------------------------------------------------------------------------
# indefinite inputs: one diagonal entry replaced so that the reference meets its first non-positive pivot at a chosen k*
# ---------------------------------------------------------------------------------------------------------------
_cases = {}


def failure_cases(tmp_dir):
    """{case: dict(input, values (CSR order), kstar, allowed fronts)}.  The new diagonal entry is A_vv - d_k - t with d_k
    the reference's pivot and t > 0 of the size of the matrix entries: the pivot becomes -t, the columns before k* do not
    change (a pivot depends on the columns left of it alone), so k* is the first non-positive one -- which the reference
    then confirms on the changed matrix."""
    if _cases:
        return _cases

    def make(case, name, pick, own_entries_fine=False):
        res, ref = structure(tmp_dir, name), reference(tmp_dir, name)
        A, csr = fr.build_input(name)
        s, k_local = pick(res)
        k = int(np.concatenate([[0], np.cumsum(res["w"])])[s]) + k_local
        v = int(ref.perm[k])
        d_k, a_vv = float(ref.d[k]), A[v, v]
        below = a_vv - d_k                                   # what the earlier columns take from the diagonal entry
        t = 0.25 * (below if own_entries_fine else a_vv)
        B = A.copy()
        B[v, v] = below - t
        if own_entries_fine:
            # the front's own entries are those of a positive definite matrix: only its Schur complement is not
            P = np.asarray(res["piv_idx"][s], np.int64)
            assert B[v, v] > 0 and np.linalg.eigvalsh(B[np.ix_(P, P)])[0] > 0
        _, kstar, d = fr.cholesky_ld(B[np.ix_(ref.perm, ref.perm)])
        assert kstar == k and float(d[k]) < -0.2 * t, (case, kstar, k)   # the reference decides, before any device is asked
        allowed, a = set(), s
        while a >= 0:
            allowed.add(a)
            a = int(res["parent"][a])
        _cases[case] = dict(input=name, values=fr.to_csr(B, fr.INPUTS[name]["pattern"]()).data, kstar=k, front=s, allowed=allowed)
        assert np.array_equal(fr.to_csr(B, fr.INPUTS[name]["pattern"]()).indices, csr.indices)

    def small_leaf(res):   # the first block column of a leaf with w <= 8 that shares its level with a w >= 257 front
        for s in range(res["nfronts"]):
            mates = [t for t in range(res["nfronts"]) if res["height"][t] == res["height"][s]]
            if res["w"][s] <= 8 and res["height"][s] == 0 and any(res["w"][t] >= 257 for t in mates):
                return s, 0
        raise AssertionError("no such front")

    def wide_column(res):  # a column > 128 of a w >= 257 front: reached only through a wide pass
        s = int(np.argmax(res["w"]))
        assert res["w"][s] >= 257
        return s, 200

    def root(res):         # the first pivot of a root with children
        for s in range(res["nfronts"]):
            if res["parent"][s] < 0 and res["height"][s] > 0:
                return s, 0
        raise AssertionError("no such front")

    make("small_leaf", "arrow_wide", small_leaf)
    make("wide_column", "arrow_wide", wide_column)
    make("root_schur", "arrow_tall", root, own_entries_fine=True)
    return _cases


def fails_file(tmp_dir):
    path = os.path.join(str(tmp_dir), "fails.npz")
    if not os.path.exists(path):
        np.savez(path, **{"%s|%s" % (case, c["input"]): c["values"] for case, c in failure_cases(tmp_dir).items()})
    return path


# ---------------------------------------------------------------------------------------------------------------
# the checks, shared with the GPU tests
# ---------------------------------------------------------------------------------------------------------------
def check_factor(res, ref, label):
    """Item 2: every front against the reference; returns (and prints) the worst error / bound."""
    assert res["status"] == 0, label
    ratios = fr.factor_ratios(res, ref)
    worst = int(np.argmax(ratios))
    print("%s: worst error / bound %.3g (front %d: w %d, u %d)" % (label, ratios[worst], worst, res["w"][worst], res["u"][worst]))
    assert ratios.max() <= 1.0, "%s: front %d (w %d, u %d) is %.3g x its bound" % (label, worst, res["w"][worst], res["u"][worst],
                                                                                    ratios[worst])
    return float(ratios.max())


def check_pivots(res, ref, label):
    """Item 3."""
    e_min, e_max, bound = fr.pivot_errors(res, ref)
    print("%s: pivot_min %.17g (rel. error %.3g), pivot_max %.17g (%.3g), bound %.3g" % (label, res["pivot_min"], e_min,
                                                                                       res["pivot_max"], e_max, bound))
    assert e_min <= bound and e_max <= bound, label


def check_failure(results, case, c, label):
    """Item 7 for one case of one child."""
    r = results[case]
    assert int(r["fail"]["status"]) == 1, "%s: the verdict is not 'not positive definite'" % label
    assert int(r["fail"]["fail_front"]) in c["allowed"], "%s: front %d named, k* = %d lies in front %d" % (
        label, int(r["fail"]["fail_front"]), c["kstar"], c["front"])
    assert "W" not in r["fail"]
    assert "[dpgo_amd]" not in results["_output"] and "pivot" not in results["_output"], results["_output"]
    assert int(r["failonly"]["status"]) == 1 and int(r["failonly"]["fail_front"]) in c["allowed"]
    first = results[c["input"]]["first"]
    for run in ("after", "failkept"):   # the SPD input factored next, by a call of its own and through the context that failed
        assert int(r[run]["status"]) == 0
        for k in ("W", "WT", "pivot_min", "pivot_max"):
            assert np.array_equal(r[run][k], first[k]), "%s: %s of the run %r behind the failure differs" % (label, k, run)


# ---------------------------------------------------------------------------------------------------------------
# the inputs cover what they were made for
# ---------------------------------------------------------------------------------------------------------------
def test_inputs_cover_the_front_shapes(fronts_tmp):
    """NB = 32, SB = 128, TS = 64; a workgroup holds 128 rows left-looking and 256 right-looking.  Shapes are read from the
    hook, not assumed: the dissector chooses some separators of its own."""
    fronts = {}
    for name in INPUTS:
        res = structure(fronts_tmp, name)
        assert fr.INPUTS[name]["pattern"]().shape[0] <= 800
        fronts[name] = res
        print("%s (n = %d, leaf %d, block %d):" % (name, fr.INPUTS[name]["pattern"]().shape[0], fr.INPUTS[name]["leaf"],
                                                   fr.INPUTS[name]["block"]),
              " ".join("%d/%d@%d" % (w, u, h) for w, u, h in zip(res["w"], res["u"], res["height"])))
    wu = [(int(w), int(u)) for r in fronts.values() for w, u in zip(r["w"], r["u"])]
    ws = [w for w, _ in wu]

    def some(pred):
        return any(pred(w, u) for w, u in wu)

    # pivots
    for exact in (1, 31, 32, 33, 64, 128, 129, 160):
        assert exact in ws, "no front with w = %d" % exact
    assert some(lambda w, u: 97 <= w <= 127)
    assert some(lambda w, u: 161 <= w <= 255 and w % 32)
    assert some(lambda w, u: w >= 257 and w % 32)
    assert 290 in ws   # 128 + 128 + 32 + 2: two wide passes and a ragged third super-block
    # update rows
    assert some(lambda w, u: u == 0 and w > 128)
    assert some(lambda w, u: u == 1)
    assert some(lambda w, u: u in (63, 65))
    assert some(lambda w, u: u > w)
    assert some(lambda w, u: w + u > 256 and (w + u) % 64)

    def level_with(res, *preds):
        for h in set(int(v) for v in res["height"]):
            lw = [int(w) for w, hh in zip(res["w"], res["height"]) if hh == h]
            if all(any(p(w) for w in lw) for p in preds):
                return True
        return False

    # a level mixing widths
    assert any(level_with(r, lambda w: w <= 8, lambda w: w >= 257) for r in fronts.values())
    assert any(level_with(r, lambda w: w == 32, lambda w: w == 33) for r in fronts.values())
    # tree
    assert any(r["height"].max() >= 2 for r in fronts.values())
    assert any(np.bincount(r["parent"][r["parent"] >= 0]).max() >= 3 for r in fronts.values() if (r["parent"] >= 0).any())

    def passes_through(res):
        for s in range(res["nfronts"]):
            p = int(res["parent"][s])
            if p < 0:
                continue
            ups, ppiv = set(res["upd_idx"][s].tolist()), set(res["piv_idx"][p].tolist())
            if ups & ppiv and ups - ppiv:
                return True
        return False

    assert any(passes_through(r) for r in fronts.values())

    def two_trees(res):
        roots = [s for s in range(res["nfronts"]) if res["parent"][s] < 0]
        lone = [s for s in roots if res["height"][s] == 0 and res["u"][s] == 0 and res["w"][s] < 32]
        return len(roots) >= 2 and bool(lone)

    assert any(two_trees(r) for r in fronts.values())
    # block
    assert any(spec["block"] == 4 for spec in fr.INPUTS.values())
    for name, spec in fr.INPUTS.items():
        if spec["block"] == 4:   # ... whose groups of 4 stayed together
            for piv in fronts[name]["piv_idx"]:
                assert len(piv) % 4 == 0 and np.array_equal(np.sort(piv).reshape(-1, 4) % 4, np.tile(np.arange(4), (len(piv) // 4, 1)))


# ---------------------------------------------------------------------------------------------------------------
# items 1 - 3 on the host numeric path
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", INPUTS)
def test_structure_and_layout(fronts_tmp, name):
    runs = host_results(fronts_tmp)[name]
    n = fr.build_input(name)[0].shape[0]
    for run in ("first", "again", "kept", "fresh"):
        res = as_result(runs[run], runs["first"])
        assert not res["on_device"]
        fr.check_structure(res, n)
        fr.check_layout(res)


@pytest.mark.parametrize("name", INPUTS)
def test_factor_against_extended_precision(fronts_tmp, name):
    runs = host_results(fronts_tmp)[name]
    ref = reference(fronts_tmp, name)
    res = as_result(runs["first"], runs["first"])
    worst = check_factor(res, ref, "host %s" % name)
    plain = float(fr.fp64_ratios(ref, res).max())
    print("host %s: kappa_2 %.3g, the fp64 restatement is at %.3g of the bound" % (name, ref.kappa, plain))
    # the condition on the inputs: ordinary fp64 arithmetic uses at most a tenth of the bound
    assert plain <= 0.1 and worst <= 0.1
    assert np.array_equal(runs["again"]["W"], runs["first"]["W"]) and np.array_equal(runs["again"]["WT"], runs["first"]["WT"])
    # the second value array (the refactorisation's) against a reference of its own
    ref2 = reference(fronts_tmp, name, second=True)
    assert check_factor(as_result(runs["kept"], runs["first"]), ref2, "host %s, second values" % name) <= 0.1
    assert np.array_equal(runs["kept"]["W"], runs["fresh"]["W"]) and np.array_equal(runs["kept"]["WT"], runs["fresh"]["WT"])


@pytest.mark.parametrize("name", INPUTS)
def test_pivot_range(fronts_tmp, name):
    runs = host_results(fronts_tmp)[name]
    check_pivots(as_result(runs["first"], runs["first"]), reference(fronts_tmp, name), "host %s" % name)
    check_pivots(as_result(runs["kept"], runs["first"]), reference(fronts_tmp, name, second=True), "host %s, second values" % name)


@pytest.mark.parametrize("case", ["small_leaf", "wide_column", "root_schur"])
def test_non_positive_pivot_where_the_reference_puts_it(fronts_tmp, case):
    c = failure_cases(fronts_tmp)[case]
    results = child("host_fails", {"DPGO_SPD_HOST_FACTOR": "1"}, fronts_tmp, fails=fails_file(fronts_tmp))
    check_failure(results, case, c, "host %s" % case)
    # the host loop names the front that holds k* itself
    assert int(results[case]["fail"]["fail_front"]) == c["front"]
