"""Extended-precision restatement of the multifrontal SOLVE (dpgo_amd/csrc/spd_solve.cpp, k_spd_level, k_root_sym +
k_root_combine): test infrastructure in the style of tests/factor_restatement.py, whose long-double Cholesky and input
builders it reuses.  Plain numpy / scipy; nothing of the library is imported here.

Reference.  x_ref = A^-1 b in np.longdouble, connected component by connected component (the solver's trees never couple
two components, and neither does the reference): the dense long-double Cholesky and two long-double substitutions for
components of up to CHOLESKY_MAX unknowns; above, a scipy fp64 sparse LU and three rounds of refinement with the residual
in long double -- a route that is only allowed because it agrees with the Cholesky route to 1e-3 of the bound on every
smaller input (asserted in tests/test_solve_restatement_host.py).

Bound.  The project's own (tests/test_gpu_operators.py), per column and per component c:
    |x_c - x_ref,c|_1  <=  BOUND_C kappa_1(A_c) u |x_ref,c|_1,        u = 2^-53,
kappa_1 = |A_c|_1 |A_c^-1|_1 from the dense fp64 inverse.  Summed over the components this implies the bound with
kappa_1(A) of the whole matrix; component by component it is the stricter statement, and the one a launch mask needs.
BOUND_C = 10.  It was checked, before any device was asked, against plain fp64 restatements of both routes the device takes
(sweeps(): two triangular sweeps over the fronts; with fused=True the roots are applied as L11^-T L11^-1 formed in fp64,
whose error is kappa u in every component): the worst ratio error / (kappa_1 u |x_ref|_1) over all inputs, both routes,
is recorded by tests/test_solve_restatement_host.py and must leave at least 4x below BOUND_C (DESIGN.md has the figures).

Right-hand sides.  Standard normal, d columns, at the unknowns' rows of a record array ((d + 1) rows of d doubles per
record; dof 1: row 0 of record i, the translation; dof d: row 1 + i % d of record i // d, the rotation rows); every
other entry of `in` and of `out` holds a sentinel (SENT_IN / SENT_OUT: quiet NaNs with a payload, so that an entry the solve
read by mistake poisons the result and an entry it wrote by mistake loses its bits).
"""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.csgraph as csgraph
import scipy.sparse.linalg as spla

import factor_restatement as fr
from factor_restatement import LD, U, block_arrow, clique_pattern, disjoint

BOUND_C = 10.0
CHOLESKY_MAX = 1300
SENT_IN = np.array([0x7ff8_0000_dead_0001], np.uint64).view(np.float64)[0]
SENT_OUT = np.array([0x7ff8_0000_beef_0002], np.uint64).view(np.float64)[0]


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
def _class_edges():
    # leaves 95/1 and 96/1 (backward: 96 narrow, 97 wide), 90/7 beside 97/7 (90: narrow forward, wide backward), the
    # single-front trees 96/0 and 97/0 (forward: 96 narrow, 97 wide)
    return disjoint(block_arrow([95, 96], 1), block_arrow([90, 97], 7), block_arrow([], 96), block_arrow([], 97))


def _narrow_only():
    # 19 cliques of 1 .. 19 vertices over a separator clique of 8 whose vertex j is coupled to every (j + 1)-th clique: the
    # positions of the root pull 1 to 19 rows (the dissector moves two cliques into the root), a leaf's pivots none
    sizes = list(range(1, 20))
    P = block_arrow(sizes, 8)
    first = np.concatenate([[0], np.cumsum(sizes)])
    s0 = int(first[-1])
    for j in range(8):
        for a in range(19):
            if a % (j + 1):
                P[first[a]:first[a + 1], s0 + j] = P[s0 + j, first[a]:first[a + 1]] = False
    return P


def _batch_edges():
    singles = [block_arrow([], w) for w in (7, 8, 9, 16, 17, 24, 25)]
    return disjoint(*(singles + [block_arrow([128, 129], 3), block_arrow([192, 193], 3)]))


MIXED_ARROWS = 520   # two 5/1 leaves each: 1040 narrow leaf tiles >= MERGE_BELOW (1024)


def _mixed_launch():
    # (5 + 1 and 5 of 11 vertices: the smallest arrow both of whose sides the dissector's level cut accepts)
    return disjoint(*([block_arrow([100, 99], 3)] + [block_arrow([5, 5], 1)] * MIXED_ARROWS))


def _three_nodes():
    return disjoint(fr._nested(), block_arrow([100, 99], 9), block_arrow([], 70))


def _three_nodes_of():
    return np.repeat([0, 1, 2], [fr._nested().shape[0], 208, 70])


def _gauge():
    return block_arrow([60, 55], 6)


# pattern, value family, (leaf, collapse, block), seed; shift: the Laplacian family's diagonal shift (default
# factor_restatement.SHIFT); nodes: the local node of every unknown (default: all on node 0); second_diag: what multiplies
# the diagonal of the second values, those of the refactorisation (default 3)
INPUTS = dict(fr.INPUTS)
INPUTS.update({
    "class_edges": dict(pattern=_class_edges, family="mixed", leaf=97, collapse=1, block=1, seed=11),
    "narrow_only": dict(pattern=_narrow_only, family="laplacian", leaf=19, collapse=1, block=1, seed=12),
    # A front with u > 1024 over few pivots (10/1100) is not something the dissector makes: a separator is a minimum cover of
    # a cut that leaves both sides 45 - 55 % of the vertices, so it is never wider than the smaller side, and the spectral
    # candidate goes through a clique as soon as that is cheaper.  Reductions beyond 8 x 128 are therefore reached by a
    # single-front tree of 1100 (forward, backward, fused; 18 blocks of the triangle, the last 12 rows high) and by leaves
    # 600/450 (1050 rows backward) and 1050/450 (1050 columns forward, 1500 rows backward) under a 450-wide root.
    "long_root": dict(pattern=lambda: disjoint(block_arrow([], 1100), block_arrow([600, 1050], 450)), family="mixed", leaf=1050,
                      collapse=1, block=1, seed=13),
    "batch_edges": dict(pattern=_batch_edges, family="mixed", leaf=193, collapse=1, block=1, seed=14),
    "mixed_launch": dict(pattern=_mixed_launch, family="laplacian", leaf=10, collapse=1, block=1, seed=15),
    "three_nodes": dict(pattern=_three_nodes, family="laplacian", leaf=128, collapse=1, block=1, seed=16, nodes=_three_nodes_of),
    # (second values: other weights, the same shift -- the plan of the first upload stays with a factor that is re-done, so a
    # second matrix whose roots could be fused would not have the plan of a fresh upload)
    "gauge": dict(pattern=_gauge, family="laplacian", leaf=60, collapse=1, block=1, seed=17, shift=1e-11, second_diag=1.0),
})

_built = {}


class Input:
    """A named input: CSR matrix (the pattern's entries, zeros included), its connected components with their dense
    blocks, the hook's arguments and the node of every unknown."""

    def __init__(self, name, second=False):
        spec = INPUTS[name]
        P = spec["pattern"]()
        self.name, self.n = name, P.shape[0]
        self.args = (spec["leaf"], spec["collapse"], spec["block"])
        self.nodes = spec["nodes"]() if "nodes" in spec else np.zeros(self.n, np.int32)
        assert len(self.nodes) == self.n
        ncomp, label = csgraph.connected_components(sp.csr_matrix(P), directed=False)
        self.comps = [np.flatnonzero(label == c) for c in range(ncomp)]
        # values component by component (a component's block is all the reference ever needs densely); components of the
        # same node only
        rows, cols, vals = [], [], []
        self.blocks = []
        for c, idx in enumerate(self.comps):
            assert len(set(self.nodes[idx].tolist())) == 1, "a component on two nodes"
            Pc = P[np.ix_(idx, idx)]
            Ac = fr.values(Pc, spec["family"], 7919 * spec["seed"] + c + (1000003 if second else 0), spec.get("shift", fr.SHIFT),
                           spec.get("second_diag", 3.0) if second else 1.0)
            self.blocks.append(Ac)
            r, k = np.nonzero(Pc | np.eye(len(idx), dtype=bool))
            rows.append(idx[r]); cols.append(idx[k]); vals.append(Ac[r, k])
        self.csr = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(self.n, self.n))
        self.csr.sort_indices()
        self.nnodes = int(self.nodes.max()) + 1
        self._ref = None

    def reference(self):
        if self._ref is None:
            self._ref = [ComponentReference(A) for A in self.blocks]
        return self._ref

    def node_of_component(self, c):
        return int(self.nodes[self.comps[c][0]])


def build_input(name, second=False):
    key = (name, second)
    if key not in _built:
        _built[key] = Input(name, second)
    return _built[key]


# ---------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------
def solve_cholesky_ld(A, B, L=None):
    """A^-1 B in long double: Cholesky, forward and backward substitution row by row."""
    if L is None:
        L, kstar, _ = fr.cholesky_ld(A)
        assert kstar < 0, "the reference does not find the matrix positive definite"
    n = A.shape[0]
    Y = np.zeros((n, B.shape[1]), LD)
    Bl = np.asarray(B, LD)
    for i in range(n):
        Y[i] = (Bl[i] - L[i, :i] @ Y[:i]) / L[i, i]
    X = np.zeros_like(Y)
    for i in range(n - 1, -1, -1):
        X[i] = (Y[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X


def solve_refined(A, B, rounds=3, lu=None):
    """The route of large components: scipy's fp64 sparse LU, then `rounds` of refinement with the residual in long double."""
    lu = lu or spla.splu(sp.csc_matrix(A))
    Al, Bl = np.asarray(A, LD), np.asarray(B, LD)
    X = np.asarray(lu.solve(np.asarray(B, np.float64)), LD)
    for _ in range(rounds):
        R = Bl - Al @ X
        X = X + np.asarray(lu.solve(np.asarray(R, np.float64)), LD)
    return X


class ComponentReference:
    """kappa_1 of a dense SPD block and its long-double solves."""

    def __init__(self, A):
        self.A = np.asarray(A, np.float64)
        self.n = self.A.shape[0]
        inv = np.linalg.inv(self.A)
        self.kappa1 = float(np.abs(self.A).sum(axis=0).max() * np.abs(inv).sum(axis=0).max())
        self._L = self._lu = None

    def solve(self, B, route=None):
        route = route or ("cholesky" if self.n <= CHOLESKY_MAX else "refined")
        if route == "refined":
            if self._lu is None:
                self._lu = spla.splu(sp.csc_matrix(self.A))
            return solve_refined(self.A, B, lu=self._lu)
        if self._L is None:
            self._L, kstar, _ = fr.cholesky_ld(self.A)
            assert kstar < 0, "the reference does not find the matrix positive definite"
        return solve_cholesky_ld(self.A, B, self._L)

    def bound(self, Xref):
        """Per column: BOUND_C kappa_1 u |x_ref|_1."""
        return BOUND_C * self.kappa1 * U * np.asarray(np.abs(Xref).sum(axis=0), np.float64)


# ---------------------------------------------------------------------------------------------------------------
# record arrays
# ---------------------------------------------------------------------------------------------------------------
def unknown_rows(n, d, dof):
    """Row of unknown i in a record array of shape (records * (d + 1), d)."""
    i = np.arange(n)
    return i * (d + 1) if dof == 1 else (i // dof) * (d + 1) + 1 + i % dof


def record_shape(n, d, dof):
    return (((n + dof - 1) // dof) * (d + 1), d)


def rhs(name, d, dof, second=False):
    """(B, in, out): the right-hand side n x d, and the two record arrays as the solve is handed them."""
    inp = build_input(name)
    rng = np.random.default_rng(100 * INPUTS[name]["seed"] + 10 * d + dof + (5 if second else 0))
    B = rng.standard_normal((inp.n, d))
    vin = np.full(record_shape(inp.n, d, dof), SENT_IN)
    vin[unknown_rows(inp.n, d, dof)] = B
    return B, vin, np.full(record_shape(inp.n, d, dof), SENT_OUT)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


_solutions = {}


def solution(name, d, dof, second=False):
    """x_ref (n x d, long double) of rhs(name, d, dof, second) for the input's first or second values: one solve per
    (input, values, d, dof), shared by every plan and never changed."""
    key = (name, d, dof, second)
    if key not in _solutions:
        inp = build_input(name, second)
        B = rhs(name, d, dof, second)[0]
        X = np.zeros((inp.n, d), LD)
        for idx, ref in zip(inp.comps, inp.reference()):
            X[idx] = ref.solve(B[idx])
        X.setflags(write=False)
        _solutions[key] = X
    return _solutions[key]


def solve_ratios(X, name, d, dof, second=False, nodes=None):
    """Per component (of the nodes in `nodes`, default all): max over the columns of |x - x_ref|_1 / bound."""
    inp = build_input(name, second)
    Xref = solution(name, d, dof, second)
    out = []
    for c, (idx, ref) in enumerate(zip(inp.comps, inp.reference())):
        if nodes is not None and inp.node_of_component(c) not in nodes:
            continue
        err = np.asarray(np.abs(np.asarray(X[idx], LD) - Xref[idx]).sum(axis=0), np.float64)
        out.append(float((err / ref.bound(Xref[idx])).max()))
    return np.asarray(out)


# ---------------------------------------------------------------------------------------------------------------
# plain fp64 restatements of the two routes of the device solve
# ---------------------------------------------------------------------------------------------------------------
def fronts_fp64(A, res):
    """Per front W_s = [L11^-1 ; -L21 L11^-1] by ordinary fp64: np.linalg.cholesky, solve_triangular, one product."""
    perm = fr.elimination_order(res)
    L = np.linalg.cholesky(np.asarray(A, np.float64)[np.ix_(perm, perm)])
    out = []
    for s, (p0, Q) in enumerate(fr.front_ranges(res)):
        P = slice(p0, p0 + int(res["w"][s]))
        X = sla.solve_triangular(L[P, P], np.eye(int(res["w"][s])), lower=True)
        out.append(np.vstack([X, -(L[Q, P] @ X)]) if len(Q) else X)
    return out


def sweeps(res, W, B, fused=False, scale=1.0, mutate=None):
    """scale * A^-1 B by the fronts W in fp64, position by position as the device does it: forward, in post-order,
    f = [b_s ; 0] + the rows each position pulls from the children's update vectors, [y ; upd] = W_s f_piv + [0 ; f_upd];
    backward, in reverse, x_s = W_s^T [y_s ; x_upd], written as scale * x_s -- so the ancestors' entries a front gathers
    are multiplied by scale again (+-1: the undo).  fused: a root (no update rows) takes  x = (W^T W) f  with the product
    formed first, as the fused root launches do.
    mutate (tests of the tests): "backward_scale_undo" drops the undo; "asm_ptr_off_by_one" lets position p pull the list of
    position p + 1."""
    nt = res["nfronts"]
    kids = [[] for _ in range(nt)]
    for s in range(nt):
        if res["parent"][s] >= 0:
            kids[int(res["parent"][s])].append(s)
    nc = B.shape[1]
    X = np.zeros((B.shape[0], nc))
    Y, UPD, done = [None] * nt, [None] * nt, np.zeros(nt, bool)
    for s in range(nt):
        piv, upd, w = np.asarray(res["piv_idx"][s], np.int64), np.asarray(res["upd_idx"][s], np.int64), int(res["w"][s])
        pos = np.concatenate([piv, upd])
        want = np.concatenate([pos[1:], [-1]]) if mutate == "asm_ptr_off_by_one" else pos
        f = np.zeros((len(pos), nc))
        f[:w] = B[piv]
        for c in kids[s]:   # (in list order, as the assembly lists are)
            loc = {int(v): i for i, v in enumerate(res["upd_idx"][c])}
            hit = np.asarray([loc.get(int(v), -1) for v in want])
            f[hit >= 0] += UPD[c][hit[hit >= 0]]
        if fused and res["parent"][s] < 0 and len(upd) == 0 and w > 0:
            X[piv] = scale * ((W[s].T @ W[s]) @ f)
            done[s] = True
            continue
        out = W[s] @ f[:w]
        Y[s] = out[:w]
        UPD[s] = out[w:] + f[w:]
    for s in range(nt - 1, -1, -1):
        if done[s]:
            continue
        piv, upd = np.asarray(res["piv_idx"][s], np.int64), np.asarray(res["upd_idx"][s], np.int64)
        sc = 1.0 if mutate == "backward_scale_undo" else scale
        X[piv] = scale * (W[s].T @ np.vstack([Y[s], sc * X[upd]]))
    return X


def restated_solve(name, table, B, fused=False, scale=1.0, mutate=None, second=False):
    """sweeps() on every connected component of a named input (table: its front table)."""
    inp = build_input(name, second)
    X = np.zeros_like(B)
    for idx, A in zip(inp.comps, inp.blocks):
        ct = component_table(table, idx)
        X[idx] = sweeps(ct, fronts_fp64(A, ct), B[idx], fused=fused, scale=scale, mutate=mutate)
    return X


# ---------------------------------------------------------------------------------------------------------------
# what a plan runs, restated from the front table and the plan read-back (spd_solve.cpp: upload)
# ---------------------------------------------------------------------------------------------------------------
WIDE_ABOVE, MERGE_BELOW, CHUNK, WAVES, HALF_BATCH = 96, 1024, 128, 8, 8


def depths(plan):
    dep = np.zeros(plan["nfronts"], np.int64)
    for f in range(plan["nfronts"] - 1, -1, -1):
        if plan["parent"][f] >= 0:
            dep[f] = dep[plan["parent"][f]] + 1
    return dep


def is_fused_root(plan, f):
    return plan["fused_root"] and plan["parent"][f] < 0 and plan["u"][f] == 0 and plan["w"][f] > 0


DEFAULT_THRESHOLDS = dict(fine_fwd=192, fine_bwd=256, fine_bwd_tall=800, fine_root=192, fine_root8=64)


def tile_classes(plan, thresholds=None):
    """The tiles of every launch as (sweep, rows, lanes per row KQ, waves NW, reduction length, chunk length, last chunk's
    length): sweep in "fwd", "bwd", "root"; narrow tiles have rows 64, NW 1.  The counts are checked against the read-back,
    and with `thresholds` (the DPGO_SPD_FINE_* of the plan) so is every launch's tile height."""
    w, u = plan["w"], plan["u"]
    dep = depths(plan)
    out = []

    def chunks(length, nw):
        cl = CHUNK if nw == 1 else min(max(((length + nw - 1) // nw + 7) & ~7, 8), CHUNK)
        last = length - (length - 1) // cl * cl
        return cl, last

    for sweep, key, level_of in (("fwd", "fwd", plan["height"]), ("bwd", "bwd", dep)):
        fwd = sweep == "fwd"
        for l, lev in enumerate(plan[key]):
            fronts = [f for f in range(plan["nfronts"]) if level_of[f] == l and not is_fused_root(plan, f) and w[f] + u[f] > 0]
            red = lambda f: w[f] if fwd else w[f] + u[f]
            ext = lambda f: w[f] + u[f] if fwd else w[f]
            t64 = lambda wide: sum((ext(f) + 63) // 64 for f in fronts if (red(f) > WIDE_ABOVE) == wide)
            merge = t64(True) > 0 and t64(False) < MERGE_BELOW
            if thresholds is not None:
                wide_tiles = t64(True) + (t64(False) if merge else 0)
                longest = max([w[f] + u[f] for f in fronts] + [0])
                fine = wide_tiles < thresholds["fine_fwd"] if fwd else (
                    wide_tiles < thresholds["fine_bwd"] or (wide_tiles < thresholds["fine_bwd_tall"] and longest >= 1000))
                assert lev["rows"] == (16 if wide_tiles > 0 and fine else 64), (sweep, l, lev["rows"], wide_tiles, longest)
            nwide = nnarrow = 0
            for f in fronts:
                wide_class = red(f) > WIDE_ABOVE or merge
                th = lev["rows"] if wide_class else 64
                for r in range(0, ext(f), th):
                    length = (min(r + th, w[f]) if r + th <= w[f] else w[f]) if fwd else w[f] + u[f] - r
                    nw = WAVES if wide_class else 1
                    out.append((sweep, th, 64 // th, nw, int(length)) + chunks(int(length), nw))
                    nwide, nnarrow = nwide + wide_class, nnarrow + (not wide_class)
            assert (nwide, nnarrow) == (lev["nwide"], lev["nnarrow"]), (sweep, l, nwide, nnarrow, lev)
    roots = [f for f in range(plan["nfronts"]) if is_fused_root(plan, f)]
    if roots and thresholds is not None and not plan["root_sym"]:
        t64 = sum((w[f] + 63) // 64 for f in roots)
        assert plan["root"]["rows"] == (8 if t64 < thresholds["fine_root8"] else 16 if t64 < thresholds["fine_root"] else 64)
    if plan["fused_root"] and not plan["root_sym"]:
        th = plan["root"]["rows"]
        for f in range(plan["nfronts"]):
            if is_fused_root(plan, f):
                for r in range(0, w[f], th):
                    out.append(("root", th, 64 // th, WAVES, int(w[f])) + chunks(int(w[f]), WAVES))
    return out


def stream_cases(tiles):
    """{(KQ, what)}: which arms of stream_first / stream_rest a set of tiles takes, per lanes-per-row: "full" (a first
    half-batch of HALF_BATCH loads), "second" (the other buffer), "third" (the first buffer again), "rest" (the predicated
    remainder), "rest_only"."""
    seen = set()
    for _, rows, kq, nw, length, cl, last in tiles:
        for kn in {cl if length > cl else last, last}:
            for q in range(kq):
                full = (kn - q + kq - 1) // kq // HALF_BATCH if kn > q else 0   # whole half-batches of lane group q
                cnt = (kn - q + kq - 1) // kq if kn > q else 0
                if full >= 1: seen.add((kq, "full"))
                if full >= 2: seen.add((kq, "second"))
                if full >= 3: seen.add((kq, "third"))
                if cnt % HALF_BATCH: seen.add((kq, "rest" if full else "rest_only"))
    return seen


def second_chunk_round(tiles, sweep):
    return any(t[0] == sweep and t[3] == WAVES and t[4] > WAVES * CHUNK for t in tiles)


# ---------------------------------------------------------------------------------------------------------------
# the structure every input was made for, asserted from a front table (the host hook's or the plan read-back's)
# ---------------------------------------------------------------------------------------------------------------
def front_set(t):
    return [(int(w), int(u)) for w, u in zip(t["w"], t["u"])]


def component_table(t, idx):
    """The fronts of the component with the (sorted) matrix indices idx, renumbered: a front table of its own."""
    loc = {int(v): i for i, v in enumerate(idx)}
    keep = [s for s in range(t["nfronts"]) if len(t["piv_idx"][s]) and int(t["piv_idx"][s][0]) in loc]
    new = {s: i for i, s in enumerate(keep)}
    return {"nfronts": len(keep), "w": np.asarray([t["w"][s] for s in keep]), "u": np.asarray([t["u"][s] for s in keep]),
            "parent": np.asarray([new.get(int(t["parent"][s]), -1) for s in keep]),
            "piv_idx": [np.asarray([loc[int(v)] for v in t["piv_idx"][s]], np.int64) for s in keep],
            "upd_idx": [np.asarray([loc[int(v)] for v in t["upd_idx"][s]], np.int64) for s in keep]}


def pull_lengths(t, f):
    """Per position (pivots, then update rows) of front f: the rows it pulls, one per child that holds the index."""
    kids = [s for s in range(t["nfronts"]) if t["parent"][s] == f]
    pos = np.concatenate([np.asarray(t["piv_idx"][f], np.int64), np.asarray(t["upd_idx"][f], np.int64)])
    return np.asarray([sum(int(v) in set(t["upd_idx"][s].tolist()) for s in kids) for v in pos])


def check_input_structure(name, t):
    """t: a front table (w, u, parent, height, piv_idx, upd_idx).  Only the inputs added here; those of
    factor_restatement.INPUTS have their table in tests/test_factor_fronts_host.py."""
    fs = front_set(t)
    h = np.asarray(t["height"])
    if name == "class_edges":
        for want in ((95, 1), (96, 1), (96, 0), (97, 0), (90, 7), (97, 7)):
            assert want in fs, (name, want, fs)
    elif name == "narrow_only":
        leaves = [f for f in range(t["nfronts"]) if h[f] == 0]
        assert len(leaves) > WAVES and len(leaves) % WAVES, len(leaves)   # a ragged last pack, and more than one
        assert all(t["w"][f] + t["u"][f] <= WIDE_ABOVE and t["u"][f] > 0 for f in leaves)
        root = [f for f in range(t["nfronts"]) if t["parent"][f] < 0]
        assert len(root) == 1 and t["w"][root[0]] <= WIDE_ABOVE
        pl = pull_lengths(t, root[0])
        assert pl.max() >= 16 and set((pl % 4).tolist()) == {0, 1, 2, 3}, pl   # every residue of PULLB = 2, 4; several rounds
    elif name == "long_root":
        assert sorted(fs) == [(450, 0), (600, 450), (1050, 450), (1100, 0)], fs
    elif name == "batch_edges":
        for w in (7, 8, 9, 16, 17, 24, 25):
            assert (w, 0) in fs
        for w in (128, 129, 192, 193):
            assert (w, 3) in fs
    elif name == "mixed_launch":
        assert fs.count((5, 1)) == 2 * MIXED_ARROWS >= MERGE_BELOW and (100, 3) in fs and (99, 3) in fs
        assert all(h[f] == 0 for f in range(t["nfronts"]) if t["u"][f] > 0)
    elif name == "three_nodes":
        node = _three_nodes_of()
        of = np.asarray([node[int(t["piv_idx"][f][0])] for f in range(t["nfronts"])])
        assert h[of == 0].max() == 2 and h[of == 1].max() == 1 and (of == 1).sum() == 3
        assert (of == 2).sum() == 1 and fs[int(np.flatnonzero(of == 2)[0])] == (70, 0)
    elif name == "gauge":
        assert t["nfronts"] == 3 and (np.asarray(t["parent"]) < 0).sum() == 1
