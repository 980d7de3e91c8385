"""Extended-precision restatement of the multifrontal factor (dpgo_amd/csrc/spd.h): test infrastructure, like
tests/cert_restatement.py.  Plain numpy / scipy; nothing of the library is imported here.

What the library stores per front s (w pivots, u update rows) is  W_s = [L11^-1 ; -L21 L11^-1]  ((w + u) x w).  Fronts are
stored in post-order (spd_solve_host relies on it), so the elimination order is piv_idx concatenated over the fronts, and
with  L = chol(A[perm][:, perm])  the blocks of front s are  L11 = L[P, P]  (P: its pivot positions, a contiguous range) and
L21 = L[Q, P]  (Q: the positions of its update rows).  L is computed densely in np.longdouble (x87 extended, eps 1.08e-19:
2 000 times below fp64), once per matrix; X = L11^-1 by long-double substitution.

The module also holds
  * the structural facts this construction relies on (check_structure),
  * a plain fp64 restatement (np.linalg.cholesky, scipy.linalg.solve_triangular, one product) whose only use is to show what
    ordinary fp64 achieves against the reference,
  * the inputs of tests/test_factor_fronts_host.py and tests/test_gpu_factor_fronts.py: clique patterns whose elimination
    trees have fronts of chosen shapes, and two value families on them.
"""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

LD = np.longdouble
# (asserted, not skipped: a platform whose long double is a plain double has no reference to offer)
assert np.finfo(LD).eps < 2e-19, "np.longdouble is not an extended-precision type here (eps = %g)" % np.finfo(LD).eps

U = 2.0 ** -53


# ---------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------
def cholesky_ld(A):
    """(L, kstar): the lower Cholesky factor of the dense symmetric A in long double, left-looking by columns (only the lower
    triangle is touched).  kstar = -1, or the index of the first non-positive pivot, where the loop stops (the columns from
    kstar on are then zero); d[k] are the pivots d_kk = L[k, k]^2 before the square root."""
    n = A.shape[0]
    L = np.zeros((n, n), LD)
    Al = np.asarray(A, LD)
    d = np.zeros(n, LD)
    for k in range(n):
        col = Al[k:, k] - L[k:, :k] @ L[k, :k]
        d[k] = col[0]
        if not col[0] > 0:
            return L, k, d
        lkk = np.sqrt(col[0])
        L[k, k] = lkk
        L[k + 1:, k] = col[1:] / lkk
    return L, -1, d


def lower_inverse_ld(T):
    """T^-1 of a lower-triangular long-double T by forward substitution on the identity, row by row."""
    w = T.shape[0]
    X = np.zeros((w, w), LD)
    for i in range(w):
        r = -(T[i, :i] @ X[:i, :])
        r[i] += 1
        X[i] = r / T[i, i]
    return X


def elimination_order(res):
    return np.concatenate([np.asarray(p, np.int64) for p in res["piv_idx"]])


def front_ranges(res):
    """Per front: (first pivot position, positions of its update rows) in the elimination order."""
    perm = elimination_order(res)
    pos = np.empty(len(perm), np.int64)
    pos[perm] = np.arange(len(perm))
    first = np.concatenate([[0], np.cumsum(res["w"])])
    return [(int(first[s]), pos[np.asarray(res["upd_idx"][s], np.int64)]) for s in range(res["nfronts"])]


class Reference:
    """The long-double factor of a dense symmetric matrix in the elimination order of `res` (what the hook returned for it),
    its per-front blocks W_ref, its pivots, and kappa_2."""

    def __init__(self, A, res):
        A = np.asarray(A, np.float64)
        self.n = A.shape[0]
        self.perm = elimination_order(res)
        self.Ap = A[np.ix_(self.perm, self.perm)]
        self.L, self.kstar, self.d = cholesky_ld(self.Ap)
        lam = np.linalg.eigvalsh(A)
        self.kappa = float(lam[-1] / lam[0]) if lam[0] > 0 else np.inf
        self.ranges = front_ranges(res)
        self.w = [int(v) for v in res["w"]]
        self._W = {}
        self._Lf = None

    def pivots(self):
        assert self.kstar < 0
        return np.asarray(self.d, LD)

    def W(self, s):
        """W_ref of front s: (w + u) x w, long double, the zero upper triangle of L11^-1 included."""
        if s not in self._W:
            p0, Q = self.ranges[s]
            P = slice(p0, p0 + self.w[s])
            X = lower_inverse_ld(self.L[P, P])
            self._W[s] = np.vstack([X, -(self.L[Q, P] @ X)]) if len(Q) else X
        return self._W[s]

    def W_fp64(self, s):
        """The same block by ordinary fp64: np.linalg.cholesky, solve_triangular, one product."""
        if self._Lf is None:
            self._Lf = np.linalg.cholesky(self.Ap)
        p0, Q = self.ranges[s]
        P = slice(p0, p0 + self.w[s])
        X = sla.solve_triangular(self._Lf[P, P], np.eye(self.w[s]), lower=True)
        return np.vstack([X, -(self._Lf[Q, P] @ X)]) if len(Q) else X

    def bound(self, s, u_rows):
        """Entrywise bound of front s: (w + u) u kappa_2(A) max|W_ref,s| -- the first-order normwise perturbation bound of a
        Cholesky factor and of a product with it; not a sharp constant."""
        return (self.w[s] + u_rows) * U * self.kappa * float(np.abs(self.W(s)).max())


# ---------------------------------------------------------------------------------------------------------------
# what the hook returned, taken apart
# ---------------------------------------------------------------------------------------------------------------
def front_W(res, s, key="W"):
    """(W_s as (w + u) x ldw, WT_s as w x ldm) of front s: views into the flat arrays, padding included."""
    w, u, ldw, ldm = int(res["w"][s]), int(res["u"][s]), int(res["ldw"][s]), int(res["ldm"][s])
    o, ot = int(res["w_off"][s]), int(res["wt_off"][s])
    W = res[key][o:o + (w + u) * ldw].reshape(w + u, ldw)
    WT = res[key + "T"][ot:ot + w * ldm].reshape(w, ldm)
    return W, WT


def check_structure(res, n):
    """The structure the reference's construction relies on."""
    nt = res["nfronts"]
    w, u, parent = res["w"], res["u"], res["parent"]
    assert len(w) == len(u) == len(parent) == nt
    for s in range(nt):   # post-order: a parent comes after its children
        assert parent[s] == -1 or nt > parent[s] > s, (s, parent[s])
    perm = elimination_order(res)
    assert sorted(perm.tolist()) == list(range(n)), "the pivot sets do not partition 0..n-1"
    for s in range(nt):
        assert len(res["piv_idx"][s]) == w[s] and len(res["upd_idx"][s]) == u[s]
        assert res["ldw"][s] >= w[s] and res["ldm"][s] >= w[s] + u[s]
        ups = set(int(v) for v in res["upd_idx"][s])
        assert len(ups) == u[s]
        if parent[s] < 0:
            assert u[s] == 0, "a root with update rows"
        else:
            p = parent[s]
            held = set(int(v) for v in res["piv_idx"][p]) | set(int(v) for v in res["upd_idx"][p])
            assert ups <= held, "front %d: an update row that its parent %d does not hold" % (s, p)
    # heights: leaves 0, a parent one above its tallest child
    h = np.zeros(nt, np.int64)
    for s in range(nt):
        if parent[s] >= 0:
            h[parent[s]] = max(h[parent[s]], h[s] + 1)
    assert np.array_equal(h, res["height"])
    # the flat arrays hold the fronts one after the other
    off = offt = 0
    for s in range(nt):
        assert res["w_off"][s] == off and res["wt_off"][s] == offt
        off += (int(w[s]) + int(u[s])) * int(res["ldw"][s])
        offt += int(w[s]) * int(res["ldm"][s])
    if res.get("W") is not None:
        assert len(res["W"]) == off and len(res["WT"]) == offt


def check_layout(res, key="W"):
    """WT[k, p] == W[p, k] bit for bit over the (w + u) x w of every front; the padding is exactly zero."""
    for s in range(res["nfronts"]):
        w, u = int(res["w"][s]), int(res["u"][s])
        W, WT = front_W(res, s, key)
        assert np.array_equal(WT[:, :w + u].view(np.int64), W[:, :w].T.view(np.int64)), "front %d: WT is not W^T" % s
        assert not W[:, w:].view(np.int64).any(), "front %d: padding of W is not zero" % s
        assert not WT[:, w + u:].view(np.int64).any(), "front %d: padding of WT is not zero" % s


def factor_ratios(res, ref, key="W"):
    """Per front: max |W_dev - W_ref| / bound over its (w + u) x w entries (zero upper triangle included)."""
    out = np.zeros(res["nfronts"])
    for s in range(res["nfronts"]):
        w, u = int(res["w"][s]), int(res["u"][s])
        W, _ = front_W(res, s, key)
        err = np.abs(np.asarray(W[:, :w], LD) - ref.W(s)).max()
        out[s] = float(err) / ref.bound(s, u)
    return out


def fp64_ratios(ref, res):
    """The same figure for the fp64 restatement."""
    out = np.zeros(res["nfronts"])
    for s in range(res["nfronts"]):
        err = np.abs(np.asarray(ref.W_fp64(s), LD) - ref.W(s)).max()
        out[s] = float(err) / ref.bound(s, int(res["u"][s]))
    return out


def pivot_errors(res, ref, suffix=""):
    """(relative error of pivot_min, of pivot_max, the bound n u kappa_2) against min / max diag(L_ref)^2."""
    d = ref.pivots()
    lo, hi = d.min(), d.max()
    return (float(abs(LD(res["pivot_min" + suffix]) - lo) / lo), float(abs(LD(res["pivot_max" + suffix]) - hi) / hi),
            ref.n * U * ref.kappa)


# ---------------------------------------------------------------------------------------------------------------
# inputs: clique patterns whose fronts have the shapes that matter
# ---------------------------------------------------------------------------------------------------------------
def clique_pattern(sizes, couplings):
    """Boolean n x n pattern: dense cliques of the given sizes (vertices numbered clique after clique), cliques a and b fully
    coupled for every (a, b) in couplings, nothing else."""
    first = np.concatenate([[0], np.cumsum(sizes)])
    n = int(first[-1])
    P = np.zeros((n, n), bool)
    for a in range(len(sizes)):
        P[first[a]:first[a + 1], first[a]:first[a + 1]] = True
    for a, b in couplings:
        P[first[a]:first[a + 1], first[b]:first[b + 1]] = True
        P[first[b]:first[b + 1], first[a]:first[a + 1]] = True
    return P


def block_arrow(sizes, n_s):
    """Cliques of `sizes`, each fully coupled to a separator clique of n_s (the last clique); with collapse = 1 and
    leaf >= max(sizes) the fronts are the leaves (n_i, n_s) and the root (n_s, 0)."""
    k = len(sizes)
    return clique_pattern(list(sizes) + [n_s], [(a, k) for a in range(k)])


def disjoint(*patterns):
    n = sum(p.shape[0] for p in patterns)
    P = np.zeros((n, n), bool)
    o = 0
    for p in patterns:
        P[o:o + p.shape[0], o:o + p.shape[0]] = p
        o += p.shape[0]
    return P


def values(P, family, seed, shift=0.0, diag_scale=1.0):
    """A dense symmetric matrix on the pattern P.
    "mixed":     off-diagonals uniform in (-1, 1), diagonal = 1.05 x the absolute row sum + 1 (signs mix: nothing about
                 M-matrices hides a sign error);
    "laplacian": the project's own class (G_tt is one): off-diagonals -weight, weights uniform in (0.5, 2), diagonal = row
                 sum of the weights + shift.
    diag_scale multiplies the diagonal afterwards (the refactorisation's second value array)."""
    rng = np.random.default_rng(seed)
    n = P.shape[0]
    R = rng.uniform(-1.0, 1.0, (n, n)) if family == "mixed" else -rng.uniform(0.5, 2.0, (n, n))
    R = np.tril(R, -1)
    A = (R + R.T) * P
    np.fill_diagonal(A, 0.0)
    absrow = np.abs(A).sum(axis=1)
    np.fill_diagonal(A, (1.05 * absrow + 1.0 if family == "mixed" else absrow + shift) * diag_scale)
    return A


def to_csr(A, P):
    """CSR with exactly the entries of the pattern (sorted indices; zeros of the pattern stay stored)."""
    n = A.shape[0]
    Pd = P | np.eye(n, dtype=bool)
    rows, cols = np.nonzero(Pd)
    return sp.csr_matrix((A[rows, cols], (rows, cols)), shape=(n, n))


# NB = 32, SB = 128, TS = 64 (spd_dev.hip); a workgroup holds 128 rows left-looking, 256 right-looking.
# Each input: pattern, value family, (leaf, collapse, block), seed.  SHIFT: see DESIGN.md (the factorisation's tests).
SHIFT = 1e-2


def _nested():
    # cliques:     0:T  1:S1  2    3    4   5:S2  6   7   8
    sizes = [96, 65, 64, 100, 20, 63, 97, 31, 8]
    coup = [(1, 0), (5, 0), (2, 1), (3, 1), (4, 1), (6, 5), (7, 5), (8, 5), (2, 0), (7, 0)]
    return clique_pattern(sizes, coup)


def _edges():
    # (two cliques a, b and a separator s with a + s and b both within 45 - 55 % of the component: the dissector's level cut
    # finds s itself; a clique cannot be cut, whatever the leaf size)
    return disjoint(block_arrow([128, 127], 1), block_arrow([32, 33], 8), block_arrow([31, 64], 33), block_arrow([], 7))


def _kron4(P):
    return np.kron(P, np.ones((4, 4), bool))


INPUTS = {
    # fronts 5/161, 33/161, 129/161, 290/161 in one level, the root 161/0
    "arrow_wide": dict(pattern=lambda: block_arrow([5, 33, 129, 290], 161), family="mixed", leaf=290, collapse=1, block=1, seed=1),
    # 1/300, 160/300, 257/300, the root 300/0
    "arrow_tall": dict(pattern=lambda: block_arrow([1, 160, 257], 300), family="laplacian", leaf=257, collapse=1, block=1, seed=2),
    # four trees: block-column and super-block edges side by side (32 beside 33; 31 beside 64; 127 beside 128 over a 1-wide
    # separator) and a tree that is one front
    "arrow_edges": dict(pattern=_edges, family="mixed", leaf=64, collapse=1, block=1, seed=3),
    "arrow_edges_lap": dict(pattern=_edges, family="laplacian", leaf=64, collapse=1, block=1, seed=4),
    # three tree levels; leaves whose update rows pass through their parent to the grandparent
    "nested": dict(pattern=_nested, family="laplacian", leaf=128, collapse=1, block=1, seed=5),
    # unknowns in groups of 4 that share their neighbours, ordered on the quotient graph
    "arrow_block4": dict(pattern=lambda: _kron4(block_arrow([2, 8, 9, 40], 17)), family="mixed", leaf=160, collapse=1, block=4,
                         seed=6),
}

_built = {}


def build_input(name, second=False):
    """(A dense, CSR) of a named input; second: the values of the refactorisation -- another seed, the diagonal times 3."""
    key = (name, second)
    if key not in _built:
        spec = INPUTS[name]
        P = spec["pattern"]()
        A = values(P, spec["family"], spec["seed"] + (1000 if second else 0), SHIFT, 3.0 if second else 1.0)
        _built[key] = (A, to_csr(A, P))
    return _built[key]
