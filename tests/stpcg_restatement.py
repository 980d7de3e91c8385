"""Restatement of the device-side control of the Steihaug-Toint CG (dpgo_amd/csrc/kernels.hip: k_cg_begin, tnt_begin_node,
cg_scal_logic, cg_scal_node, flag_arrive's hand-over): test infrastructure, like the other *_restatement.py modules.  Plain
Python on doubles; nothing of the library is imported here.

State: one record per node (the fields of CgNode, kernels.h), the three masks

    dmask[0]  the nodes of the step under way (Hessian product, s / H s update)
    dmask[1]  the nodes that go on to the preconditioner and to the next step
    dmask[2]  the active nodes whose CG is over (their trial point can be taken)

and the two pinned summaries: CG_SUMMARY words per node (stop ordinal or CG_LIVE_ORD, h_M_norm, cg_it) and the seven
TNT_SUMMARY words (the six start sums, then `active`).

Arithmetic is C's: sqrt of a negative number is NaN and every comparison with NaN is false (oracle/tnt.py does the same);
x / 0 is an infinity or NaN.

Every launch also leaves, per node,

    bound[field]   for each scalar the launch computed: 16 u times the sum of the absolute values of the terms of its
                   expression, the expression evaluated with mpmath at 120 bits from the same double inputs (`exact[field]`
                   is that value).  For the boundary root (-b + sqrt(b^2 + a c)) / a that is 16 u (|b| + sqrt(b^2 + a c)) / a.
                   Every stored scalar is fewer than 8 rounded operations on these terms, and the device may contract
                   multiply-adds where the host may not: 16.  A field without an entry was copied or set to a constant: it
                   is exact.
    margins        (what, relative margin) of every comparison the node took: |a - b| / max(|a|, |b|).  A comparison of
                   integers, one with a NaN side (false whatever the rounding) and the sign test of a sum that was handed
                   in (no arithmetic behind it) have margin inf.
    exit           what the launch decided for the node (the EXIT_* names below)
"""
import math

import mpmath

U = 2.0 ** -53
K = 16.0
CG_LIVE_ORD = 1e18
CG_SUMMARY_WORDS = 3
TNT_SUMMARY_WORDS = 7
KERNEL_EPS = 1e-8

FIELDS = ("sk_M_pk", "sk_M_2", "pk_M_2", "rv", "Delta", "Delta_2", "target", "h_M_norm", "c1", "cr", "al", "kap", "be")
INT_FIELDS = ("cg_it", "max_it", "live", "stop_ord")

# what a launch decided for a node
EXIT_NONE = "untouched"              # not part of the launch
EXIT_INACTIVE = "gradient tests"     # begin_device: failed a gradient test, no CG
EXIT_START_TARGET = "target at start"
EXIT_START_LIMIT = "limit at start"
EXIT_LIVE = "live"                   # begin: the CG runs
EXIT_STEP = "step"                   # phase 0: a plain step
EXIT_BOUNDARY = "boundary"
EXIT_CURVATURE = "curvature"
EXIT_KERNEL = "kernel"
EXIT_GO_ON = "go on"                 # phase 1: another step follows
EXIT_TARGET = "target"
EXIT_LIMIT = "limit"

_mp = mpmath.mp.clone()
_mp.prec = 120
_M = _mp.mpf


def c_sqrt(x):
    return math.sqrt(x) if x >= 0 else float("nan")


def c_div(a, b):
    if b != 0:
        try:
            return a / b
        except OverflowError:
            return math.copysign(math.inf, a) * math.copysign(1.0, b)
    if a == 0 or math.isnan(a):
        return float("nan")
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def c_mul(a, b):
    """(Python's float product is C's, inf * 0 = NaN included)"""
    return a * b


def rel_margin(a, b):
    if math.isnan(a) or math.isnan(b):
        return math.inf
    if math.isinf(a) or math.isinf(b):
        return math.inf if a != b else 0.0
    m = max(abs(a), abs(b))
    return abs(a - b) / m if m > 0 else 0.0


def _bound(terms):
    """16 u sum |terms| (mpmath values) as a double, rounded up"""
    return float(K * U * sum(abs(t) for t in terms)) * (1 + 2 * U)


def new_record():
    r = {f: 0.0 for f in FIELDS}
    r.update({f: 0 for f in INT_FIELDS})
    return r


class Node:
    """What a launch left for one node besides its record"""

    def __init__(self):
        self.bound, self.exact, self.margins, self.exit = {}, {}, [], EXIT_NONE

    def put(self, rec, field, value, exact=None, terms=None):
        rec[field] = value
        if terms is not None:
            self.exact[field] = exact
            self.bound[field] = _bound(terms)

    def took(self, what, a, b, exact=False):
        self.margins.append((what, math.inf if exact else rel_margin(a, b)))


def boundary_root(nd, rec, field, sgn=1.0):
    """rec[field] = sgn (-b + sqrt(b^2 + a c)) / a, b = sk_M_pk, a = pk_M_2, c = Delta_2 - sk_M_2"""
    b, a, D2, s2 = rec["sk_M_pk"], rec["pk_M_2"], rec["Delta_2"], rec["sk_M_2"]
    disc = b * b + a * (D2 - s2)
    v = sgn * c_div(-b + c_sqrt(disc), a)
    if math.isfinite(v):
        dm = _M(b) * _M(b) + _M(a) * (_M(D2) - _M(s2))
        root = _mp.sqrt(dm)
        nd.put(rec, field, v, sgn * (-_M(b) + root) / _M(a), [(abs(_M(b)) + root) / _M(a)])
    else:
        nd.put(rec, field, v)


class Control:
    """The records, masks and summaries of a group of `nnodes` nodes.  The launches take per-node sequences indexed by the
    local node; entries of nodes that are not part of the launch are never read (they may be NaN)."""

    def __init__(self, nnodes, records=None, masks=(0, 0, 0)):
        self.n = nnodes
        self.rec = [dict(r) for r in records] if records is not None else [new_record() for _ in range(nnodes)]
        self.dmask = list(masks)
        self.cg_summary = [[0.0] * CG_SUMMARY_WORDS for _ in range(nnodes)]
        self.tnt_summary = [[0.0] * TNT_SUMMARY_WORDS for _ in range(nnodes)]
        self.last = [Node() for _ in range(nnodes)]

    # ---- the start values (shared by both starts)
    def _start(self, nd, rv, Delta, target, max_it, target_exact=None, target_terms=None):
        c = new_record()
        c["pk_M_2"] = c["rv"] = rv
        c["Delta"] = Delta
        D2 = Delta * Delta
        nd.put(c, "Delta_2", D2, _M(Delta) * _M(Delta), [_M(Delta) * _M(Delta)] if math.isfinite(D2) else None)
        nd.put(c, "target", target, target_exact, target_terms)
        c["max_it"] = max_it
        return c

    def _first_test(self, nd, c):
        """the stopping test of the first step: True when the CG runs"""
        nd.took("cg_it >= max_it", c["cg_it"], c["max_it"], exact=True)
        if c["cg_it"] >= c["max_it"]:
            nd.exit = EXIT_START_LIMIT
            return False
        r = c_sqrt(c["rv"])
        nd.took("sqrt(rv) <= target", r, c["target"])
        if r <= c["target"]:
            nd.exit = EXIT_START_TARGET
            return False
        nd.exit = EXIT_LIVE
        return True

    # ---- k_cg_begin
    def begin_host(self, bits, rv, Delta, target, max_it):
        self.last = [Node() for _ in range(self.n)]
        m = 0
        for a in range(self.n):
            if not (bits >> a) & 1:
                continue
            nd = self.last[a]
            c = self._start(nd, rv[a], Delta[a], target[a], max_it)
            c["live"] = int(self._first_test(nd, c))
            if not c["live"]:
                c["h_M_norm"] = c_sqrt(c["sk_M_2"])
            self.rec[a] = c
            m |= c["live"] << a
        self.dmask = [m, m, bits & ~m]

    # ---- tnt_begin_node (k_tnt_begin, and the first half of k_cg_scal_begin)
    def begin_device(self, bits, sums, use_precon, max_it, grad_tol, pgrad_tol, kappa, theta, Delta):
        """sums[a]: |grad|^2, <X, nabla>, <X, g>, <X, g_alt>, |P grad|^2, <grad, P grad>; without a preconditioner the last
        two are not read: the summary holds zeros there"""
        self.last = [Node() for _ in range(self.n)]
        for a in range(self.n):
            bit = 1 << a
            if not (bits >> a) & 1:
                for q in range(3):
                    self.dmask[q] &= ~bit
                continue
            nd = self.last[a]
            v = [float(sums[a][q]) for q in range(4)] + ([float(sums[a][4]), float(sums[a][5])] if use_precon else [0.0, 0.0])
            gnorm = c_sqrt(v[0])
            pgnorm = c_sqrt(v[4]) if use_precon else gnorm
            rv0 = v[5] if use_precon else v[0]
            nd.took("gnorm < grad_tol", gnorm, grad_tol)
            active = not (gnorm < grad_tol)
            if active:
                nd.took("pgnorm < pgrad_tol", pgnorm, pgrad_tol)
                active = not (pgnorm < pgrad_tol)
            r0 = c_sqrt(rv0)
            if rv0 >= 0:
                pw = math.pow(r0, theta)
                target = r0 * min(kappa, pw)
                nd.took("min(kappa, r0^theta)", kappa, pw)
                t_exact = _mp.sqrt(_M(rv0)) * min(_M(kappa), _mp.power(_mp.sqrt(_M(rv0)), _M(theta)))
                c = self._start(nd, rv0, Delta[a], target, max_it, t_exact, [t_exact])
            else:
                c = self._start(nd, rv0, Delta[a], float("nan"), max_it)
            if active:
                c["live"] = int(self._first_test(nd, c))
            else:
                c["live"] = 0
                nd.exit = EXIT_INACTIVE
            if not c["live"]:
                c["h_M_norm"] = c_sqrt(c["sk_M_2"])
            self.rec[a] = c
            self.tnt_summary[a] = v + [1.0 if active else 0.0]
            if c["live"]:
                self.dmask[0] |= bit
                self.dmask[1] |= bit
                self.dmask[2] &= ~bit
            else:
                self.dmask[0] &= ~bit
                self.dmask[1] &= ~bit
                if active:
                    self.dmask[2] |= bit
                else:
                    self.dmask[2] &= ~bit

    # ---- cg_scal_logic, phase 0: the step length, the boundary / curvature / kernel exits
    def _phase0_node(self, nd, c, v):
        kappa_k, hphp, pp, pr = (float(x) for x in v)
        ratio = c_div(c_sqrt(hphp), c_sqrt(pp))
        nd.took("|Hp| / |p| < eps", ratio, KERNEL_EPS)
        stop = False
        if ratio < KERNEL_EPS:
            nd.took("<p, r> < 0", pr, 0.0, exact=True)
            sgn = 1.0
            if pr < 0:
                sgn = -1.0
                c["sk_M_pk"] = -c["sk_M_pk"]
            boundary_root(nd, c, "c1", sgn)
            nd.exit = EXIT_KERNEL
            stop = True
        else:
            nd.took("kappa_k <= 0", kappa_k, 0.0, exact=True)
            alpha = c_div(c["rv"], kappa_k)
            t1, t2 = c_mul(c_mul(2.0, alpha), c["sk_M_pk"]), c_mul(c_mul(alpha, alpha), c["pk_M_2"])
            skp1 = c["sk_M_2"] + t1 + t2
            if kappa_k <= 0:
                nd.exit = EXIT_CURVATURE
                stop = True
            else:
                nd.took("skp1 > Delta_2", skp1, c["Delta_2"])
                if skp1 > c["Delta_2"]:
                    nd.exit = EXIT_BOUNDARY
                    stop = True
            if stop:
                boundary_root(nd, c, "c1")
            else:
                am = _M(c["rv"]) / _M(kappa_k)
                for f in ("c1", "cr", "al"):
                    nd.put(c, f, alpha, am, [am])
                c["kap"] = kappa_k
                terms = [_M(c["sk_M_2"]), 2 * am * _M(c["sk_M_pk"]), am * am * _M(c["pk_M_2"])]
                nd.put(c, "sk_M_2", skp1, sum(terms), terms)
                nd.exit = EXIT_STEP
        if stop:
            c["cr"] = 0.0
            nd.bound.pop("cr", None)
            nd.exact.pop("cr", None)
            c["h_M_norm"] = c["Delta"]
            c["live"] = 0
            c["stop_ord"] = 2 * c["cg_it"] + 1

    # ---- phase 1: beta, the recurrences, the next step's stopping test
    def _phase1_node(self, nd, c, v):
        rk_vk = float(v[0])
        al, kap, b, a = c["al"], c["kap"], c["sk_M_pk"], c["pk_M_2"]
        be = c_div(rk_vk, al * kap)
        bm = _M(rk_vk) / (_M(al) * _M(kap))
        t = [bm * _M(b), bm * _M(al) * _M(a)]
        nd.put(c, "sk_M_pk", be * (b + al * a), sum(t), t)
        t = [_M(rk_vk), bm * bm * _M(a)]
        nd.put(c, "pk_M_2", rk_vk + be * be * a, sum(t), t)
        c["rv"] = rk_vk
        nd.put(c, "be", be, bm, [bm])
        c["cg_it"] += 1
        nd.took("cg_it >= max_it", c["cg_it"], c["max_it"], exact=True)
        stop = c["cg_it"] >= c["max_it"]
        nd.exit = EXIT_LIMIT if stop else EXIT_GO_ON
        if not stop:
            r = c_sqrt(c["rv"])
            nd.took("sqrt(rv) <= target", r, c["target"])
            if r <= c["target"]:
                stop = True
                nd.exit = EXIT_TARGET
        if stop:
            h = c_sqrt(c["sk_M_2"])
            hm = _mp.sqrt(_M(c["sk_M_2"])) if c["sk_M_2"] >= 0 else None
            nd.put(c, "h_M_norm", h, hm, [hm] if hm is not None else None)
            c["live"] = 0
            c["stop_ord"] = 2 * c["cg_it"]

    # ---- cg_scal_node over the nodes of dmask[phase], the summaries, and flag_arrive's hand-over
    def _scal(self, phase, sums, fresh=True):
        if fresh:
            self.last = [Node() for _ in range(self.n)]
        on = self.dmask[phase]
        for a in range(self.n):
            c = self.rec[a]
            if (on >> a) & 1:
                (self._phase0_node if phase == 0 else self._phase1_node)(self.last[a], c, sums[a])
                if not c["live"]:
                    self.dmask[1] &= ~(1 << a)
                    self.dmask[2] |= 1 << a
            self.cg_summary[a] = [CG_LIVE_ORD if c["live"] else float(c["stop_ord"]), c["h_M_norm"], float(c["cg_it"])]
        if phase == 1:
            self.dmask[0] = self.dmask[1]

    def phase0(self, sums):
        """sums[a]: <p, H p>, <H p, H p>, <p, p>, <p, r>"""
        self._scal(0, sums)

    def phase1(self, sums):
        """sums[a][0]: <r, v>"""
        self._scal(1, sums)

    # ---- k_cg_scal_begin: begin_device, then phase 0 of the nodes it left live
    def scal_begin(self, bits, start_sums, step_sums, use_precon, max_it, grad_tol, pgrad_tol, kappa, theta, Delta):
        self.begin_device(bits, start_sums, use_precon, max_it, grad_tol, pgrad_tol, kappa, theta, Delta)
        begun = self.last
        self._scal(0, step_sums)
        for a in range(self.n):   # (both halves' comparisons and bounds; a field the step wrote again keeps the step's)
            nd = self.last[a]
            nd.margins = begun[a].margins + nd.margins
            for f, b in begun[a].bound.items():
                nd.bound.setdefault(f, b)
                nd.exact.setdefault(f, begun[a].exact[f])
            if nd.exit == EXIT_NONE:
                nd.exit = begun[a].exit

    # ---- the pinned summaries
    def summaries(self):
        """(stop ordinal or CG_LIVE_ORD, h_M_norm, cg_it) per node and the seven TNT_SUMMARY words per node"""
        return [list(w) for w in self.cg_summary], [list(w) for w in self.tnt_summary]

    def min_margin(self):
        m = [(x, what, a) for a, nd in enumerate(self.last) for what, x in nd.margins]
        return min(m) if m else (math.inf, "", -1)
