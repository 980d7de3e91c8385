"""The device's Steihaug-Toint control -- k_cg_begin, k_tnt_begin, k_cg_scal, k_cg_scal_begin -- launch by launch on GIVEN partial
sums (NodeGroup.debug_cg_scalars) against tests/stpcg_restatement.py, which tests/test_stpcg_restatement_host.py pins to the
reference's recorded STPCG answers.

Every launch is compared with the restatement applied to the state the device itself left after the launch before (the first
launch of every script resets all nodes), so both sides start from the same doubles:
  decisions   live, stop_ord, cg_it, max_it, the three masks, the summaries' ordinal and `active`: exact
  scalars     within the restatement's bound (16 u sum |terms| of the expression, around its value at 120 bits); a field the
              launch does not compute is unchanged bit for bit
  summaries   the pinned words equal the device's record bit for bit
The sums are small integers times powers of two, split unevenly over a node's own segments, so every summation order gives
the same exact sum; the segments of nodes that must not be read, the neighbour segments and the unused slots hold huge
values / NaN.  Every comparison the restatement takes has a relative margin >= 1e-6 (asserted on the host below, and again
on the device's own state).

Groups: synthetic.ladder(3) -- 6 nodes of 1 to 3 own segments, different nodes taking different branches in one launch -- and a
one-node synthetic.grid(17, 17, 16): 73 own segments, a second trip of every reduction wave's k += 64 loop.
"""
import math

import numpy as np
import pytest

import stpcg_restatement as R

NAN = float("nan")
MIN_MARGIN = 1e-6
FIRST = 16          # cg_first_slot(): where k_cg_scal_begin finds the step's four sums
PRE = 6             # MAX_DOTS: the two preconditioned sums of the start sit in slots 6, 7
TOL = dict(grad_tol=2.0 ** -10, pgrad_tol=2.0 ** -8, kappa=0.05, theta=0.9)


# ---------------------------------------------------------------------------------------------------------------------
# scripts: lists of launches; a launch: kind, the by-value arguments, sums = {slot: {node: exact value}}

def _reset(L, rv=None, Delta=None, target=None, max_it=10):
    """every node live: dmask = [all, all, 0]"""
    return dict(kind="begin_host", bits=(1 << L) - 1, max_it=max_it, rv=rv or [4.0] * L, Delta=Delta or [64.0] * L,
                target=target or [2.0 ** -10] * L, sums={})


def _sums(per_node, slot0=0):
    """{node: [v0, v1, ...]} -> {slot: {node: value}}"""
    out = {}
    for a, vals in per_node.items():
        for q, v in enumerate(vals):
            out.setdefault(slot0 + q, {})[a] = v
    return out


# ---- script 1: begin_host.  roles: target reached at the start, a slightly negative rv (sqrt is NaN: live), live, outside
HOST_ROLES = ("target", "negative", "live", "outside")


def script_begin_host(roles):
    L = len(roles)
    rv = [{"target": 4.0, "negative": -2.0 ** -40, "live": 9.0, "outside": 5.0}[r] for r in roles]
    target = [{"target": 3.0, "negative": 1.0, "live": 2.0 ** -10, "outside": 7.0}[r] for r in roles]
    Delta = [3.0 + a for a in range(L)]
    bits = sum(1 << a for a, r in enumerate(roles) if r != "outside")
    return [_reset(L),
            dict(kind="begin_host", bits=bits, max_it=10, rv=rv, Delta=Delta, target=target, sums={}),
            _reset(L),
            # the iteration limit reached at the start: the smallest max_it the entry accepts
            dict(kind="begin_host", bits=bits, max_it=0, rv=rv, Delta=Delta, target=target, sums={})]


def expect_begin_host(roles, snaps):
    for a, r in enumerate(roles):
        want = {"target": R.EXIT_START_TARGET, "negative": R.EXIT_LIVE, "live": R.EXIT_LIVE, "outside": R.EXIT_NONE}[r]
        assert snaps[1]["exits"][a] == want, (a, r, snaps[1]["exits"][a])
        assert snaps[3]["exits"][a] == (R.EXIT_NONE if r == "outside" else R.EXIT_START_LIMIT)
    live = sum(1 << a for a, r in enumerate(roles) if r in ("negative", "live"))
    over = sum(1 << a for a, r in enumerate(roles) if r == "target")
    assert snaps[1]["masks"] == [live, live, over]
    assert snaps[3]["masks"] == [0, 0, sum(1 << a for a, r in enumerate(roles) if r != "outside")]


# ---- script 2: begin_device.  roles: live with target = r0 kappa / = r0 r0^theta, failing grad_tol, failing pgrad_tol only,
# outside
DEV_ROLES = ("kappa side", "power side", "small gradient", "small pgradient", "outside", "kappa side")


def _start_sums(role, use_precon):
    # |grad|^2, <X, nabla>, <X, g>, <X, g_alt> [, |P grad|^2, <grad, P grad>]
    if role == "kappa side":
        v = [9.0, 5.0, -3.0, 7.0, 16.0, 12.0]          # r0 = 3 / sqrt(12): r0^theta > kappa
    elif role == "power side":
        v = [2.0 ** -12, 5.0, -3.0, 7.0, 2.0 ** -10, 2.0 ** -14]   # r0 = 2^-6 / 2^-7: r0^theta < kappa
    elif role == "small gradient":
        v = [2.0 ** -30, 1.0, 2.0, 3.0, 4.0, 1.0]      # gnorm = 2^-15 < grad_tol
    elif role == "small pgradient":
        # with the preconditioner pgnorm = 2^-15; without it pgnorm = gnorm = 2^-9, between the two tolerances
        v = [4.0, 1.0, 2.0, 3.0, 2.0 ** -30, 1.0] if use_precon else [2.0 ** -18, 1.0, 2.0, 3.0, 4.0, 1.0]
    else:
        return None
    return v if use_precon else v[:4]


def _start_launch(kind, roles, use_precon, max_it, step=None):
    L = len(roles)
    sums = {}
    for a, r in enumerate(roles):
        v = _start_sums(r, use_precon)
        if v is None:
            continue
        for q in range(4):
            sums.setdefault(q, {})[a] = v[q]
        if use_precon:
            sums.setdefault(PRE, {})[a] = v[4]
            sums.setdefault(PRE + 1, {})[a] = v[5]
    if step:
        for slot, d in _sums(step, FIRST).items():
            sums[slot] = d
    bits = sum(1 << a for a, r in enumerate(roles) if r != "outside")
    return dict(kind=kind, bits=bits, use_precon=use_precon, max_it=max_it, Delta=[2.0 + a for a in range(L)], sums=sums, **TOL)


def script_begin_device(roles):
    L = len(roles)
    out = []
    for use_precon in (0, 1):
        out += [_reset(L), _start_launch("begin_device", roles, use_precon, 10)]
    return out + [_reset(L), _start_launch("begin_device", roles, 1, 0)]   # active, but the limit is reached at the start


def expect_begin_device(roles, snaps):
    for i in (1, 3, 5):
        for a, r in enumerate(roles):
            e = snaps[i]["exits"][a]
            if r in ("kappa side", "power side"):
                assert e == (R.EXIT_LIVE if i < 5 else R.EXIT_START_LIMIT)
                side = dict(snaps[i]["margins"][a])
                assert "min(kappa, r0^theta)" in side
            else:
                assert e == (R.EXIT_NONE if r == "outside" else R.EXIT_INACTIVE), (i, a, r, e)
        act = sum(1 << a for a, r in enumerate(roles) if r in ("kappa side", "power side"))
        assert snaps[i]["masks"] == ([act, act, 0] if i < 5 else [0, 0, act])
        for a, r in enumerate(roles):
            if r not in ("outside",):
                assert snaps[i]["tnt"][a][6] == (1.0 if r in ("kappa side", "power side") else 0.0)
    # both sides of the min were taken
    k = [a for a, r in enumerate(roles) if r == "kappa side"][:1] + [a for a, r in enumerate(roles) if r == "power side"][:1]
    if len(k) == 2:
        for i in (1, 3):
            t = [snaps[i]["records"][a]["target"] / math.sqrt(snaps[i]["records"][a]["rv"]) for a in k]
            assert abs(t[0] - TOL["kappa"]) <= 4 * R.U and t[1] < 0.5 * TOL["kappa"]


# ---- scripts 3 and 4: the steps.  A role is what the node does at each scalar launch; until then it takes plain steps:
#   step 1: kappa = 8 -> alpha = 1/2, |s|^2 = 1;  <r, v> = 1 -> beta = 1/4, sk_M_pk = 1/2, pk_M_2 = 5/4
#   step 2: kappa = 4 -> alpha = 1/4;             <r, v> = 1/4 -> beta = 1/4, sk_M_pk = 13/64, pk_M_2 = 21/64
#   step 3: kappa = 2, <r, v> = 1/16;  step 4: kappa = 1, <r, v> = 1/64
PLAIN0 = ([8.0, 16.0, 4.0, -4.0], [4.0, 9.0, 1.25, -1.0], [2.0, 3.0, 0.375, -0.25], [1.0, 2.0, 0.25, -0.0625])
PLAIN1 = ([1.0], [0.25], [0.0625], [2.0 ** -6])
STEP_ROLES = {
    # role: (the step it ends at, the phase, the sums it ends with, the exit, its radius)
    "plain": (None, None, None, None, 64.0),
    "boundary@1": (0, 0, [1.0, 16.0, 4.0, -4.0], R.EXIT_BOUNDARY, 2.0),            # alpha = 4: |s|^2 = 64 > 4, sk_M_pk = 0
    "boundary@3": (2, 0, [2.0 ** -6, 3.0, 0.375, -0.25], R.EXIT_BOUNDARY, 2.0),    # after two steps, sk_M_pk = 13/64 > 0
    "curvature@1": (0, 0, [-2.0, 16.0, 4.0, -4.0], R.EXIT_CURVATURE, 64.0),
    "curvature@2": (1, 0, [-1.0, 9.0, 1.25, -1.0], R.EXIT_CURVATURE, 64.0),
    "zero curvature@1": (0, 0, [0.0, 16.0, 4.0, -4.0], R.EXIT_CURVATURE, 64.0),
    "kernel-@1": (0, 0, [0.0, 0.0, 4.0, -4.0], R.EXIT_KERNEL, 8.0),
    "kernel+@1": (0, 0, [0.0, 0.0, 4.0, 4.0], R.EXIT_KERNEL, 8.0),
    "kernel-@3": (2, 0, [0.0, 0.0, 0.375, -0.25], R.EXIT_KERNEL, 8.0),             # sk_M_pk = 13/64 changes sign
    "kernel+@3": (2, 0, [0.0, 0.0, 0.375, 0.25], R.EXIT_KERNEL, 8.0),
    "target@1": (0, 1, [2.0 ** -22], R.EXIT_TARGET, 64.0),                         # sqrt(<r, v>) = 2^-11 <= target = 2^-10
    "target@2": (1, 1, [2.0 ** -24], R.EXIT_TARGET, 64.0),
}
STEP_SETS = (("plain", "boundary@1", "curvature@1", "zero curvature@1", "kernel-@1", "kernel+@1"),
             ("plain", "boundary@3", "kernel-@3", "kernel+@3", "curvature@2", "boundary@1"),
             ("target@2", "plain", "target@1", "curvature@2", "kernel-@3", "target@1"))


def _step_launches(roles, nsteps):
    out, live = [], set(range(len(roles)))
    for j in range(nsteps):
        for phase in (0, 1):
            per = {}
            for a in sorted(live):
                end, ph, vals, _, _ = STEP_ROLES[roles[a]]
                if end == j and ph == phase:
                    per[a] = vals
                else:
                    per[a] = (PLAIN0 if phase == 0 else PLAIN1)[j]
            out.append(dict(kind="scal%d" % phase, sums=_sums(per), ends=[a for a in per if STEP_ROLES[roles[a]][:2] == (j, phase)]))
            live -= set(out[-1]["ends"])
    return out


def script_steps(roles, max_it=10, nsteps=4):
    """scal0, scal1 pairs: three steps and a surplus pair, under which the nodes that have stopped must keep their records"""
    L = len(roles)
    return [_reset(L, Delta=[STEP_ROLES[r][4] for r in roles], max_it=max_it)] + _step_launches(roles, nsteps)


def expect_steps(roles, script, snaps, max_it=10):
    all_bits = (1 << len(roles)) - 1
    live, over = all_bits, 0
    assert snaps[0]["masks"] == [all_bits, all_bits, 0]
    for i in range(1, len(script)):
        q, s = script[i], snaps[i]
        phase = 0 if q["kind"] == "scal0" else 1
        step = (i - 1) // 2
        before = live
        for a in range(len(roles)):
            bit = 1 << a
            rec, e = s["records"][a], s["exits"][a]
            if not before & bit:
                assert e == R.EXIT_NONE and rec == snaps[i - 1]["records"][a], (i, a)   # a stopped node keeps its record
                continue
            hit_limit = phase == 1 and step + 1 >= max_it
            if a in q["ends"] or hit_limit:
                live &= ~bit
                over |= bit
                want = STEP_ROLES[roles[a]][3] if a in q["ends"] and not (hit_limit and phase == 1) else R.EXIT_LIMIT
                assert e == want, (i, a, roles[a], e)
                assert not rec["live"] and rec["cg_it"] == step + phase
                if phase == 0:
                    assert rec["cr"] == 0.0 and rec["h_M_norm"] == rec["Delta"] and rec["stop_ord"] == 2 * rec["cg_it"] + 1
                else:
                    assert rec["stop_ord"] == 2 * rec["cg_it"]
            else:
                assert e == (R.EXIT_STEP if phase == 0 else R.EXIT_GO_ON), (i, a, roles[a], e)
        # a node that stops at phase 0 leaves dmask[1], joins dmask[2] and stays in dmask[0] until phase 1 is over
        assert s["masks"] == [before if phase == 0 else live, live, over], (i, s["masks"])
        if phase == 1:
            assert s["masks"][0] == s["masks"][1]
        for a in range(len(roles)):   # the summary: the ordinal the node stopped at, or CG_LIVE_ORD
            rec = s["records"][a]
            assert s["cg"][a][0] == (R.CG_LIVE_ORD if rec["live"] else float(rec["stop_ord"]))
    # the kernel branch turns the stored sk_M_pk with <p, r> < 0
    for a, r in enumerate(roles):
        if r.startswith("kernel") and max_it > 3:
            end = STEP_ROLES[r][0]
            i = 1 + 2 * end
            b, c = snaps[i - 1]["records"][a]["sk_M_pk"], snaps[i]["records"][a]["sk_M_pk"]
            assert c == (-b if r[6] == "-" else b) and (end == 0 or b != 0.0)
            assert math.copysign(1.0, snaps[i]["records"][a]["c1"]) == (-1.0 if r[6] == "-" else 1.0)
        if r == "boundary@3" and max_it > 3:
            assert snaps[5]["records"][a]["sk_M_pk"] > 0 and snaps[5]["records"][a]["c1"] > 0


# ---- script 5: k_cg_scal_begin = begin_device, then scal0 of the nodes it left live, on the same sums
BEGIN_SETS = ((("kappa side", "power side", "small gradient", "small pgradient", "outside", "kappa side"),
               ("plain", "boundary@1", "curvature@1", "kernel-@1", "plain", "kernel+@1")),)


def _first_step_sums(start_roles, step_roles):
    """the first step's sums of every candidate: a node that fails the gradient tests has them too (its product ran for
    nothing), and they must be ignored"""
    return {a: (STEP_ROLES[s][2] if STEP_ROLES[s][0] == 0 and STEP_ROLES[s][1] == 0 else PLAIN0[0])
            for a, (r, s) in enumerate(zip(start_roles, step_roles)) if r != "outside"}


def scripts_scal_begin(start_roles, step_roles, use_precon):
    L = len(start_roles)
    step = _first_step_sums(start_roles, step_roles)
    fused = [_reset(L), _start_launch("scal_begin", start_roles, use_precon, 10, step=step)]
    live = {a: v for a, v in step.items() if start_roles[a] in ("kappa side", "power side")}
    apart = [_reset(L), _start_launch("begin_device", start_roles, use_precon, 10), dict(kind="scal0", sums=_sums(live))]
    return fused, apart


# ---------------------------------------------------------------------------------------------------------------------
# the restatement over a script, from its own state (host) or from the state the device left (GPU)

def _restate(C, q, L):
    def per_node(slots):
        return [[q["sums"].get(s, {}).get(a, NAN) for s in slots] for a in range(L)]
    k = q["kind"]
    if k == "begin_host":
        C.begin_host(q["bits"], q["rv"], q["Delta"], q["target"], q["max_it"])
    elif k in ("begin_device", "scal_begin"):
        args = (q["use_precon"], q["max_it"], q["grad_tol"], q["pgrad_tol"], q["kappa"], q["theta"], q["Delta"])
        start = per_node([0, 1, 2, 3, PRE, PRE + 1])
        if k == "begin_device":
            C.begin_device(q["bits"], start, *args)
        else:
            C.scal_begin(q["bits"], start, per_node(range(FIRST, FIRST + 4)), *args)
    elif k == "scal0":
        C.phase0(per_node(range(4)))
    else:
        C.phase1(per_node([0]))


def _snapshot(C):
    cg, tnt = C.summaries()
    return dict(records=[dict(r) for r in C.rec], masks=list(C.dmask), cg=cg, tnt=tnt, exits=[nd.exit for nd in C.last],
                margins=[list(nd.margins) for nd in C.last], nodes=C.last)


def restate_script(script, L):
    C, snaps = R.Control(L), []
    for q in script:
        _restate(C, q, L)
        snaps.append(_snapshot(C))
    return snaps


def _margins_ok(snaps):
    for i, s in enumerate(snaps):
        for a, ms in enumerate(s["margins"]):
            for what, m in ms:
                assert m >= MIN_MARGIN, (i, a, what, m)


def _same(x, y):
    return x == y or (isinstance(x, float) and isinstance(y, float) and math.isnan(x) and math.isnan(y))


# ---------------------------------------------------------------------------------------------------------------------
# host part: the scripts take the branches they are meant to take, with the margins the device test relies on

def _singles(role_names):
    return [(r,) for r in role_names]


def test_scripts_on_the_restatement():
    for roles in [HOST_ROLES + ("live", "target")] + _singles(HOST_ROLES):
        sc = script_begin_host(roles)
        snaps = restate_script(sc, len(roles))
        expect_begin_host(roles, snaps)
        _margins_ok(snaps)
    snaps = restate_script(script_begin_device(DEV_ROLES), 6)
    expect_begin_device(DEV_ROLES, snaps)
    _margins_ok(snaps)
    for roles in list(STEP_SETS) + _singles(STEP_ROLES):
        for max_it in (10, 1, 2):
            sc = script_steps(roles, max_it)
            snaps = restate_script(sc, len(roles))
            expect_steps(roles, sc, snaps, max_it)
            _margins_ok(snaps)
    for start_roles, step_roles in list(BEGIN_SETS) + [((r,), (s,)) for r in DEV_ROLES[:4] for s in ("plain", "boundary@1", "kernel-@1")]:
        for use_precon in (0, 1):
            fused, apart = scripts_scal_begin(start_roles, step_roles, use_precon)
            sf, sa = restate_script(fused, len(start_roles)), restate_script(apart, len(start_roles))
            _margins_ok(sf)
            _margins_ok(sa)
            assert sf[-1]["records"] == sa[-1]["records"] or all(
                all(_same(x[f], y[f]) for f in x) for x, y in zip(sf[-1]["records"], sa[-1]["records"]))
            assert sf[-1]["masks"] == sa[-1]["masks"] and sf[-1]["tnt"] == sa[-1]["tnt"]


def test_partial_tables_sum_exactly_in_any_order():
    rng = np.random.default_rng(5)
    for nseg in (1, 2, 3, 73):
        for v in (9.0, -2.0 ** -40, 2.0 ** -30, 0.375, 0.0, 13.0 / 64):
            parts = _split(v, nseg)
            assert len(parts) == nseg and (nseg == 1 or len(set(parts)) > 1 or v == 0.0)
            for _ in range(5):
                p = rng.permutation(parts)
                assert float(np.sum(p)) == v and math.fsum(p) == v and float(np.cumsum(p)[-1]) == v
            lanes = [sum(parts[k::64]) for k in range(min(64, nseg))]   # the reduction wave's own order
            assert sum(lanes) == v


# ---------------------------------------------------------------------------------------------------------------------
# the partial-sum tables

WEIGHTS = (3, -1, 5, 1, -2, 2, -3, 4, -5, 7)   # eighths of the sum, cyclically; the last segment takes the rest


def _split(v, nseg):
    """v as nseg pieces, multiples of v / 8 with small integer factors: exact under every summation order"""
    if nseg == 1:
        return [v]
    w = [WEIGHTS[j % len(WEIGHTS)] for j in range(nseg - 1)]
    w.append(8 - sum(w))
    return [v * (m / 8.0) for m in w]


def _table(layout, q):
    nseg_all, own, _ = layout
    if not q["sums"]:
        return None
    nslots = max(q["sums"]) + 1
    T = np.full((nslots, nseg_all), NAN)
    for slot, per in q["sums"].items():
        # what must not be read: the neighbour segments, and the own segments of the nodes that are not part of the launch
        T[slot] = [(-1.0) ** k * 3.0e200 for k in range(nseg_all)]
        for a, v in per.items():
            T[slot, own[a]:own[a + 1]] = _split(v, own[a + 1] - own[a])
    return T


# ---------------------------------------------------------------------------------------------------------------------
# GPU part

def _measurements_graph(g, nn):
    import dpgo_amd
    return dpgo_amd.graph_from_edges(g["d"], g["num_poses"], g["I"], g["J"], g["R"], g["t"], g["kappa"], g["tau"], nn)


@pytest.fixture(scope="module")
def ladder_group():
    import dpgo_amd
    from dpgo_amd import synthetic
    g = synthetic.ladder(3)
    grp = dpgo_amd.NodeGroup(_measurements_graph(g, g["num_nodes"]), range(g["num_nodes"]), dpgo_amd.Options.driver(0, True))
    layout = grp.debug_seg_layout()
    assert sorted(set(np.diff(layout[1]))) == [1, 2, 3] and len(layout[1]) == 7
    return grp, layout


@pytest.fixture(scope="module")
def wide_group():
    import dpgo_amd
    from dpgo_amd import synthetic
    g = synthetic.grid(17, 17, 16)
    grp = dpgo_amd.NodeGroup(_measurements_graph(g, 1), [0], dpgo_amd.Options.driver(0, True))
    layout = grp.debug_seg_layout()
    assert list(np.diff(layout[1])) == [73]
    return grp, layout


def run_on_device(group, script):
    """The script on the device, every launch against the restatement applied to the device's own state before it.
    Returns (the device's outputs, the restatement's snapshots)."""
    grp, layout = group
    L = len(layout[1]) - 1
    assert script[0]["kind"] == "begin_host" and script[0]["bits"] == (1 << L) - 1
    launches = []
    for q in script:
        d = {k: v for k, v in q.items() if k not in ("sums", "ends")}
        d["partials"] = _table(layout, q)
        launches.append(d)
    dev = grp.debug_cg_scalars(launches)
    snaps, prev = [], None
    for i, (q, o) in enumerate(zip(script, dev)):
        C = R.Control(L) if prev is None else R.Control(L, prev["records"], prev["masks"])
        if prev is not None:
            C.cg_summary = [list(w) for w in prev["cg_summary"]]
            C.tnt_summary = [list(w) for w in prev["tnt_summary"]]
        _restate(C, q, L)
        s = _snapshot(C)
        snaps.append(s)
        _margins_ok([s])
        # ---- decisions: exact
        assert o["masks"] == s["masks"], (i, q["kind"], o["masks"], s["masks"])
        for a in range(L):
            got, want, nd = o["records"][a], s["records"][a], s["nodes"][a]
            for f in R.INT_FIELDS:
                assert got[f] == want[f], (i, q["kind"], a, f, got[f], want[f])
            # ---- scalars: within the bound where the launch computed them, untouched bit for bit where it did not
            for f in R.FIELDS:
                if f in nd.bound:
                    err = abs(got[f] - float(nd.exact[f]))
                    assert err <= nd.bound[f], (i, q["kind"], a, f, got[f], float(nd.exact[f]), err, nd.bound[f])
                else:
                    assert _same(got[f], want[f]), (i, q["kind"], a, f, got[f], want[f])
        # ---- the pinned summaries: the restatement's decisions, and the device's own record bit for bit
        wrote_cg = q["kind"] in ("scal0", "scal1", "scal_begin")
        for a in range(L):
            rec, w = o["records"][a], o["cg_summary"][a]
            if wrote_cg:
                assert w[0] == s["cg"][a][0] == (R.CG_LIVE_ORD if rec["live"] else float(rec["stop_ord"])), (i, a, w)
                assert w[2] == s["cg"][a][2] == float(rec["cg_it"]), (i, a, w)
                assert _same(float(w[1]), rec["h_M_norm"]), (i, a, w, rec["h_M_norm"])
            elif prev is not None:
                assert all(_same(float(x), float(y)) for x, y in zip(w, prev["cg_summary"][a])), (i, a)
            if prev is not None or (q["kind"] != "begin_host" and (q["bits"] >> a) & 1):
                # the six sums are exact, `active` is a decision
                assert all(_same(float(x), float(y)) for x, y in zip(o["tnt_summary"][a], s["tnt"][a])), (i, a, o["tnt_summary"][a], s["tnt"][a])
        if q["kind"] == "scal_begin":
            for a in range(L):
                if (q["bits"] >> a) & 1:
                    assert np.array_equal(o["dev_tnt"][a], o["tnt_summary"][a]), (i, a)
        # ---- the flag: raised by the launches that have one, to the next sequence value; the arrival counter is back at 0
        assert o["arrived"] == 0 and o["flag"] == o["seq"]
        if i > 0:
            assert o["seq"] == dev[i - 1]["seq"] + (1 if wrote_cg else 0)
        prev = o
    return dev, snaps


@pytest.mark.gpu
def test_begin_host(ladder_group):
    roles = HOST_ROLES + ("live", "target")
    dev, snaps = run_on_device(ladder_group, script_begin_host(roles))
    expect_begin_host(roles, snaps)
    out = roles.index("outside")
    for i in (1, 3):   # a node outside `bits`: its record untouched, its bit cleared in all three masks
        assert all(_same(dev[i]["records"][out][f], dev[i - 1]["records"][out][f]) for f in R.FIELDS + R.INT_FIELDS)
        assert not any((m >> out) & 1 for m in dev[i]["masks"]) and (dev[i - 1]["masks"][0] >> out) & 1
    neg = roles.index("negative")
    assert dev[1]["records"][neg]["live"] == 1 and dev[1]["records"][neg]["rv"] < 0


@pytest.mark.gpu
def test_begin_device(ladder_group):
    dev, snaps = run_on_device(ladder_group, script_begin_device(DEV_ROLES))
    expect_begin_device(DEV_ROLES, snaps)
    for i in (1, 3, 5):
        for a, r in enumerate(DEV_ROLES):
            if r in ("small gradient", "small pgradient"):   # active = 0: out of every mask, dmask[2] included
                assert dev[i]["tnt_summary"][a][6] == 0.0 and not any((m >> a) & 1 for m in dev[i]["masks"])
        # without the preconditioner the two preconditioned sums are not read (their slots hold NaN): zeros in the summary
        if i == 1:
            assert all(dev[i]["tnt_summary"][a][4] == 0.0 and dev[i]["tnt_summary"][a][5] == 0.0
                       for a, r in enumerate(DEV_ROLES) if r != "outside")


@pytest.mark.gpu
@pytest.mark.parametrize("roles", STEP_SETS, ids=["first step", "later steps", "targets"])
@pytest.mark.parametrize("max_it", [10, 2, 1])
def test_steps(ladder_group, roles, max_it):
    sc = script_steps(roles, max_it)
    dev, snaps = run_on_device(ladder_group, sc)
    expect_steps(roles, sc, snaps, max_it)
    # the surplus pair at the end: every node that has stopped keeps its record and its summary, bit for bit
    for a in range(len(roles)):
        if not dev[-3]["records"][a]["live"]:
            assert all(_same(dev[-1]["records"][a][f], dev[-3]["records"][a][f]) for f in R.FIELDS + R.INT_FIELDS)
            assert np.array_equal(dev[-1]["cg_summary"][a], dev[-3]["cg_summary"][a])


def _assert_same_state(x, y, L, what):
    for a in range(L):
        for f in R.FIELDS + R.INT_FIELDS:
            assert _same(x["records"][a][f], y["records"][a][f]), (what, a, f, x["records"][a][f], y["records"][a][f])
    assert x["masks"] == y["masks"], what
    for k in ("cg_summary", "tnt_summary"):
        assert np.array_equal(x[k], y[k], equal_nan=True), (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("use_precon", [0, 1])
def test_scal_begin_is_begin_device_then_scal0(ladder_group, use_precon):
    start_roles, step_roles = BEGIN_SETS[0]
    fused, apart = scripts_scal_begin(start_roles, step_roles, use_precon)
    df, sf = run_on_device(ladder_group, fused)
    da, _ = run_on_device(ladder_group, apart)
    _assert_same_state(df[-1], da[-1], len(start_roles), "scal_begin")
    for a, r in enumerate(start_roles):
        if r in ("small gradient", "small pgradient"):   # its first-step sums were there, and were ignored
            assert FIRST in fused[1]["sums"] and a in fused[1]["sums"][FIRST]
            assert sf[-1]["exits"][a] == R.EXIT_INACTIVE and df[-1]["records"][a]["c1"] == 0.0 and df[-1]["records"][a]["stop_ord"] == 0
    took = {sf[-1]["exits"][a] for a in range(len(start_roles))}
    assert {R.EXIT_STEP, R.EXIT_BOUNDARY, R.EXIT_KERNEL, R.EXIT_INACTIVE, R.EXIT_NONE} <= took


@pytest.mark.gpu
def test_wide_node(wide_group):
    """Scripts 1, 3, 4 and 5 on a node of 73 own segments, one branch after the other."""
    for r in HOST_ROLES:
        dev, snaps = run_on_device(wide_group, script_begin_host((r,)))
        expect_begin_host((r,), snaps)
    for r in STEP_ROLES:
        for max_it in (10, 1):
            sc = script_steps((r,), max_it)
            dev, snaps = run_on_device(wide_group, sc)
            expect_steps((r,), sc, snaps, max_it)
    for r in DEV_ROLES[:4]:
        for s in ("plain", "boundary@1", "kernel-@1"):
            for use_precon in (0, 1):
                fused, apart = scripts_scal_begin((r,), (s,), use_precon)
                df, _ = run_on_device(wide_group, fused)
                da, _ = run_on_device(wide_group, apart)
                _assert_same_state(df[-1], da[-1], 1, (r, s, use_precon))


@pytest.mark.gpu
def test_flag_sequence(ladder_group):
    """Five flag-raising launches in a row raise the flag to five consecutive values and leave the arrival counter at 0 -- a
    sixth launch completes."""
    sc = script_steps(STEP_SETS[0], 10, nsteps=3)
    assert [q["kind"] for q in sc[1:]] == ["scal0", "scal1"] * 3
    dev, _ = run_on_device(ladder_group, sc)
    flags = [o["flag"] for o in dev[1:]]
    assert flags[:5] == list(range(flags[0], flags[0] + 5)) and flags[5] == flags[0] + 5
    assert all(o["arrived"] == 0 for o in dev)
