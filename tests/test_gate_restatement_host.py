"""tests/gate_restatement.py against the oracle (oracle/hash.py: amm_pgo, oracle/tnt.py: tnt, both pinned to the reference):
the restated conjuncts, evaluated on the oracle's own scalars, reproduce what the oracle DID in every iteration of every node
-- whether its first trust-region step was accepted, whether another trust-region iteration began behind it, whether it
redid the half step, restarted, fell back -- on smallGrid3D in 2 nodes under the driver's options and under three sets that force one branch each.

The oracle is watched from outside: its calls of proximal, evaluate_G and tnt are recorded (the order tells the branches
apart), and the first trust-region iteration's vectors give the sums the gate reads.  The oracle evaluates the surrogate by
its own formula, so the restated scalars agree with its own to rounding only: every comparison the restatement takes must
have a relative margin above MARGIN, which is asserted -- none of these runs decides anything within 1e-9 of a threshold.
"""
import os

import numpy as np
import pytest

import gate_restatement as GR
from oracle import g2o as og
from oracle import hash as ohash
from oracle.hash import Options
from oracle.problem import LOSS_HUBER
from oracle.star import DistPGO, chordal_initialization

MARGIN = 1e-9
STEPS = 24
FORCED = {"defaults": {}, "psi": dict(psi=1e12), "phi": dict(phi=1e3),
          "second iteration": dict(max_iterations=2, max_iterations_accepted=2, rel_func_decrease_tol=0.0, stepsize_tol=0.0)}


class Watch:
    """one node's amm_pgo under observation"""

    def __init__(self, nd):
        self.nd, self.events, self.in_tnt, self.tnts = nd, [], False, []
        p = nd.problem
        self._prox, self._evalG, self._tnt = p.proximal, p.evaluate_G, nd._tnt
        p.proximal = self.proximal
        p.evaluate_G = self.evaluate_G
        nd._tnt = self.tnt

    def proximal(self, *a):
        out = self._prox(*a)
        self.events.append(("P", out))
        return out

    def evaluate_G(self, *a):
        out = self._evalG(*a)
        if not self.in_tnt:
            self.events.append(("G", out))
        return out

    def tnt(self, x0, g):
        rec = dict(x0=x0, g=g, log=[], steps=[], status="")
        real = ohash.tnt_mod.tnt

        def spy(f, QM, metric, retract, x, precon, prm):
            state = {}

            def QM2(y):
                grad, Hess = QM(y)
                state.setdefault("grad", grad)
                state.setdefault("Hess", Hess)
                return grad, Hess

            def retract2(y, h):
                out = retract(y, h)
                if not rec["steps"]:
                    rec["steps"].append(dict(h=h, x_prop=out, fx=f(y), fx_prop=f(out), t0=metric(y, h, h), t1=metric(y, state["grad"], h),
                                             t2=metric(y, h, state["Hess"](y, h))))
                return out
            return real(f, QM2, metric, retract2, x, precon, prm, log=rec["log"])

        ohash.tnt_mod.tnt, self.in_tnt = spy, True
        try:
            out = self._tnt(x0, g)
            rec["status"] = out["status"]
        finally:
            ohash.tnt_mod.tnt, self.in_tnt = real, False
        self.events.append(("T", rec))
        self.tnts.append(rec)
        return out

    def iterate(self):
        """-> None (not refined), or (the restated Verdict, what the oracle did)"""
        r, o, p = self.nd.results, self.nd.options, self.nd.problem
        before = dict(f=r.f, Fk0=r.Fk[0], Fk1=r.Fk[1], fobj=r.fobj[0], hits0=r.soft_restart_hits[0], hits1=r.soft_restart_hits[1])
        Xak, g0 = r.Xak.copy(), r.g[0]
        self.events, self.tnts = [], []
        assert self.nd.iterate() == 0
        kinds = "".join(k for k, _ in self.events)
        if not r.refined:
            return None
        assert kinds.startswith("PGTG"), kinds
        rest = kinds[4:]
        did = dict(redo=rest.startswith("PG"))
        rest = rest[2:] if did["redo"] else rest
        did["restart"] = rest.startswith("T") or rest.startswith("PT")
        rest = rest[(1 if rest.startswith("T") else 2):] if did["restart"] else rest
        did["fall_back"] = rest == "G"
        assert rest in ("", "G"), kinds
        first = self.tnts[0]
        did["tnt_iterations"] = len(first["log"])
        did["accepted"] = [e["accepted"] for e in first["log"]]
        # a further trust-region iteration began behind the first: it took a step of its own, or its gradient test ended it at
        # once (TNT.h:477-484; "IterationLimit" is the loop's condition failing, TNT.h:446-449)
        did["another"] = len(first["log"]) >= 2 or (len(first["log"]) == 1 and first["status"] in ("Gradient", "PreconditionedGradient"))
        f = before["f"]
        Xakh, Gkh = self.events[0][1], self.events[1][1]
        t, b = [0.0] * 16, [0.0] * 8
        b[6] = 1.0 if first["log"] else 0.0
        if first["steps"]:
            s = first["steps"][0]
            x0, xp, g = first["x0"], s["x_prop"], first["g"]
            b[2] = float(np.sum(x0 * g))
            b[1] = 2.0 * (s["fx"] - f) - b[2]
            t[0], t[1], t[2] = s["t0"], s["t1"], s["t2"]
            t[3], t[4] = float(np.sum(xp * g)), float(np.sum(xp * g0))
            t[5] = 2.0 * (s["fx_prop"] - f) - t[3]
        t[GR.DS] = float(np.sum((Xakh - Xak) ** 2))
        t[GR.DS + 1] = Gkh - f
        opt = dict(max_it=o.max_iterations, max_acc=o.max_iterations_accepted, max_hits0=o.max_soft_restart_hits[0],
                   max_hits1=o.max_soft_restart_hits[1], rel_tol=o.rel_func_decrease_tol, step_tol=o.stepsize_tol, psi=o.psi, phi=o.phi)
        return GR.gate_node(t, b, False, opt=opt, **before), did


def _margin_ok(v, skip=()):
    for what, lhs, op, rhs, _ in v.comparisons:
        if what in skip or isinstance(lhs, int):
            continue
        scale = max(abs(lhs), abs(rhs))
        assert scale == 0.0 or not np.isfinite(scale) or abs(lhs - rhs) > MARGIN * scale, (what, lhs, rhs)


@pytest.fixture(scope="module")
def runs(fixtures_dir):
    path = os.path.join(fixtures_dir, "smallGrid3D.g2o")
    num_poses, mm = og.read_g2o_file(path)
    X0 = chordal_initialization(num_poses, mm)
    out = {}
    for tag, kw in FORCED.items():
        o = Options.driver(LOSS_HUBER, True)
        for k, v in kw.items():
            setattr(o, k, v)
        drv = DistPGO(path, 2, o, X0=X0, mm=mm, num_poses=num_poses)
        watches = [Watch(nd) for nd in drv.nodes]
        rows = []
        for _ in range(STEPS):
            rows.append([w.iterate() for w in watches])
            for nd in drv.nodes:
                nd.communicate(drv.nodes)
            for nd in drv.nodes:
                nd.update()
        out[tag] = rows
    return out


@pytest.mark.parametrize("tag", sorted(FORCED))
def test_the_restated_conjuncts_are_what_the_oracle_did(runs, tag):
    refined = 0
    for row in runs[tag]:
        for got in row:
            if got is None:
                continue
            refined += 1
            v, did = got
            c = v.conjuncts
            assert c["cg_over"]
            assert c["active"] == (did["tnt_iterations"] >= 1)
            if not c["active"]:
                continue
            _margin_ok(v, skip=() if not (did["redo"] or did["restart"]) else ("Fk0 - Gk < phi (Fk0 - Gkh)",))
            assert c["accepted"] == did["accepted"][0], (v.values, did)
            if c["accepted"]:
                assert c["ends"] == (not did["another"]), (v.values, did)
            assert c["no_redo"] == (not did["redo"]), (v.values, did)
            assert (c["no_hard_restart"] and c["no_soft_restart0"] and c["no_soft_restart1"]) == (not did["restart"]), (v.values, did)
            if not did["redo"] and not did["restart"]:     # (else the oracle falls back on the redone Gkh / the restarted Gk)
                assert c["no_fall_back"] == (not did["fall_back"]), (v.values, did)
            # the verdict: the common course is one accepted, final trust-region iteration and nothing after it
            common = (did["accepted"][0] and not did["another"] and not did["redo"] and not did["restart"]
                      and not did["fall_back"])
            assert v.common == common, (v.conjuncts, did)
    assert refined >= STEPS       # (the early regime: the nodes are refined)


def test_both_verdicts_occur_and_every_forcing_set_forces_its_branch(runs):
    def verdicts(tag):
        return [got[0].common for row in runs[tag] for got in row if got is not None]

    def active(tag):
        return [got for row in runs[tag] for got in row if got is not None and got[0].conjuncts["active"]]
    assert any(verdicts("defaults")) and not all(v for t in FORCED for v in verdicts(t))
    assert not any(verdicts("psi")) and all(did["redo"] for _, did in active("psi"))
    assert not any(verdicts("phi")) and all(did["fall_back"] or did["redo"] or did["restart"] for _, did in active("phi"))
    assert not any(verdicts("second iteration"))
    assert all(did["another"] for _, did in active("second iteration") if did["accepted"][0])
    assert any(did["tnt_iterations"] == 2 for _, did in active("second iteration"))
