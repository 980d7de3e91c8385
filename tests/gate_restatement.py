"""The verdict of one node in the gate of a speculative update, restated from the reference: does the AMM-PGO# iteration of
this node take its COMMON course?

  acceptance and stopping    Optimization/Riemannian/TNT.h:446-449, 513-575 (one trust-region iteration: the predicted and the
                             actual decrease, the gain ratio, the acceptance test, the two stopping tests behind an accepted
                             step, the loop's two iteration limits)
  redo, restarts, fall-back  DPGO/src/DPGOHash.cpp:366-367, 386-400, 434 (oracle/hash.py:302-334 is its Python form)

in the terms the device has them in:

  t[0..15]  the trial point's sums: |h|^2, <grad, h>, <h, Hess h>, <X+, g>, <X+, g[k]>, <X+, nabla(X+)>; from slot DS = 12 on
            the half step's parked ones, |Xakh - Xak|^2 and G(Xakh | g[k]) - f
  b[0..7]   the refinement's start: |grad|^2, <X, nabla(X)>, <X, g>, <X, g[k]>, two preconditioned sums, `active`
  live      the CG record's flag: the truncated CG has not ended yet
  f, Fk0, Fk1, fobj, hits0, hits1   the node's scalars of the last update()
  opt       max_it, max_acc (TNT's iteration limits), rel_tol, step_tol, psi, phi, max_hits0, max_hits1

The surrogate at a point is G(X | g, f) = f + <X, g> + 1/2 <X, G X> = 1/2 (<X, nabla> + <X, g>) + f with nabla = G X + g.

Plain Python floats: IEEE doubles, every product and every sum rounded on its own (no fused multiply-add), the operands in the
order the reference's expressions have them.  Returns the verdict, the nine conjuncts, and every comparison taken with both
operands (tests/stpcg_restatement.py does the same for its margins).

contract (tests only): ONE expression evaluated the way a compiler that contracts a product and the sum behind it would --
the exact product, one rounding (fractions.Fraction) -- to show that an input tells the two evaluations apart:
"fx", "fx_prop" (0.5 (..) + f), "dm" (-t1 - 0.5 t2), "minG" (Fk0 - psi t[DS]), "fall" (the product phi (Fk0 - Gkh) not rounded
before it is compared).
"""
import math
from collections import namedtuple
from fractions import Fraction

DS = 12                                  # the half step's parked sums
ETA1 = 0.05                              # TNTParams::eta1 (TNT.h:85)
SQRT_EPS = math.sqrt(2.0 ** -52)         # TNT.h:323: sqrt(numeric_limits<Scalar>::epsilon())
CONJUNCTS = ("active", "cg_over", "accepted", "ends", "no_redo", "no_hard_restart", "no_soft_restart0", "no_soft_restart1",
             "no_fall_back")
OPTIONS = ("max_it", "max_acc", "max_hits0", "max_hits1", "rel_tol", "step_tol", "psi", "phi")

Verdict = namedtuple("Verdict", "common conjuncts comparisons values")


def _div(a, b):
    """IEEE division: x / 0 is +-inf or NaN, never an exception"""
    if b == 0.0:
        if a == 0.0 or math.isnan(a):
            return float("nan")
        return math.copysign(float("inf"), a) * math.copysign(1.0, b)
    return a / b


def _sqrt(x):
    return math.sqrt(x) if x >= 0 else float("nan")


def fma(a, b, c):
    """a b + c with one rounding (finite operands)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def gate_node(t, b, live, f, Fk0, Fk1, fobj, hits0, hits1, opt, contract=None):
    t, b = [float(x) for x in t], [float(x) for x in b]
    cmp = []

    def took(what, lhs, op, rhs):
        r = {">": lhs > rhs, "<": lhs < rhs, ">=": lhs >= rhs}[op]
        cmp.append((what, lhs, op, rhs, r))
        return r

    # ---- the trust-region iteration (TNT.h:513-575)
    fx = 0.5 * (b[1] + b[2]) + f                       # f(x): the surrogate at the refinement's start
    fx_prop = 0.5 * (t[5] + t[3]) + f                  # f(x_proposed)
    h_norm = _sqrt(t[0])
    dm = -t[1] - 0.5 * t[2]                            # :514-515
    if contract == "fx":
        fx = fma(0.5, b[1] + b[2], f)
    if contract == "fx_prop":
        fx_prop = fma(0.5, t[5] + t[3], f)
    if contract == "dm":
        dm = fma(-0.5, t[2], -t[1])
    df = fx - fx_prop                                  # :518
    rel_dec = _div(df, SQRT_EPS + abs(fx))             # :521
    rho = _div(df, dm)                                 # :524
    accepted = (not math.isnan(rho)) and took("rho > eta1", rho, ">", ETA1)          # :535
    # behind an accepted step (:565-574); `or` as the reference's two `break`s: the second test is only taken after the first
    stop_rel = took("rel_dec < rel_tol", rel_dec, "<", opt["rel_tol"])
    stop_step = (not stop_rel) and took("h_norm < step_tol", h_norm, "<", opt["step_tol"])
    # the loop goes on while iteration < max_iterations && iteration_accepted < max_iterations_accepted (:446-449): after one
    # accepted iteration both counters are 1
    another = 1 < opt["max_it"] and 1 < opt["max_acc"]
    ends = stop_rel or stop_step or not another
    # ---- DPGOHash.cpp:366-367, 383-400, 434
    Gk = fx_prop - t[3] + t[4]                         # G(X+ | g[k], f): only the linear term depends on g
    Gkh = t[DS + 1] + f
    minG = Fk0 - opt["psi"] * t[DS]
    if contract == "minG":
        minG = fma(-opt["psi"], t[DS], Fk0)
    redo = took("Gkh > minG", Gkh, ">", minG)
    hard = took("Gk > Fk0", Gk, ">", Fk0)
    soft0 = took("Gk > Fk1", Gk, ">", Fk1) and took("hits0 >= max_hits0", hits0, ">=", opt["max_hits0"])
    soft1 = took("Gk > fobj", Gk, ">", fobj) and took("hits1 > max_hits1", hits1, ">", opt["max_hits1"])
    fall = took("Fk0 - Gk < phi (Fk0 - Gkh)", Fk0 - Gk, "<", opt["phi"] * (Fk0 - Gkh))
    if contract == "fall":
        fall = Fraction(Fk0 - Gk) < Fraction(opt["phi"]) * Fraction(Fk0 - Gkh)
    c = dict(active=b[6] != 0.0, cg_over=not live, accepted=accepted, ends=ends, no_redo=not redo, no_hard_restart=not hard,
             no_soft_restart0=not soft0, no_soft_restart1=not soft1, no_fall_back=not fall)
    values = dict(fx=fx, fx_prop=fx_prop, h_norm=h_norm, dm=dm, df=df, rel_dec=rel_dec, rho=rho, Gk=Gk, Gkh=Gkh, minG=minG,
                  fall_lhs=Fk0 - Gk, fall_rhs=opt["phi"] * (Fk0 - Gkh),
                  stop_rel=stop_rel, stop_step=stop_step, another=another)
    return Verdict(all(c[k] for k in CONJUNCTS), c, cmp, values)


def gate_group(nodes):
    """the group's word: all ones if every node takes the common course, else 0 (nodes: the Verdicts)"""
    return 0xFFFFFFFFFFFFFFFF if all(v.common for v in nodes) else 0
