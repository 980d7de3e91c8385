"""A per-edge, per-pose restatement of the robust inter-edge pass (k_inter), the objective (k_cost) and the Dynamic rescale
(k_rescale_decide / k_rescale_apply), in extended precision, with the forward rounding bounds of the device's fp64
evaluation beside every quantity.  Not the oracle's sparse products: every edge and every pose is written out.

Layout.  Reference layout of a node: Z = [t_own (n0) ; R_own^T blocks (d n0) ; t_nbr (n1) ; R_nbr^T blocks (d n1)], d columns.
Here a point is (T, Y): T[p] the translation (a row), Y[p] the d x d block of pose p = 0 .. n0 + n1 - 1 (own poses first).
An edge e = (i, j, R, t, tau, kappa) has the residuals
    u_e = T_i - T_j + t^T Y_i  (d),    W_e = R^T Y_i - Y_j  (d x d),    s_e = tau |u_e|^2 + kappa |W_e|_F^2.

Bounds (u = 2^-53, gamma_k = k u / (1 - k u)); each counts the roundings of the device's statement of the operation:
  u_c:     one subtraction and d fused multiply-adds: d + 1 roundings of a sum of d + 2 terms: gamma_{d+2} sum |terms|
  W_rc:    d fused multiply-adds on -Y_j: d roundings, d + 1 terms: gamma_{d+1} sum |terms|
  s:       delta_s = sum c (2 |r| delta_r + delta_r^2) over the d + d^2 residual entries r with weight c, plus per term one
           product (c r) and one fused multiply-add, accumulated over n = d + d^2 terms: gamma_{n+2} (s + that)
  w, rho:  w is non-increasing and rho non-decreasing in s for every loss: [s - delta_s, s + delta_s] is mapped through the
           reference's own w and rho at its end points (valid across the Huber kink); plus the function's own roundings:
           Huber w = sqrt(dl) / sqrt(max(s, dl)): two square roots and a division, 3 u w; rho = min(2 sqrt(dl) sqrt(s) - dl, s):
           the two roots, the product and the subtraction, 4 u (2 sqrt(dl) sqrt(s) + dl) -- the cancellation near s = dl
           Geman-McClure w = dl^2 / (s + dl)^2: sum, two products, division, the sum's rounding twice: 5 u w; rho = dl (s / q): 3 u rho
           Welsch w = exp(-s / dl): the quotient's rounding through exp, (s / dl) u, and exp itself within one ulp (2 u):
           (s / dl + 2) u w, plus the smallest subnormal where fp64 underflows and the reference does not;
           rho = dl - dl w: dl delta_w + u dl w + u rho
  vectors: per incidence term w a: delta_w |a| + w delta_a, delta_a from the residual bounds through the coefficients plus the
           coefficient products' own roundings (d + 2 per rotation entry of a tail term, 2 otherwise); the accumulation over the
           k incidences of the pose, gamma_{k+2} sum |w a|
  g:       DfE's bound, plus the D block product: D is itself a sum of k + 1 terms assembled in fp64 (gamma_{k+2} sum |terms|),
           the product has d + 1 terms per entry (gamma_{d+2} |D| |z|), plus the subtraction (u |g|)
  sums:    the per-term bounds summed, plus n u sum |terms| for a reduction of n terms in any order
  blocks:  an entry of a block-diagonal term is a sum of k products of up to four factors: gamma_{k+4} sum |terms|
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "the restatement needs an extended-precision long double"
U = 2.0 ** -53
TINY = 2.0 ** -1074
LOSS_NONE, LOSS_HUBER, LOSS_GM, LOSS_WELSCH = 0, 1, 2, 3

MUTANTS = (
    "head_as_tail",          # one head incidence treated as tail
    "R_for_RT",              # R_e used for R_e^T
    "tau_kappa",             # tau and kappa exchanged
    "hub_last_skipped",      # the last incidence of the hub pose skipped
    "huber_rho_no_min",      # Huber's rho without the min
    "gm_w_not_squared",      # Geman-McClure's weight not squared
    "no_Dz",                 # D z left out of g
    "quad_no_half",          # the 1/2 of the quad term left out
    "Q_own_only",            # Q missing on neighbour rows
    "lazy_from_Znbr",        # a neighbour row taken from Znbr where nsrc >= 0
    "gamma_other_node",      # gamma of the wrong node used for a neighbour row
    "Xref_R_kept",           # Xref's rotations not replaced
    "clamp_0.1",             # a new scale clamped at 0.1 in place of 0.01
    "rescale_ge",            # w >= scale for w > scale in the rescale test
    "ttT_on_head",           # the t t^T term put on the head end
)


def gam(k):
    return k * U / (1.0 - k * U)


def _abs(x):
    return np.abs(x)


class Edges:
    """The measurements of one kind (inter / intra) of a node, endpoints as pose indices of the node's (T, Y)."""

    def __init__(self, info, meas, d):
        m = len(meas)
        n0 = info.n[0]
        self.m, self.d = m, d
        self.i = np.empty(m, np.int64)
        self.j = np.empty(m, np.int64)
        for e in range(m):
            bi, ki = info.index[int(meas.inode[e])][int(meas.ipose[e])]
            bj, kj = info.index[int(meas.jnode[e])][int(meas.jpose[e])]
            self.i[e] = ki + (n0 if bi else 0)
            self.j[e] = kj + (n0 if bj else 0)
        self.R = np.asarray(meas.R, LD).reshape(m, d, d)
        self.t = np.asarray(meas.t, LD).reshape(m, d)
        self.tau = np.asarray(meas.tau, LD)
        self.kappa = np.asarray(meas.kappa, LD)

    def take(self, idx):
        o = object.__new__(Edges)
        o.m, o.d = len(idx), self.d
        for k in ("i", "j", "R", "t", "tau", "kappa"):
            setattr(o, k, getattr(self, k)[idx])
        return o


def poses(Z, n0, n1, d):
    """Reference layout -> (T, Y) in extended precision."""
    Z = np.asarray(Z, LD)
    o = (d + 1) * n0
    assert Z.shape == ((d + 1) * (n0 + n1), d), Z.shape
    T = np.vstack([Z[:n0], Z[o:o + n1]])
    Y = np.concatenate([Z[n0:o].reshape(n0, d, d), Z[o + n1:].reshape(n1, d, d)])
    return T, Y


def stack(T, Y, n0, n1):
    d = T.shape[1]
    return np.vstack([T[:n0], Y[:n0].reshape(n0 * d, d), T[n0:n0 + n1], Y[n0:n0 + n1].reshape(n1 * d, d)])


def loss_fn(loss, dl, s, mut=None):
    """(w, rho) of the squared residual s (DPGOProblem.cpp:647-675), in the precision of s."""
    dl = s.dtype.type(dl)
    if loss == LOSS_HUBER:
        rs = np.sqrt(np.maximum(s, dl))
        w = np.sqrt(dl) / rs
        lin = 2 * np.sqrt(dl) * rs - dl
        return w, (lin if mut == "huber_rho_no_min" else np.minimum(lin, s))
    if loss == LOSS_GM:
        q = s + dl
        w = dl * dl / (q * q)
        return (dl / q if mut == "gm_w_not_squared" else w), dl * (s / q)
    if loss == LOSS_WELSCH:
        w = np.exp(-s / dl)
        return w, dl - dl * w
    return np.ones_like(s), s.copy()


def loss_bounds(loss, dl, s, ds):
    """(delta_w, delta_rho): the interval [s - ds, s + ds] through the reference's own functions, plus their roundings."""
    w, rho = loss_fn(loss, dl, s)
    w_lo, rho_hi = loss_fn(loss, dl, s + ds)
    w_hi, rho_lo = loss_fn(loss, dl, np.maximum(s - ds, 0))
    dw = np.maximum(w_hi - w, w - w_lo)
    drho = np.maximum(rho_hi - rho, rho - rho_lo)
    if loss == LOSS_HUBER:
        dw = dw + 3 * U * w_hi
        # (well below the kink the linear branch evaluates to dl (1 -+ 4 u) > s and the min returns s itself: no rounding of its own)
        lin = 4 * U * (2 * np.sqrt(LD(dl)) * np.sqrt(np.maximum(s + ds, LD(dl))) + LD(dl))
        drho = drho + np.where(s + ds >= LD(dl) * (1 - 8 * U), lin, 0)
    elif loss == LOSS_GM:
        dw = dw + 5 * U * w_hi
        drho = drho + 3 * U * rho_hi
    elif loss == LOSS_WELSCH:
        own = ((s + ds) / LD(dl) + 2) * U * w_hi + TINY
        drho = drho + LD(dl) * own + U * LD(dl) * w_hi + U * rho_hi
        dw = dw + own
    return dw, drho


class Restatement:
    """One node's inter-edge operations.  info: the oracle's DataInfo of the node (its measurements and local indices)."""

    def __init__(self, info, d, loss, dl, xi):
        self.d, self.n0, self.n1 = d, info.n[0], info.n[1]
        self.P = self.n0 + self.n1
        self.loss, self.dl, self.xi = loss, dl, xi
        self.inter = Edges(info, info.inter, d)
        self.intra = Edges(info, info.intra, d)
        E = self.inter
        self.ninc = np.bincount(np.concatenate([E.i, E.j]), minlength=self.P)
        self.hub = int(np.argmax(self.ninc))

    # ---- residuals ---------------------------------------------------------------------------------------------------
    def residuals(self, E, T, Y, dT=None, dY=None, mut=None):
        """u, W, s of every edge of E at (T, Y) with their bounds; dT, dY: entrywise bounds on the point itself (the device's
        point is a rounded one: the fused extrapolation)."""
        d = self.d
        R = np.swapaxes(E.R, 1, 2) if mut == "R_for_RT" else E.R
        tau, kap = (E.kappa, E.tau) if mut == "tau_kappa" else (E.tau, E.kappa)
        dT = np.zeros(T.shape, LD) if dT is None else dT
        dY = np.zeros(Y.shape, LD) if dY is None else dY
        Yi, Yj = Y[E.i], Y[E.j]
        u = T[E.i] - T[E.j] + np.einsum("eq,eqc->ec", E.t, Yi)
        au = _abs(T[E.i]) + _abs(T[E.j]) + np.einsum("eq,eqc->ec", _abs(E.t), _abs(Yi))
        du = gam(d + 2) * au + dT[E.i] + dT[E.j] + np.einsum("eq,eqc->ec", _abs(E.t), dY[E.i])
        W = np.einsum("eqr,eqc->erc", R, Yi) - Yj
        aW = np.einsum("eqr,eqc->erc", _abs(R), _abs(Yi)) + _abs(Yj)
        dW = gam(d + 1) * aW + np.einsum("eqr,eqc->erc", _abs(R), dY[E.i]) + dY[E.j]
        s = tau * np.sum(u * u, axis=1) + kap * np.sum(W * W, axis=(1, 2))
        A = tau * np.sum(2 * _abs(u) * du + du * du, axis=1) + kap * np.sum(2 * _abs(W) * dW + dW * dW, axis=(1, 2))
        ds = A + gam(d + d * d + 2) * (s + A)
        return dict(u=u, W=W, s=s, du=du, dW=dW, ds=ds, tau=tau, kappa=kap, R=R)

    def weights(self, r, mut=None):
        w, rho = loss_fn(self.loss, self.dl, r["s"], mut)
        dw, drho = loss_bounds(self.loss, self.dl, r["s"], r["ds"])
        return w, rho, dw, drho

    # ---- DfE = B1^T W B1 Z on all rows ---------------------------------------------------------------------------------
    def _terms(self, E, r, w, dw):
        """Per edge: the tail pose's term (t: d, R: d x d) and the head pose's, with bounds and absolute values."""
        d = self.d
        tau, kap, R, u, W, du, dW = r["tau"], r["kappa"], r["R"], r["u"], r["W"], r["du"], r["dW"]
        w1, w2 = w[:, None], w[:, None, None]
        dw1, dw2 = dw[:, None], dw[:, None, None]
        a_t = tau[:, None] * u
        da_t = tau[:, None] * du + 2 * U * _abs(a_t)
        tt = tau[:, None] * E.t
        a_R = tt[:, :, None] * u[:, None, :] + kap[:, None, None] * np.einsum("eqr,erc->eqc", R, W)
        abs_R = _abs(tt)[:, :, None] * _abs(u)[:, None, :] + kap[:, None, None] * np.einsum("eqr,erc->eqc", _abs(R), _abs(W))
        da_R = _abs(tt)[:, :, None] * du[:, None, :] + kap[:, None, None] * np.einsum("eqr,erc->eqc", _abs(R), dW) \
            + gam(d + 2) * abs_R
        h_R = kap[:, None, None] * W
        dh_R = kap[:, None, None] * dW + 2 * U * _abs(h_R)
        return dict(
            tail_t=w1 * a_t, tail_R=w2 * a_R, head_t=-w1 * a_t, head_R=-w2 * h_R,
            d_tail_t=dw1 * _abs(a_t) + w1 * da_t, d_tail_R=dw2 * _abs(a_R) + w2 * da_R,
            d_head_t=dw1 * _abs(a_t) + w1 * da_t, d_head_R=dw2 * _abs(h_R) + w2 * dh_R)

    def dfe(self, T, Y, dT=None, dY=None, mut=None):
        """DfE on all poses as (Ft, FR), its bounds, and the per-edge quantities."""
        E, P, d = self.inter, self.P, self.d
        r = self.residuals(E, T, Y, dT, dY, mut)
        w, rho, dw, drho = self.weights(r, mut)
        tm = self._terms(E, r, w, dw)
        keep_tail = np.ones(E.m, bool)
        keep_head = np.ones(E.m, bool)
        extra = None
        if mut == "hub_last_skipped":
            at_hub = np.nonzero((E.i == self.hub) | (E.j == self.hub))[0]
            e = at_hub[-1]
            (keep_tail if E.i[e] == self.hub else keep_head)[e] = False
        if mut == "head_as_tail":
            # the first edge whose head is an own pose: at that pose the role bit reads "tail" -- the pose itself taken as z_i
            e = int(np.nonzero(E.j < self.n0)[0][0])
            keep_head[e] = False
            sw = E.take(np.array([e]))
            sw.i, sw.j = sw.j.copy(), sw.i.copy()
            rs = self.residuals(sw, T, Y, dT, dY)
            ws, _, dws, _ = self.weights(rs)
            extra = (int(E.j[e]), self._terms(sw, rs, ws, dws))
        Ft, FR = np.zeros((P, d), LD), np.zeros((P, d, d), LD)
        dFt, dFR = np.zeros((P, d), LD), np.zeros((P, d, d), LD)
        aFt, aFR = np.zeros((P, d), LD), np.zeros((P, d, d), LD)
        for role, idx, keep in (("tail", E.i, keep_tail), ("head", E.j, keep_head)):
            np.add.at(Ft, idx[keep], tm[role + "_t"][keep])
            np.add.at(FR, idx[keep], tm[role + "_R"][keep])
            np.add.at(dFt, idx[keep], tm["d_" + role + "_t"][keep])
            np.add.at(dFR, idx[keep], tm["d_" + role + "_R"][keep])
            np.add.at(aFt, idx[keep], _abs(tm[role + "_t"][keep]))
            np.add.at(aFR, idx[keep], _abs(tm[role + "_R"][keep]))
        if extra is not None:
            p, x = extra
            Ft[p] += x["tail_t"][0]
            FR[p] += x["tail_R"][0]
        k = gam(self.ninc + 2)
        dFt = dFt + k[:, None] * aFt
        dFR = dFR + k[:, None, None] * aFR
        return dict(Ft=Ft, FR=FR, dFt=dFt, dFR=dFR, w=w, rho=rho, dw=dw, drho=drho, s=r["s"], ds=r["ds"])

    # ---- block-diagonal terms --------------------------------------------------------------------------------------------
    def _end_blocks(self, E, mut=None):
        """E_end of every edge: (tail block, head block), (d+1) x (d+1)."""
        d, B = self.d, self.d + 1
        tail = np.zeros((E.m, B, B), LD)
        head = np.zeros((E.m, B, B), LD)
        ttT = E.tau[:, None, None] * E.t[:, :, None] * E.t[:, None, :]
        tail[:, 0, 0] = head[:, 0, 0] = E.tau
        for k in range(d):
            tail[:, 1 + k, 1 + k] = E.kappa
            head[:, 1 + k, 1 + k] = E.kappa
        tail[:, 0, 1:] = tail[:, 1:, 0] = E.tau[:, None] * E.t
        if mut == "ttT_on_head":
            head[:, 1:, 1:] += ttT
        else:
            tail[:, 1:, 1:] += ttT
        return tail, head

    def blocks(self, scale=None, dynamic=False, mut=None):
        """The block-diagonal terms of the surrogate: Gi = sum 2 s_e E_end over the inter-node incidences of an OWN pose (what the
        inter-node edges add to G's diagonal blocks; D = Gi + xi I), Q on all poses (the sum over both endpoints, + 2 xi I on own
        ones), H on own poses (Gi + 2 E_end over the intra-node incidences + 1.5 xi I, 0.5 xi I with Dynamic rescale:
        assemble_node) and from it T, N, V.  Each with its entrywise assembly bound."""
        d, B, n0, P = self.d, self.d + 1, self.n0, self.P
        E = self.inter
        sc = np.ones(E.m, LD) if scale is None else np.asarray(scale, LD)
        tail, head = self._end_blocks(E, mut)
        A = np.zeros((P, B, B), LD)
        absA = np.zeros((P, B, B), LD)
        w2 = (2 * sc)[:, None, None]
        np.add.at(A, E.i, w2 * tail)
        np.add.at(A, E.j, w2 * head)
        np.add.at(absA, E.i, _abs(w2 * tail))
        np.add.at(absA, E.j, _abs(w2 * head))
        I = np.eye(B, dtype=LD)
        own = (np.arange(P) < n0)[:, None, None]
        Q = A + np.where(own, 2 * LD(self.xi) * I, 0)
        if mut == "Q_own_only":
            Q = np.where(own, Q, 0)
        kk = gam(self.ninc + 4)[:, None, None]
        D = A[:n0] + LD(self.xi) * I
        ti, hi = self._end_blocks(self.intra)
        Hi = np.zeros((P, B, B), LD)
        absH = np.zeros((P, B, B), LD)
        np.add.at(Hi, self.intra.i, 2 * ti)
        np.add.at(Hi, self.intra.j, 2 * hi)
        np.add.at(absH, self.intra.i, _abs(2 * ti))
        np.add.at(absH, self.intra.j, _abs(2 * hi))
        nintra = np.bincount(np.concatenate([self.intra.i, self.intra.j]), minlength=P)
        H = Hi[:n0] + A[:n0] + (0.5 if dynamic else 1.5) * LD(self.xi) * I
        dH = gam(self.ninc[:n0] + nintra[:n0] + 5)[:, None, None] * (absH[:n0] + absA[:n0] + LD(self.xi) * I)
        Tv = 1 / H[:, 0, 0]
        N = Tv[:, None] * H[:, 0, 1:]
        V = H[:, 1:, 1:] - H[:, 1:, 0][:, :, None] * N[:, None, :]
        Gd = 0.5 * Hi[:n0] + A[:n0] + LD(self.xi) * I   # G's diagonal blocks: the intra-node edges count once there
        return dict(Gd=Gd, dGd=dH, Gi=A[:n0], dGi=(kk * absA)[:n0], D=D, dD=(kk * (absA + LD(self.xi) * I))[:n0], Q=Q, dQ=kk * (absA + 2 * LD(self.xi) * I),
                    H=H, dH=dH, T=Tv, N=N, V=V)

    # ---- the update pass (k_inter mode 0) ------------------------------------------------------------------------------------
    def update(self, Z, Zprev=None, DfE_old=None, GX=None, X=None, scale=None, dynamic=False, mut=None):
        """Everything launch_inter_update leaves, at Z (reference layout, own and neighbour rows).  Zprev, DfE_old (all rows): the
        quad term; GX, X (own rows): Dfobj, its tangent projection and |grad F|^2.  Values in extended precision, reference
        layout; every `d_x` is the bound of `x`."""
        d, n0, n1, B = self.d, self.n0, self.n1, self.d + 1
        T, Y = poses(Z, n0, n1, d)
        f = self.dfe(T, Y, mut=mut)
        out = dict(w=f["w"], dw=f["dw"], s=f["s"], ds=f["ds"], rho=f["rho"], drho=f["drho"])
        out["DfE"] = stack(f["Ft"], f["FR"], n0, n1)
        out["d_DfE"] = stack(f["dFt"], f["dFR"], n0, n1)
        out["sum_rho"] = np.sum(f["rho"])
        out["d_sum_rho"] = np.sum(f["drho"]) + self.inter.m * U * np.sum(_abs(f["rho"]))
        bl = self.blocks(scale, dynamic, mut)
        # g = DfE_own - D z: z as the (d+1) x d matrix [t ; Y] of the pose
        zmat = np.concatenate([T[:n0, None, :], Y[:n0]], axis=1)
        Dz = np.einsum("prk,pkc->prc", bl["D"], zmat)
        dDz = np.einsum("prk,pkc->prc", bl["dD"], _abs(zmat)) + gam(d + 2) * np.einsum("prk,pkc->prc", _abs(bl["D"]), _abs(zmat))
        fmat = np.concatenate([f["Ft"][:n0, None, :], f["FR"][:n0]], axis=1)
        dfmat = np.concatenate([f["dFt"][:n0, None, :], f["dFR"][:n0]], axis=1)
        gmat = fmat if mut == "no_Dz" else fmat - Dz
        dg = dfmat + dDz + U * _abs(gmat)
        out["g"] = stack(gmat[:, 0], gmat[:, 1:], n0, 0)
        out["d_g"] = stack(dg[:, 0], dg[:, 1:], n0, 0)
        terms = zmat * gmat
        out["zg"] = np.sum(terms)
        out["d_zg"] = np.sum(_abs(zmat) * dg) + gam((d + 1) * d + 1) * np.sum(_abs(terms)) + n0 * U * np.sum(_abs(terms))
        if Zprev is not None:
            Tp, Yp = poses(Zprev, n0, n1, d)
            To, Yo = poses(DfE_old, n0, n1, d)
            zall = np.concatenate([T[:, None, :], Y], axis=1)
            dz = zall - np.concatenate([Tp[:, None, :], Yp], axis=1)
            old = np.concatenate([To[:, None, :], Yo], axis=1)
            qz = np.einsum("prk,pkc->prc", bl["Q"], dz)
            dqz = np.einsum("prk,pkc->prc", bl["dQ"], _abs(dz)) + gam(d + 3) * np.einsum("prk,pkc->prc", _abs(bl["Q"]), _abs(dz))
            half = LD(1.0) if mut == "quad_no_half" else LD(0.5)
            inner = half * qz + old
            terms = dz * inner
            # dz: one subtraction (u |dz|, carried through Q above as one more term); inner: one fused multiply-add; the row's sum
            # of (d+1) d products by fused multiply-adds
            dterm = _abs(dz) * (0.5 * dqz) + (2 * U + gam((d + 1) * d + 1)) * _abs(dz) * (0.5 * _abs(qz) + _abs(old))
            out["quad"] = np.sum(terms)
            out["d_quad"] = np.sum(dterm) + self.P * U * np.sum(_abs(terms))
        if GX is not None:
            Tg, Yg = poses(GX, n0, 0, d)
            Tx, Yx = poses(X, n0, 0, d)
            vt = Tg + gmat[:, 0]
            vR = Yg + gmat[:, 1:]
            dvt = dg[:, 0] + U * _abs(vt)
            dvR = dg[:, 1:] + U * _abs(vR)
            out["Df"] = stack(vt, vR, n0, 0)
            out["d_Df"] = stack(dvt, dvR, n0, 0)
            # Proj_x(v) = v - sym(v x^T) x per block (SOdProduct.h:96-103): 3 d + 2 roundings per entry
            sym = lambda a, b: 0.5 * (np.einsum("pik,pjk->pij", a, b) + np.einsum("pik,pjk->pji", a, b))
            o = vR - np.einsum("pij,pjc->pic", sym(vR, Yx), Yx)
            ax = _abs(Yx)
            do = dvR + np.einsum("pij,pjc->pic", sym(dvR, ax), ax) \
                + gam(3 * d + 2) * (_abs(vR) + np.einsum("pij,pjc->pic", sym(_abs(vR), ax), ax))
            sq = np.concatenate([(vt * vt).ravel(), (o * o).ravel()])
            dsq = np.concatenate([(2 * _abs(vt) * dvt + dvt * dvt).ravel(), (2 * _abs(o) * do + do * do).ravel()])
            out["gn"] = np.sum(sq)
            out["d_gn"] = np.sum(dsq) + (gam((d + 1) * d + 1) + n0 * U) * np.sum(sq)
        return out

    # ---- the lazy unpack ---------------------------------------------------------------------------------------------------------
    def lazy_rows(self, Znbr_rows, recv, nsrc, mut=None):
        """The neighbour rows the pass reads (n1 records of (d+1) d numbers): from the receive buffer where nsrc >= 0, from Znbr else."""
        out = np.array(Znbr_rows, copy=True)
        if mut != "lazy_from_Znbr":
            for r in range(self.n1):
                if nsrc[r] >= 0:
                    out[r] = recv[nsrc[r]]
        return out

    # ---- the iterate pass (k_inter mode 1) -----------------------------------------------------------------------------------------
    def iterate(self, Zc, Zp, gamma, GXc=None, GXp=None, scale=None, dynamic=False, prox=False, Xref=None, gamma_other=None, mut=None):
        """launch_inter_iterate at Y = Zc + gamma (Zc - Zp) (gamma = 0, Zp = Zc: the plain shape at Zc): Y on all rows, g and
        <Y, g> over own rows; with GXc, GXp: Df = g + GXc + gamma (GXc - GXp); with prox: the proximal half step on Df."""
        d, n0, n1 = self.d, self.n0, self.n1
        Tc, Yc = poses(Zc, n0, n1, d)
        Tp, Yp = poses(Zp, n0, n1, d)
        gm = np.full(self.P, LD(gamma))
        if mut == "gamma_other_node":
            gm[n0:] = LD(gamma_other)
        T = Tc + gm[:, None] * (Tc - Tp)
        Y = Yc + gm[:, None, None] * (Yc - Yp)
        # the device's point: fl(zc + gamma fl(zc - zp)): u |gamma (zc - zp)| + u |y|
        dT = U * (_abs(gm[:, None] * (Tc - Tp)) + _abs(T)) * (gamma != 0)
        dY = U * (_abs(gm[:, None, None] * (Yc - Yp)) + _abs(Y)) * (gamma != 0)
        f = self.dfe(T, Y, dT, dY, mut=mut)
        bl = self.blocks(scale, dynamic, mut)
        out = dict(Y=stack(T, Y, n0, n1), d_Y=stack(dT, dY, n0, n1))
        zmat = np.concatenate([T[:n0, None, :], Y[:n0]], axis=1)
        dzmat = np.concatenate([dT[:n0, None, :], dY[:n0]], axis=1)
        Dz = np.einsum("prk,pkc->prc", bl["D"], zmat)
        dDz = np.einsum("prk,pkc->prc", bl["dD"], _abs(zmat)) + np.einsum("prk,pkc->prc", _abs(bl["D"]), dzmat + gam(d + 2) * _abs(zmat))
        fmat = np.concatenate([f["Ft"][:n0, None, :], f["FR"][:n0]], axis=1)
        dfmat = np.concatenate([f["dFt"][:n0, None, :], f["dFR"][:n0]], axis=1)
        gmat = fmat if mut == "no_Dz" else fmat - Dz
        dg = dfmat + dDz + U * _abs(gmat)
        out["g"], out["d_g"] = stack(gmat[:, 0], gmat[:, 1:], n0, 0), stack(dg[:, 0], dg[:, 1:], n0, 0)
        terms = zmat * gmat
        out["zg"] = np.sum(terms)
        out["d_zg"] = np.sum(_abs(zmat) * dg + dzmat * _abs(gmat)) + (gam((d + 1) * d + 1) + n0 * U) * np.sum(_abs(terms))
        if GXc is not None:
            a = np.asarray(GXc, LD)
            b = np.asarray(GXp, LD)
            lin = a + LD(gamma) * (a - b)
            Df = out["g"] + lin
            # fl(a - b), the fused multiply-add, the sum with g
            dDf = out["d_g"] + U * (_abs(LD(gamma) * (a - b)) + _abs(lin)) + U * _abs(Df)
            out["Df"], out["d_Df"] = Df, dDf
            if prox:
                Tf, Yf = poses(Df, n0, 0, d)
                dTf, dYf = poses(dDf, n0, 0, d)
                Tv, N, V = bl["T"], bl["N"], bl["V"]
                # M = -Df_R + N^T Df_t + V R0   (DPGOProblem.cpp:618-620)
                M = -Yf + N[:, :, None] * Tf[:, None, :] + np.einsum("prk,pkc->prc", V, Y[:n0])
                out["M"] = M
                out["d_M"] = dYf + _abs(N)[:, :, None] * dTf[:, None, :] + np.einsum("prk,pkc->prc", _abs(V), dY[:n0]) \
                    + gam(d + 3) * (_abs(Yf) + _abs(N)[:, :, None] * _abs(Tf)[:, None, :] + np.einsum("prk,pkc->prc", _abs(V), _abs(Y[:n0])))
                out["prox_t"] = lambda Rnew: T[:n0] - np.einsum("pk,pkc->pc", N, np.asarray(Rnew, LD) - Y[:n0]) - Tv[:, None] * Tf
                out["prox_t_bound"] = lambda Rnew: gam(d + 2) * (_abs(T[:n0]) + np.einsum("pk,pkc->pc", _abs(N), _abs(np.asarray(Rnew, LD) - Y[:n0]))
                                                                + _abs(Tv[:, None] * Tf)) + dT[:n0] + np.einsum("pk,pkc->pc", _abs(N), dY[:n0]) \
                    + _abs(Tv)[:, None] * dTf + np.sum(_abs(N), axis=1)[:, None] * 1e-12
        return out

    @staticmethod
    def xref_after(Xref, Xout, n0, mut=None):
        """Xref once the proximal step has gone by: its translations kept, its rotations replaced by Xout's."""
        out = np.array(Xref, copy=True)
        if mut != "Xref_R_kept":
            out[n0:] = Xout[n0:]
        return out

    # ---- the objective (k_cost) ------------------------------------------------------------------------------------------------------
    def cost(self, Z, eform):
        """(slot 0: the sum over the intra-node edges of s_e; slot 1: the sum over the inter-node edges of rho(s_e)) with bounds.
        eform 1 states the rotation part as kappa (|Y_i|^2 + |Y_j|^2 - 2 <Y_i, R Y_j>) (the data-matrix form)."""
        d = self.d
        T, Y = poses(Z, self.n0, self.n1, d)
        out = []
        for E, robust in ((self.intra, False), (self.inter, True)):
            r = self.residuals(E, T, Y)
            s, ds = r["s"], r["ds"]
            if eform:
                Yi, Yj = Y[E.i], Y[E.j]
                RY = np.einsum("eqr,erc->eqc", E.R, Yj)
                aRY = np.einsum("eqr,erc->eqc", _abs(E.R), _abs(Yj))
                rot = np.sum(Yi * Yi + Yj * Yj - 2 * Yi * RY, axis=(1, 2))
                arot = np.sum(Yi * Yi + Yj * Yj + 2 * _abs(Yi) * aRY, axis=(1, 2))
                tr = E.tau * np.sum(r["u"] ** 2, axis=1)
                dtr = E.tau * np.sum(2 * _abs(r["u"]) * r["du"] + r["du"] ** 2, axis=1) + gam(d + 2) * tr
                s = tr + E.kappa * rot
                # per entry: d fused multiply-adds for R Y_j, three products, two sums; d^2 entries accumulated, one fused multiply-add
                ds = dtr + E.kappa * gam(d + 5 + d * d + 1) * arot + U * _abs(s)
            if robust:
                rho = loss_fn(self.loss, self.dl, s)[1]
                drho = loss_bounds(self.loss, self.dl, s, ds)[1]
            else:
                rho, drho = s, ds
            out.append((np.sum(rho), np.sum(drho) + max(E.m, 1) * U * np.sum(_abs(rho))))
        return out


# ---- the Dynamic rescale's decision (DPGOProblem.cpp:300-321) -- exact in fp64: one product and two comparisons per edge ----------
def rescale_decide(w, scale, count, max_count, mut=None):
    """-> (flag, new scales, new counter) of one node: rescaled when the counter has reached max_count or a weight exceeds its
    scale; new scales clip(1.25 w, 0.01, 1)."""
    w = np.asarray(w, np.float64)
    scale = np.asarray(scale, np.float64)
    over = np.any(w >= scale) if mut == "rescale_ge" else np.any(w > scale)
    if count >= max_count or over:
        return 1, np.clip(1.25 * w, 0.1 if mut == "clamp_0.1" else 0.01, 1.0), 0
    return 0, scale.copy(), count + 1


# ---- the inputs of the tests (host and GPU alike) ---------------------------------------------------------------------------------
def measurements(g):
    from oracle import g2o as og
    z = np.zeros(len(g["I"]), np.int64)
    return og.Measurements(z, g["I"], z, g["J"], g["R"], g["t"], g["kappa"], g["tau"])


def node_measurements(g):
    from oracle import g2o as og
    return og.partition_measurements(g["num_poses"], measurements(g), g["num_nodes"])[1]


def truth_point(g, info, a, span):
    """The ground truth of inter_ladder on node a's rows, reference layout (float64)."""
    d, n0, n1 = g["d"], info.n[0], info.n[1]
    T = np.zeros((n0 + n1, d))
    Y = np.zeros((n0 + n1, d, d))
    for nd, tab in info.index.items():
        for p, (blk, k) in tab.items():
            gid = nd * span + p
            T[k + (n0 if blk else 0)] = g["tg"][gid]
            Y[k + (n0 if blk else 0)] = g["Rg"][gid].T
    return stack(T, Y, n0, n1)


def extrapolated_point(rng, Ztruth, n0, n1, d):
    """A point as an extrapolation leaves it: rotation blocks off the manifold (entries scaled by 1 -+ 0.3, sheared), translations
    up to 1e3 (log-uniform factors 1 .. 100 on [0, 10)): the cancellation in u matters."""
    T, Y = poses(Ztruth, n0, n1, d)
    T = np.asarray(T, np.float64) * 10.0 ** rng.uniform(0, 2, (n0 + n1, 1))
    Y = np.asarray(Y, np.float64) * (1 + 0.3 * rng.uniform(-1, 1, Y.shape)) + 0.1 * rng.standard_normal(Y.shape)
    return stack(T, Y, n0, n1)


def regime_counts(s, dl):
    """How many squared residuals fall in each regime of the losses."""
    s = np.asarray(s, np.float64)
    return dict(small=int(np.sum(s < 1e-3 * dl)), kink_below=int(np.sum((s >= 0.9 * dl) & (s < dl))),
                kink_above=int(np.sum((s > dl) & (s <= 1.1 * dl))), large=int(np.sum((s > 1e2 * dl) & (s <= 745 * dl))),
                underflow=int(np.sum(s > 745 * dl)))


def within(got, ref, bound):
    """(all entries within their bound, the worst error / bound ratio)."""
    err = np.abs(np.asarray(got, LD) - ref)
    b = np.asarray(bound, LD)
    ratio = np.where(err == 0, LD(0), err / np.where(b > 0, b, LD(TINY)))
    worst = float(np.max(ratio)) if np.size(ratio) else 0.0
    return bool(np.all(err <= b)), worst


def iterate_inputs(rs, rng, Zc, Zp, gamma, scale=None, dynamic=False):
    """The kept products and the reference point of an iterate pass: GXp random; GXc such that the matrix the fused proximal step
    projects, M = -Df_R + N^T Df_t + V R0, is s_p (Q_p + 0.3 E_p) per pose -- Q_p a rotation, |E_p| <= 1 / d entrywise, s_p the size of
    the terms that cancel to it (as test_gpu_operators.py chooses its Df); Xref random."""
    d, n0 = rs.d, rs.n0
    it = rs.iterate(Zc, Zp, gamma, scale=scale, dynamic=dynamic)
    bl = rs.blocks(scale, dynamic)
    gt, gR = poses(it["g"], n0, 0, d)
    _, Y = poses(it["Y"], n0, rs.n1, d)
    lin_t = 10.0 * rng.standard_normal((n0, d))
    Dft = gt + lin_t
    rest = bl["N"][:, :, None] * Dft[:, None, :] + np.einsum("prk,pkc->prc", bl["V"], Y[:n0])
    sc = np.maximum(1.0, np.linalg.norm(np.asarray(rest, np.float64).reshape(n0, -1), axis=1))[:, None, None]
    Q = np.linalg.qr(rng.standard_normal((n0, d, d)))[0]
    Q[:, :, 0] *= np.sign(np.linalg.det(Q))[:, None]
    Mstar = sc * (Q + 0.3 * rng.uniform(-1, 1, (n0, d, d)) / d)
    lin_R = rest - Mstar - gR
    lin = np.asarray(stack(lin_t, lin_R, n0, 0), np.float64)
    GXp = 50.0 * rng.standard_normal(lin.shape)
    GXc = (lin + gamma * GXp) / (1.0 + gamma)
    Xref = np.asarray(Zc[:(d + 1) * n0], np.float64) + 0.1 * rng.standard_normal(lin.shape)
    return GXc, GXp, Xref
