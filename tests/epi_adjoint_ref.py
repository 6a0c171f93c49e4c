"""The adjoints of the epipolar distances, restated per point in numpy float64, with a 50-digit mpmath twin.

Written from the reference's lines (deepFEPE/dsac_tools/utils_F.py), not from the kernels:
  :291-308 _sampson_dist    e = s^2 / (A + Q)
  :310-339 _sym_epi_dist    e = s^2 (1 / (A + eps) + 1 / (Q + eps)), eps = 1e-10 in the batched branch only, clamp(max=clamp_at)
  :341-361 _epi_distance    d1 = |s| / sqrt(A), d2 = |s| / sqrt(Q), returns ((d1 + d2) / 2, d1, d2)
  :400-413 compute_epi_residual, here with respect to the POINTS (tests/epipolar_ref.py has the forward and the adjoint to F)
with x = (x0, x1, x2), y likewise (third coordinate the constant 1, no gradient, unless if_homo), a = F x, b = F^T y, s = y^T F x,
A = a0^2 + a1^2, Q = b0^2 + b1^2.  The forward is tests/epipolar_ref.py's (its _homo is used, and the CPU test holds the values
below to its sym_epi, sampson and epi_distance); this file adds the derivatives.  Every metric is e(s, A, Q), so
de = cs ds + cA dA + cQ dQ with
  ds/dF_rc = y_r x_c          ds/dx = b                          ds/dy = a
  dA/dF_rc = 2 a_r x_c [r<2]  dA/dx_c = 2 (a0 F_0c + a1 F_1c)    dA/dy = 0
  dQ/dF_rc = 2 b_c y_r [c<2]  dQ/dy_r = 2 (b0 F_r0 + b1 F_r1)    dQ/dx = 0
Conventions (where torch's autograd has a choice, the line it follows): with a clamp the gradient passes where e <= clamp_at (:337,
torch.clamp(max=) passes it AT the bound); sign(0) = 0 (:347, :407, the derivative torch gives abs() at 0); k = 0 where a norm is 0
(:407), as tests/epipolar_ref.py states for the adjoint to F.

Next to every output stand two sums over its terms:
  T  the sum of the absolute values of the terms as they are (|cs| |y_r x_c| + 2 |cA| |a_r x_c| + 2 |cQ| |b_c y_r|, ...), with the
     gate applied: a clamped-out point has T = 0.  The summation error of g_F is stated against it.
  M  T plus the first-order effect of the roundings INSIDE the computed quantities.  The issue states the bound against the
     absolute-term sum alone; that cannot hold here, and this is the one place where this file departs from its wording: s = y^T F x
     cancels by four to five digits at an inlier in pixel coordinates, so its fp64 value is off by 2^-53 sbar, sbar = sum |y_r F_rc x_c|
     >> |s|, and every term carries |d term / d s| 2^-53 sbar, which T does not see.  M adds exactly these: with the errors (in units
     of 2^-53) ds = sbar, da_r = abar_r = sum_c |F_rc x_c|, db_c likewise, dA = 2 (|a0| abar_0 + |a1| abar_1) + A, dQ likewise,
       dcs = |d cs/d s| ds + |d cs/d A| dA + |d cs/d Q| dQ,   dcA, dcQ likewise   (analytic, per kind)
       M(g_F_rc) = T + dcs |y_r x_c| + 2 dcA |a_r x_c| + 2 |cA| abar_r |x_c| + 2 dcQ |b_c y_r| + 2 |cQ| bbar_c |y_r|
     and the same for g_x, g_y and the residual.  Nothing is squared that the derivative does not square (2 |s| sbar, not sbar^2),
     every reciprocal carries one condition factor, and a clamped-out point that is not flagged has M = 0.
The kernels read fp32, work in fp64 and round each output once, so per output
  |got - ref| <= 2^-24 |ref| + 2^-149 + C 2^-53 M                                    bound(...)
(2^-149, the smallest fp32 step, is what rounding an fp64 value below the normal range can move it by; the issue's statement leaves
it out) and for a sum over the N points of a pair (g_F, the loss sums) additionally N 2^-53 sum T.  check() of
tests/epi_adjoint_cases.py asserts that the g_F bound of every pair stays below MAX_BOUND_FRACTION of the pair's largest |g_F|, so a
bound that tests nothing fails.

The constant.  It is not chosen: tests/test_epi_adjoint_ref_cpu.py runs the HOST build of csrc/epi_adjoint_math.h (tests/emu/
emu_epi_adjoint.cpp, g++) against the 50-digit twin below on every shared case of tests/epi_adjoint_cases.py (scenes in pixel
coordinates and integer-built cases) and takes the smallest c for which |host - exact| <= c 2^-53 M holds for every output.
Measured there:
  C_MEASURED = 1.3     (largest ratio seen: 1.23, on a scene case; 0.2 .. 0.65 on the integer-built ones;
                        test_host_arithmetic_within_the_measured_constant prints it), used as 4 x = 5.2
The bound used everywhere is 4 x that, the margin tests/epipolar_ref.py and tests/test_refcfg_gpu.py use; it covers the device's
1-ulp fp64 division and square root and its tree sums.  The restatement against the reference's own float64 autograd
(tests/golden/epi_adjoint.npz) is measured the same way: torch's matmul order differs from the restatement's by roundings of the same
products, so the distance is stated in the same unit:
  C_GOLDEN_MEASURED = 1.0   (largest ratio seen: 0.86), used as 4 x = 4.
Flagged points: |e - clamp_at| <= C 2^-53 de (the gate may fall either way) or |s| <= C 2^-53 sbar with sbar > 0 (the sign may).  A
flagged point is never dropped: it keeps its float64 branch and twice the T it would have with the gate open widens the bound of what
it touches.  Cases built from small integers (every product and sum exact in fp64) are decided exactly and are not flagged.  Over the
shared cases no point is flagged (the fp64 bands are ~1e-12 relative; FLAGGED_NOTE)."""
import numpy as np

import epipolar_ref as er

U32 = 2.0 ** -24
U64 = 2.0 ** -53
TINY32 = 2.0 ** -149
C_MEASURED = 1.3
C_GOLDEN_MEASURED = 1.0
C = 4 * C_MEASURED
C_GOLDEN = 4 * C_GOLDEN_MEASURED
FLAGGED_NOTE = "shared cases: 0 near-gate and 0 sign-uncertain points in every case"

_F64 = np.float64
_M2 = np.array([1.0, 1.0, 0.0])


class Out:
    pass


def _terms(F, X, Y, homo, exact=False):
    F = np.asarray(F, dtype=_F64)
    x, y = er._homo(X, homo), er._homo(Y, homo)
    t = Out()
    t.F, t.x, t.y = F, x, y
    t.a = np.einsum("brc,bnc->bnr", F, x)
    t.b = np.einsum("brc,bnr->bnc", F, y)
    t.s = (y * t.a).sum(-1)
    t.A = t.a[..., 0] ** 2 + t.a[..., 1] ** 2
    t.Q = t.b[..., 0] ** 2 + t.b[..., 1] ** 2
    aF, ax, ay = np.abs(F), np.abs(x), np.abs(y)
    t.abar = np.einsum("brc,bnc->bnr", aF, ax)
    t.bbar = np.einsum("brc,bnr->bnc", aF, ay)
    t.sbar = (ay * t.abar).sum(-1)
    if exact:  # every product and sum is exact: a computed quantity carries no error beyond its own rounding
        t.abar, t.bbar, t.sbar = np.abs(t.a), np.abs(t.b), np.abs(t.s)
    # the error of A = a0^2 + a1^2 in units of 2^-53, to first order: 2 |a_r| da_r and the roundings of the squares and their sum
    t.dA = 2 * (np.abs(t.a[..., 0]) * t.abar[..., 0] + np.abs(t.a[..., 1]) * t.abar[..., 1]) + t.A
    t.dQ = 2 * (np.abs(t.b[..., 0]) * t.bbar[..., 0] + np.abs(t.b[..., 1]) * t.bbar[..., 1]) + t.Q
    return t


def _assemble(t, c, d, o, flagged):
    """The three outputs from c = (cs, cA, cQ); their T from |c|; their M from T, the coefficient errors d = (dcs, dcA, dcQ) and the
    errors of a and b; W = twice the T of the open-gate coefficients o where the point is flagged."""
    F, x, y, a, b = t.F[:, None], t.x, t.y, t.a, t.b
    cs, cA, cQ = c
    acs, acA, acQ = (np.abs(v) for v in c)
    dcs, dcA, dcQ = d
    e = lambda v: v[..., None]          # noqa: E731
    ee = lambda v: v[..., None, None]   # noqa: E731
    yx = y[..., :, None] * x[..., None, :]
    ax_ = (a * _M2)[..., :, None] * x[..., None, :]
    by_ = (b * _M2)[..., None, :] * y[..., :, None]
    abx = (t.abar * _M2)[..., :, None] * np.abs(x)[..., None, :]
    bby = (t.bbar * _M2)[..., None, :] * np.abs(y)[..., :, None]
    r = Out()
    r.gF_pt = ee(cs) * yx + 2 * ee(cA) * ax_ + 2 * ee(cQ) * by_
    tf = lambda u, v, w: ee(u) * np.abs(yx) + 2 * ee(v) * np.abs(ax_) + 2 * ee(w) * np.abs(by_)   # noqa: E731
    r.TF_pt = tf(acs, acA, acQ)
    r.MF_pt = r.TF_pt + tf(dcs, dcA, dcQ) + 2 * ee(acA) * abx + 2 * ee(acQ) * bby
    r.WF_pt = 2.0 * tf(*o) * ee(flagged)
    aFr = a[..., 0:1] * F[..., 0, :], a[..., 1:2] * F[..., 1, :]            # a0 F_0c, a1 F_1c   [B,N,3]
    bFc = b[..., 0:1] * F[..., :, 0], b[..., 1:2] * F[..., :, 1]            # b0 F_r0, b1 F_r1
    aaF, abF = np.abs(aFr[0]) + np.abs(aFr[1]), np.abs(bFc[0]) + np.abs(bFc[1])
    aF = np.abs(F)
    baF = t.abar[..., 0:1] * aF[..., 0, :] + t.abar[..., 1:2] * aF[..., 1, :]
    bbF = t.bbar[..., 0:1] * aF[..., :, 0] + t.bbar[..., 1:2] * aF[..., :, 1]
    r.gX = e(cs) * b + 2 * e(cA) * (aFr[0] + aFr[1])
    r.gY = e(cs) * a + 2 * e(cQ) * (bFc[0] + bFc[1])
    r.TX = e(acs) * np.abs(b) + 2 * e(acA) * aaF
    r.TY = e(acs) * np.abs(a) + 2 * e(acQ) * abF
    r.MX = r.TX + e(dcs) * np.abs(b) + e(acs) * t.bbar + 2 * e(dcA) * aaF + 2 * e(acA) * baF
    r.MY = r.TY + e(dcs) * np.abs(a) + e(acs) * t.abar + 2 * e(dcQ) * abF + 2 * e(acQ) * bbF
    r.WX = 2.0 * (e(o[0]) * np.abs(b) + 2 * e(o[1]) * aaF) * e(flagged)
    r.WY = 2.0 * (e(o[0]) * np.abs(a) + 2 * e(o[2]) * abF) * e(flagged)
    return r


def metrics_adjoint(kind, F, X, Y, homo, g, clamp_at=None, eps=0.0, exact=False, c=C, eps32=True):
    """kind 0 / 1: g [B,N]; kind 2: g [3,B,N].  float32 inputs as the kernels see them.  Returns an Out with value(s) and vmag (the M
    of the value), the per-point outputs gF_pt [B,N,3,3], gX, gY [B,N,3] (third column meaningless unless homo), their T*, M* and W*
    (the widening by flagged points), the sums gF, TF, MF [B,3,3], and flagged [B,N].  exact: the case is built from small integers,
    every decision is exact, nothing is flagged."""
    t = _terms(F, X, Y, homo, exact)
    g = np.asarray(g, dtype=_F64)
    eps = float(np.float32(eps)) if eps32 else float(eps)  # the float32 the kernel is given; the reference's own double 1e-10
    s, A, Q, sb, dA, dQ = t.s, t.A, t.Q, t.sbar, t.dA, t.dQ
    as_ = np.abs(s)
    none = np.zeros(s.shape, bool)
    with np.errstate(all="ignore"):
        if kind == 0:
            iA, iQ = 1.0 / (A + eps), 1.0 / (Q + eps)
            R = iA + iQ
            e_open = s * s * R
            # de = 2 s R ds + s^2 dR, its own roundings, and the second order that remains where s = 0
            vmag = 2 * as_ * sb * R + s * s * (iA * iA * dA + iQ * iQ * dQ) + e_open + U64 * sb * sb * R
            if clamp_at is None:
                gate, flagged, value = ~none, none, e_open
            else:
                cl = float(np.float32(clamp_at))
                gate = e_open <= cl
                flagged = np.abs(e_open - cl) <= c * U64 * vmag
                value = np.where(e_open > cl, cl, e_open)
            flagged = none if exact else flagged
            ag, gg = np.abs(g), g * gate
            ocs, ocA, ocQ = 2 * s * R, -s * s * iA * iA, -s * s * iQ * iQ          # the open-gate coefficients of one unit of g
            live = np.abs(gg)                                                      # 0 for a clamped-out point
            coef = (gg * ocs, gg * ocA, gg * ocQ)
            d = (live * (2 * R * sb + 2 * as_ * (iA * iA * dA + iQ * iQ * dQ)),
                 live * (2 * as_ * iA * iA * sb + 2 * s * s * iA ** 3 * dA + U64 * sb * sb * iA * iA),
                 live * (2 * as_ * iQ * iQ * sb + 2 * s * s * iQ ** 3 * dQ + U64 * sb * sb * iQ * iQ))
            o = (ag * np.abs(ocs), ag * np.abs(ocA), ag * np.abs(ocQ))
        elif kind == 1:
            iD = 1.0 / (A + Q)
            dD = dA + dQ
            value = s * s * iD
            vmag = 2 * as_ * sb * iD + s * s * iD * iD * dD + value + U64 * sb * sb * iD
            gate, flagged = ~none, none
            ag = np.abs(g)
            cA = -g * s * s * iD * iD
            coef = (g * 2 * s * iD, cA, cA)
            dcA = ag * (2 * as_ * iD * iD * sb + 2 * s * s * iD ** 3 * dD + U64 * sb * sb * iD * iD)
            d = (ag * (2 * iD * sb + 2 * as_ * iD * iD * dD), dcA, dcA)
            o = tuple(np.abs(v) for v in coef)
        else:
            rA, rQ = np.sqrt(A), np.sqrt(Q)
            d1, d2 = as_ / rA, as_ / rQ
            value = np.stack(((d1 + d2) / 2.0, d1, d2))
            m1, m2 = sb / rA + as_ * dA / (2 * A * rA) + d1, sb / rQ + as_ * dQ / (2 * Q * rQ) + d2
            vmag = np.stack(((m1 + m2) / 2.0, m1, m2))
            flagged = none if exact else ((as_ <= c * U64 * sb) & (sb > 0))
            gate = ~none
            h1, h2 = g[1] + 0.5 * g[0], g[2] + 0.5 * g[0]
            ah1, ah2 = np.abs(g[1]) + 0.5 * np.abs(g[0]), np.abs(g[2]) + 0.5 * np.abs(g[0])
            sg = np.sign(s)
            coef = (sg * (h1 / rA + h2 / rQ), -h1 * as_ / (2 * A * rA), -h2 * as_ / (2 * Q * rQ))
            d = (ah1 * dA / (2 * A * rA) + ah2 * dQ / (2 * Q * rQ),
                 ah1 * (sb / (2 * A * rA) + 0.75 * as_ * dA / (A * A * rA)),
                 ah2 * (sb / (2 * Q * rQ) + 0.75 * as_ * dQ / (Q * Q * rQ)))
            o = (ah1 / rA + ah2 / rQ, np.abs(coef[1]), np.abs(coef[2]))           # whichever sign
        r = _assemble(t, coef, d, o, flagged)
    r.t, r.value, r.vmag, r.gate, r.flagged = t, value, vmag, gate, flagged
    r.gF, r.TF, r.MF = r.gF_pt.sum(1), r.TF_pt.sum(1), r.MF_pt.sum(1)
    r.N = s.shape[1]
    return r


def residual_adjoint(pts1, pts2, F, clamp_at, g, exact=False, c=C):
    """compute_epi_residual w.r.t. pts1, pts2 [B,N,3]: Out with g1, g2 [B,N,3], T1, T2, M1, M2, W1, W2, flagged [B,N] and d
    (unclamped)."""
    t = _terms(F, pts1, pts2, True, exact)  # a = l2 = F x1, b = l1 = F^T x2, s = dd
    g = np.asarray(g, dtype=_F64)
    cl = float(np.float32(clamp_at))
    F_ = t.F[:, None]
    aF = np.abs(F_)
    with np.errstate(all="ignore"):
        n1, n2 = np.sqrt(t.Q), np.sqrt(t.A)
        # dn = dA / (2 n) and the rounding of the root; a norm that is exactly 0 from exact terms carries none
        dn1 = np.where(n1 > 0, t.dQ / (2 * n1), np.where(t.dQ > 0, np.inf, 0.0)) + n1
        dn2 = np.where(n2 > 0, t.dA / (2 * n2), np.where(t.dA > 0, np.inf, 0.0)) + n2
        i1, i2 = 1.0 / (n1 + 1e-6), 1.0 / (n2 + 1e-6)
        S, dS = i1 + i2, i1 * i1 * dn1 + i2 * i2 * dn2 + i1 + i2
        ad = np.abs(t.s)
        d, dd = ad * S, t.sbar * S + ad * dS
        gate = d <= cl
        flagged = (np.abs(d - cl) <= c * U64 * dd) | ((ad <= c * U64 * t.sbar) & (t.sbar > 0))
        flagged = np.zeros(d.shape, bool) if exact else flagged
        k1 = np.where(n1 > 0, ad * i1 * i1 / n1, 0.0)
        k2 = np.where(n2 > 0, ad * i2 * i2 / n2, 0.0)
        dk1 = np.where(n1 > 0, t.sbar * i1 * i1 / n1 + ad * (2 * i1 ** 3 / n1 + i1 * i1 / (n1 * n1)) * dn1, 0.0)
        dk2 = np.where(n2 > 0, t.sbar * i2 * i2 / n2 + ad * (2 * i2 ** 3 / n2 + i2 * i2 / (n2 * n2)) * dn2, 0.0)
        e = lambda v: v[..., None]  # noqa: E731
        u1 = (t.a[..., 0:1] * F_[..., 0, :], t.a[..., 1:2] * F_[..., 1, :])   # F[:2,:]^T l2[:2]
        u2 = (t.b[..., 0:1] * F_[..., :, 0], t.b[..., 1:2] * F_[..., :, 1])   # F[:,:2] l1[:2]
        au1, au2 = np.abs(u1[0]) + np.abs(u1[1]), np.abs(u2[0]) + np.abs(u2[1])
        bu1 = t.abar[..., 0:1] * aF[..., 0, :] + t.abar[..., 1:2] * aF[..., 1, :]
        bu2 = t.bbar[..., 0:1] * aF[..., :, 0] + t.bbar[..., 1:2] * aF[..., :, 1]
        sg, ag = np.sign(t.s), np.abs(g)
        live = ag * gate
        r = Out()
        r.g1 = e(g * gate) * (e(sg * S) * t.b - e(k2) * (u1[0] + u1[1]))
        r.g2 = e(g * gate) * (e(sg * S) * t.a - e(k1) * (u2[0] + u2[1]))
        open1, open2 = e(S) * np.abs(t.b) + e(k2) * au1, e(S) * np.abs(t.a) + e(k1) * au2
        r.T1, r.T2 = e(live) * open1, e(live) * open2
        r.M1 = r.T1 + e(live) * (e(dS) * np.abs(t.b) + e(S) * t.bbar + e(dk2) * au1 + e(k2) * bu1)
        r.M2 = r.T2 + e(live) * (e(dS) * np.abs(t.a) + e(S) * t.abar + e(dk1) * au2 + e(k1) * bu2)
        r.W1, r.W2 = 2.0 * e(ag * flagged) * open1, 2.0 * e(ag * flagged) * open2
    r.t, r.d, r.gate, r.flagged = t, d, gate, flagged
    return r


def loss(kind, F, X, Y, homo, w=None, g_sum=None, clamp_at=None, eps=0.0, exact=False):
    """The reduced form: sums [B] = sum_n w e (e: kind 0, 1 or the first plane of kind 2) and, for g_sum [B], the adjoint: an Out of
    metrics_adjoint for the upstream g_sum[b] w[b,n], plus sums, Msum, Tsum [B], gw, Mgw [B,N]."""
    B, N = np.asarray(X).shape[:2]
    w64 = np.ones((B, N)) if w is None else np.asarray(w, dtype=_F64)
    gs = np.ones(B) if g_sum is None else np.asarray(g_sum, dtype=_F64)
    g = gs[:, None] * w64
    if kind == 2:
        g = np.stack((g, np.zeros_like(g), np.zeros_like(g)))
    r = metrics_adjoint(kind, F, X, Y, homo, g, clamp_at, eps, exact)
    v, vm = (r.value[0], r.vmag[0]) if kind == 2 else (r.value, r.vmag)
    vm = np.where(r.gate, vm, np.abs(v))  # a clamped value is the constant itself
    with np.errstate(all="ignore"):
        r.e, r.sums, r.Tsum, r.Msum = v, (w64 * v).sum(1), (np.abs(w64) * np.abs(v)).sum(1), (np.abs(w64) * vm).sum(1)
        r.gw, r.Mgw = gs[:, None] * v, np.abs(gs)[:, None] * vm
    return r


# ---- the bound -------------------------------------------------------------------------------------------------------------------
def bound(ref, M, c=C):
    """Per output rounded once from fp64: 2^-24 |ref| + 2^-149 + c 2^-53 M.  Not finite where the reference is not."""
    with np.errstate(all="ignore"):
        b = U32 * np.abs(ref) + TINY32 + c * U64 * M
    return np.where(np.isfinite(ref) & np.isfinite(M), b, np.inf)


def bound_sum(ref, M_pt, T_pt, W_pt, c=C):
    """A sum over the points (axis 1) rounded once: the per-point fp64 terms, the summation, and the widening of the flagged points."""
    N = T_pt.shape[1]
    with np.errstate(all="ignore"):
        b = U32 * np.abs(ref) + TINY32 + c * U64 * M_pt.sum(1) + N * U64 * T_pt.sum(1) + W_pt.sum(1)
    return np.where(np.isfinite(ref) & np.isfinite(b), b, np.inf)


def bound_point(ref, M, W, c=C):
    """A per-point output [B,N,k]: bound() plus the widening where the point is flagged."""
    with np.errstate(all="ignore"):
        b = bound(ref, M, c) + W
    return np.where(np.isfinite(b), b, np.inf)


def within(got, ref, bnd):
    """got within bnd of ref wherever the bound is finite (a non-finite point may produce anything in what it touches)."""
    with np.errstate(all="ignore"):
        return (np.abs(np.asarray(got, dtype=_F64) - ref) <= bnd) | ~np.isfinite(bnd)


# ---- the 50-digit twin -----------------------------------------------------------------------------------------------------------
def _mp_point(kind, F, x, y, g, clamp_at, eps, mp):
    """One point at the working precision of mp: (values, gF[9], gx[3], gy[3]) as mpf lists.  g: 3 upstream values."""
    m = mp.mpf
    F = [m(float(v)) for v in np.asarray(F).reshape(9)]
    x, y, g = [m(float(v)) for v in x], [m(float(v)) for v in y], [m(float(v)) for v in g]
    a = [F[3 * r] * x[0] + F[3 * r + 1] * x[1] + F[3 * r + 2] * x[2] for r in range(3)]
    b = [F[c] * y[0] + F[3 + c] * y[1] + F[6 + c] * y[2] for c in range(3)]
    s = y[0] * a[0] + y[1] * a[1] + y[2] * a[2]
    A, Q = a[0] ** 2 + a[1] ** 2, b[0] ** 2 + b[1] ** 2
    sg = mp.sign(s)
    if kind == 0:
        e_ = m(float(np.float32(eps)))
        iA, iQ = 1 / (A + e_), 1 / (Q + e_)
        e = s * s * (iA + iQ)
        passes = clamp_at is None or e <= m(float(np.float32(clamp_at)))
        vals = [e if passes else m(float(np.float32(clamp_at)))]
        gg = g[0] if passes else m(0)
        cs, cA, cQ = gg * 2 * s * (iA + iQ), -gg * s * s * iA * iA, -gg * s * s * iQ * iQ
    elif kind == 1:
        iD = 1 / (A + Q)
        vals = [s * s * iD]
        cs, cA = g[0] * 2 * s * iD, -g[0] * s * s * iD * iD
        cQ = cA
    else:
        rA, rQ = mp.sqrt(A), mp.sqrt(Q)
        d1, d2 = abs(s) / rA, abs(s) / rQ
        vals = [(d1 + d2) / 2, d1, d2]
        h1, h2 = g[1] + g[0] / 2, g[2] + g[0] / 2
        cs, cA, cQ = sg * (h1 / rA + h2 / rQ), -h1 * abs(s) / (2 * A * rA), -h2 * abs(s) / (2 * Q * rQ)
    gF = [cs * y[r] * x[c] + (2 * cA * a[r] * x[c] if r < 2 else 0) + (2 * cQ * b[c] * y[r] if c < 2 else 0) for r in range(3) for c in range(3)]
    gx = [cs * b[c] + 2 * cA * (a[0] * F[c] + a[1] * F[3 + c]) for c in range(3)]
    gy = [cs * a[r] + 2 * cQ * (b[0] * F[3 * r] + b[1] * F[3 * r + 1]) for r in range(3)]
    return vals, gF, gx, gy


def _mp_residual_point(F, x1, x2, g, clamp_at, mp):
    m = mp.mpf
    F = [m(float(v)) for v in np.asarray(F).reshape(9)]
    x, y, g = [m(float(v)) for v in x1], [m(float(v)) for v in x2], m(float(g))
    a = [F[3 * r] * x[0] + F[3 * r + 1] * x[1] + F[3 * r + 2] * x[2] for r in range(3)]   # l2
    b = [F[c] * y[0] + F[3 + c] * y[1] + F[6 + c] * y[2] for c in range(3)]               # l1
    s = y[0] * a[0] + y[1] * a[1] + y[2] * a[2]
    n1, n2 = mp.sqrt(b[0] ** 2 + b[1] ** 2), mp.sqrt(a[0] ** 2 + a[1] ** 2)
    i1, i2 = 1 / (n1 + m(1e-6)), 1 / (n2 + m(1e-6))
    S = i1 + i2
    gg = g if abs(s) * S <= m(float(np.float32(clamp_at))) else m(0)
    k1 = abs(s) * i1 * i1 / n1 if n1 > 0 else m(0)
    k2 = abs(s) * i2 * i2 / n2 if n2 > 0 else m(0)
    sg = mp.sign(s)
    g1 = [gg * (sg * S * b[c] - k2 * (a[0] * F[c] + a[1] * F[3 + c])) for c in range(3)]
    g2 = [gg * (sg * S * a[r] - k1 * (b[0] * F[3 * r] + b[1] * F[3 * r + 1])) for r in range(3)]
    return g1, g2


def worst_ratio(got, exact, M, mp):
    """max |got - exact| / (2^-53 M) over the finite entries: got float64 array, exact a flat list of mpf, M float64 array."""
    worst = 0.0
    with mp.workdps(50):
        for gv, ev, mv in zip(np.asarray(got, dtype=_F64).ravel(), exact, np.asarray(M, dtype=_F64).ravel()):
            if not np.isfinite(mv) or not np.isfinite(gv):
                continue
            if mp.isnan(ev):  # the twin gives up on the whole point where one of its divisions is by zero
                continue
            err = abs(mp.mpf(float(gv)) - ev)
            if err == 0:
                continue
            if mv == 0.0:
                return np.inf
            worst = max(worst, float(err / (mp.mpf(U64) * mp.mpf(float(mv)))))
    return worst


def mp_metrics(kind, F, X, Y, homo, g, clamp_at=None, eps=0.0):
    """The twin of metrics_adjoint: dict of flat mpf lists in the order of value [P?,B,N], gF_pt [B,N,9], gX, gY [B,N,3]."""
    import mpmath as mp

    x, y = er._homo(X, homo), er._homo(Y, homo)
    g = np.asarray(g, dtype=_F64)
    g3 = g if kind == 2 else np.stack((g, np.zeros_like(g), np.zeros_like(g)))
    B, N = x.shape[:2]
    out = {"value": [[] for _ in range(3 if kind == 2 else 1)], "gF_pt": [], "gX": [], "gY": []}
    with mp.workdps(50):
        for b in range(B):
            for n in range(N):
                try:
                    v, gF, gx, gy = _mp_point(kind, F[b], x[b, n], y[b, n], g3[:, b, n], clamp_at, eps, mp)
                except ZeroDivisionError:
                    nan = mp.mpf("nan")
                    v, gF, gx, gy = [nan] * len(out["value"]), [nan] * 9, [nan] * 3, [nan] * 3
                for p, vv in enumerate(v):
                    out["value"][p].append(vv)
                out["gF_pt"] += gF
                out["gX"] += gx
                out["gY"] += gy
    out["value"] = [v for plane in out["value"] for v in plane]
    return out


def mp_residual(pts1, pts2, F, clamp_at, g):
    import mpmath as mp

    out = {"g1": [], "g2": []}
    B, N = np.asarray(pts1).shape[:2]
    with mp.workdps(50):
        for b in range(B):
            for n in range(N):
                g1, g2 = _mp_residual_point(F[b], pts1[b, n], pts2[b, n], np.asarray(g)[b, n], clamp_at, mp)
                out["g1"] += g1
                out["g2"] += g2
    return out
