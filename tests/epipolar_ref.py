"""The clamped symmetric epipolar distance and its adjoint with respect to F, restated per point in numpy float64.

Written from the reference's lines, not from the kernels:
  utils_F.py:400-413 (compute_epi_residual)      l1 = pts2 @ F, l2 = pts1 @ F^T, dd = sum(pts1 * l1),
                                                 d = |dd| (1 / (|l1[:2]| + 1e-6) + 1 / (|l2[:2]| + 1e-6)), out = clamp(d, max=clamp_at)
  train_good_utils.py:325-326                    pts*_eval = T* @ virt*^T          (an fp32 tensor: rounded once)
  train_good_utils.py:340-342, 352               losses = compute_epi_residual(pts1_eval, pts2_eval, F_l, clamp_at), their mean
  train_good_utils.py:356-358                    E_l = K^T T2^T F_l T1 K
  utils_F.py:291-361                             _sampson_dist, _sym_epi_dist, _epi_distance (the metrics at the end of this file)
It is the one yardstick of the four kernels that compute this quantity: floss_kernel (csrc/floss.hip), tail_floss_row
(csrc/loss_tail_body.h), epi_residual_kernel and epi_metrics_kernel (csrc/geom.hip).  No torch in here.

Inputs are what the kernels see: float32 F_layers [L,B,3,3], float32 T1 / T2 ([3,3] shared or [B,3,3] per pair), float32 K [B,3,3],
float32 homogeneous pixel points [B,M,3], clamp_at (rounded to float32), upstream weights.  The transformed points are float32(T v) with the product
formed in float64 -- the reference's pts_eval is an fp32 tensor and the kernels round once in the same place -- so both sides start
from identical points.

Conventions of the restatement (where the reference's autograd has a choice, the line it follows):
  * gate: the gradient passes where d <= clamp_at (utils_F.py:411, torch.clamp(max=) passes the gradient AT the bound);
  * sign(0) = 0 (utils_F.py:407, the derivative torch gives dd.abs() at dd = 0);
  * k1 = 0 where n1 = 0, k2 = 0 where n2 = 0 (utils_F.py:407, the subgradient torch gives norm(2, 2) at the zero vector);
  * the forward value of a NaN distance stays NaN under the clamp (torch.clamp propagates NaN; utils_F.py:336-337).

Per point, with x1 = float32(T1 v1), x2 = float32(T2 v2), l1 = F^T x2, l2 = F x1, n1 = |l1[:2]|, n2 = |l2[:2]|, i = 1 / (n + 1e-6):
  dd = x2^T F x1,  S = i1 + i2,  d = |dd| S,  A = sum_rc |x2_r| |F_rc| |x1_c|  (the condition number of dd: fp32 evaluates dd to
  about 2^-24 A whatever the order),
  d d / d F_rc = sign(dd) S x2_r x1_c  -  k1 l1_c x2_r [c<2]  -  k2 l2_r x1_c [r<2],   k1 = |dd| i1^2 / n1,  k2 = |dd| i2^2 / n2,
  mag_rc = the same three terms with absolute values and with A in place of |dd| in k1 and k2 (what one fp32 rounding of dd, of a
  norm or of a product moves the entry by, in units of 2^-24),
  cmax_rc = the three terms with absolute values (an upper bound of |d d / d F_rc|).

Bounds (c in units of 2^-24; `u` below is 2^-24 for the fp32 kernels):
  bound_fwd(c)     = c u (A S + d)                                              per point
  bound_grad(c, G) = c u sum_live G mag_rc  +  sum_flagged G w cmax_rc          per (layer, pair, entry)
A point is flagged when an fp32 evaluation may take the other branch: near_gate (|d - clamp_at| <= bound_fwd) or sign_uncertain
(|dd| <= c u A, A > 0).  A flagged point is never left out of a sum: the reference keeps it with its float64 branch and its whole possible
contribution (w = 1 near the gate: in or out; w = 2 at an uncertain sign: + or -) widens the bound of the entries it touches.

The two constants.  They are not chosen: tests/test_epipolar_ref_cpu.py evaluates the oracle in torch float32 on the CPU, forward
and autograd, on every shared case of tests/epipolar_cases.py and takes the smallest c that holds it.  Measured there:
  forward  C_FWD_MEASURED  = 1.8   (per-point distances and per-pair sums)
  gradient C_GRAD_MEASURED = 12.0  (d sum / d F per layer and pair)
The bounds used everywhere are 4 x those values, the margin tests/test_refcfg_gpu.py gives the reference's own float32 run; it covers
the 1-ulp hardware rcp / sqrt, the fma contraction and the DPP tree sums, none of which torch's CPU path has.  The CPU test asserts that
the float32 oracle sits inside a quarter of the bound.
Flagged points over the shared cases, at the bands of C_FWD: see FLAGGED_NOTE below (at most 1 % of the points of any case)."""
import numpy as np

U32 = 2.0 ** -24
C_FWD_MEASURED = 1.8
C_GRAD_MEASURED = 12.0
C_FWD = 4 * C_FWD_MEASURED
C_GRAD = 4 * C_GRAD_MEASURED
FLAGGED_NOTE = "shared cases (the unperturbed one apart): 0 near-gate and 0..2 sign-uncertain points per case, 0 + 2 of 118 042 points in all"

_F64 = np.float64


def per_pair(T, B):
    """[3,3] (shared) or [B,3,3] -> float64 [B,3,3]."""
    T = np.asarray(T, dtype=_F64)
    if T.ndim == 2:
        T = np.broadcast_to(T, (B, 3, 3))
    assert T.shape == (B, 3, 3), T.shape
    return T


def transform_points(T, v):
    """float32(T v), the product in float64 (train_good_utils.py:325-326).  T [3,3] or [B,3,3], v [B,M,3] float32."""
    v = np.asarray(v)
    assert v.dtype == np.float32
    T = per_pair(T, v.shape[0])
    return np.einsum("brc,bmc->bmr", T, v.astype(_F64)).astype(np.float32)


class PointTerms:
    """Everything per (layer, pair, point); arrays [L,B,M] and [L,B,M,3,3]."""

    def flags(self, c=C_FWD, u=U32):
        near_gate = np.abs(self.d - self.clamp_at) <= c * u * (self.A * self.S + self.d)
        sign_uncertain = (np.abs(self.dd) <= c * u * self.A) & (self.A > 0)  # A = 0: every product of dd is exactly 0 in any format
        return near_gate, sign_uncertain

    def bound_fwd(self, c=C_FWD, u=U32):
        return c * u * (self.A * self.S + self.d)


def point_terms(F, x1, x2, clamp_at):
    """F [L,B,3,3] (any float), x1 / x2 [B,M,3] already transformed: the per-point quantities of utils_F.py:402-411 in float64."""
    F = np.asarray(F, dtype=_F64)
    x1, x2 = np.asarray(x1, dtype=_F64), np.asarray(x2, dtype=_F64)
    p = PointTerms()
    p.clamp_at = float(np.float32(clamp_at))  # the float32 the kernels are given
    p.x1, p.x2 = x1, x2
    l1 = np.einsum("bmr,lbrc->lbmc", x2, F)   # pts2 @ F: rows F^T x2       (:402)
    l2 = np.einsum("bmc,lbrc->lbmr", x1, F)   # pts1 @ F^T: rows F x1       (:403)
    p.l1, p.l2 = l1, l2
    p.dd = (x1[None] * l1).sum(-1)            # (:405)
    p.n1 = np.sqrt(l1[..., 0] ** 2 + l1[..., 1] ** 2)
    p.n2 = np.sqrt(l2[..., 0] ** 2 + l2[..., 1] ** 2)
    i1, i2 = 1.0 / (p.n1 + 1e-6), 1.0 / (p.n2 + 1e-6)
    p.S = i1 + i2
    ad = np.abs(p.dd)
    p.d = ad * p.S                            # (:407)
    p.out = np.minimum(p.d, p.clamp_at)       # (:411)
    p.A = np.einsum("bmr,lbrc,bmc->lbm", np.abs(x2), np.abs(F), np.abs(x1))
    p.gate = p.d <= p.clamp_at                # convention: torch.clamp(max=) passes the gradient at the bound
    sg = np.sign(p.dd)                        # convention: sign(0) = 0
    with np.errstate(divide="ignore", invalid="ignore"):
        r1 = np.where(p.n1 > 0, i1 * i1 / p.n1, 0.0)   # convention: k1 = 0 where n1 = 0
        r2 = np.where(p.n2 > 0, i2 * i2 / p.n2, 0.0)
    cmask = np.array([1.0, 1.0, 0.0])
    x2r, x1c = x2[None, :, :, :, None], x1[None, :, :, None, :]
    t1 = (l1 * cmask)[..., None, :] * x2r      # l1_c x2_r [c<2]
    t2 = (l2 * cmask)[..., :, None] * x1c      # l2_r x1_c [r<2]
    t0 = x2r * x1c
    e = lambda a: a[..., None, None]
    p.dF = e(sg * p.S) * t0 - e(ad * r1) * t1 - e(ad * r2) * t2
    p.cmax = e(p.S) * np.abs(t0) + e(ad * r1) * np.abs(t1) + e(ad * r2) * np.abs(t2)
    p.mag = e(p.S) * np.abs(t0) + e(p.A * r1) * np.abs(t1) + e(p.A * r2) * np.abs(t2)
    return p


class Ref:
    """Per (layer, pair): loss_sum [L,B], E [L,B,3,3] (None without K), and g_F(...) / bound_grad(...)."""

    def sums(self):
        """d loss_sum / d F per (layer, pair) [L,B,3,3]: the gated sum of the per-point derivatives."""
        return (self.pt.dF * self.pt.gate[..., None, None]).sum(2)

    def g_F(self, g_loss_sum=None, g_E=None):
        g = np.zeros(self.F.shape, dtype=_F64)
        if g_loss_sum is not None:
            g = g + np.broadcast_to(np.asarray(g_loss_sum, dtype=_F64), self.F.shape[:2])[..., None, None] * self.sums()
        if g_E is not None:  # E = A^T F C  ->  g_F += A g_E C^T
            g = g + np.einsum("bij,lbjk,bmk->lbim", self.A2, np.asarray(g_E, dtype=_F64), self.C1)
        return g

    def bound_loss_sum(self, c=C_FWD, u=U32):
        return self.pt.bound_fwd(c, u).sum(2)

    def bound_grad(self, c=C_GRAD, G=1.0, u=U32, c_flag=C_FWD, u_flag=U32):
        """[L,B,3,3].  G: |upstream weight| per (layer, pair) (scalar or [L,B]), or per point [L,B,M]."""
        p = self.pt
        G = np.abs(np.asarray(G, dtype=_F64))
        G = np.broadcast_to(G if G.ndim == 3 else np.broadcast_to(G, self.F.shape[:2])[..., None], p.d.shape)[..., None, None]
        near, sgn = p.flags(c_flag, u_flag)
        flagged = near | sgn
        live = (p.gate | flagged)[..., None, None]
        w = np.where(sgn, 2.0, 1.0) * flagged
        return (c * u * G * live * p.mag).sum(2) + (G * w[..., None, None] * p.cmax).sum(2)

    def bound_contribution(self, G=1.0):
        """sum G cmax: what |g_F| cannot exceed whatever branch every point takes."""
        G = np.broadcast_to(np.abs(np.asarray(G, dtype=_F64)), self.F.shape[:2])[..., None, None]
        return G * self.pt.cmax.sum(2)

    def flagged(self, c=C_FWD, u=U32):
        return self.pt.flags(c, u)


def floss_ref(F_layers, T1, T2, K, virt1, virt2, clamp_at):
    """The per-layer body of get_all_loss_DeepF (train_good_utils.py:325-358) on float32 inputs, in float64."""
    F_layers = np.asarray(F_layers)
    assert F_layers.dtype == np.float32 and F_layers.ndim == 4
    B = F_layers.shape[1]
    r = Ref()
    r.F = F_layers.astype(_F64)
    r.x1, r.x2 = transform_points(T1, virt1), transform_points(T2, virt2)
    r.pt = point_terms(r.F, r.x1, r.x2, clamp_at)
    r.loss_sum = r.pt.out.sum(2)
    r.E = None
    if K is not None:
        K = per_pair(K, B)
        r.A2, r.C1 = per_pair(T2, B) @ K, per_pair(T1, B) @ K
        r.E = np.einsum("bji,lbjk,bkm->lbim", r.A2, r.F, r.C1)   # (T2 K)^T F (T1 K)   (:356-358)
        nrm = lambda a: np.sqrt((a ** 2).sum((-1, -2)))
        r.E_scale = nrm(r.A2)[None] * nrm(r.F) * nrm(r.C1)[None]  # [L,B]
    return r


def residual_ref(pts1, pts2, F, clamp_at):
    """compute_epi_residual (utils_F.py:400-413) on float32 points [B,N,3] used as they are and float32 F [B,3,3]: a Ref with one
    layer; .out [B,N] is the clamped distance, g_F_points(g) the adjoint for a per-point upstream g [B,N]."""
    F = np.asarray(F)
    assert F.dtype == np.float32 and np.asarray(pts1).dtype == np.float32
    r = Ref()
    r.F = F.astype(_F64)[None]
    r.pt = point_terms(r.F, pts1, pts2, clamp_at)
    r.out = r.pt.out[0]
    r.loss_sum = r.pt.out.sum(2)
    r.E = None
    return r


def g_F_points(r, g):
    """sum_i g_i gate_i d d_i / d F  [B,3,3] for a per-point upstream g [B,N]."""
    g = np.asarray(g, dtype=_F64)[None]
    return (r.pt.dF * (r.pt.gate * g)[..., None, None]).sum(2)[0]


# ---- the 2-D / homogeneous metrics of utils_F.py:291-361 -------------------------------------------------------------------------
def _homo(X, homo):
    X = np.asarray(X, dtype=_F64)
    return X if homo else np.concatenate((X, np.ones(X.shape[:-1] + (1,))), -1)


def _metric_terms(F, X, Y, homo):
    F = np.asarray(F, dtype=_F64)
    X, Y = _homo(X, homo), _homo(Y, homo)
    Fx = np.einsum("brc,bnc->bnr", F, X)     # F x      (:302, :325, :354)
    Fty = np.einsum("brc,bnr->bnc", F, Y)    # F^T y    (:303, :328, :355)
    num = (Y * Fx).sum(-1)                   # y^T F x  (:301)
    return num, Fx[..., 0] ** 2 + Fx[..., 1] ** 2, Fty[..., 0] ** 2 + Fty[..., 1] ** 2


def sym_epi(F, X, Y, homo=False, clamp_at=None, eps=0.0):
    """_sym_epi_dist (:310-339), squared; eps is the 1e-10 of the batched branch (:329), taken as the float32 the kernel is given.
    A NaN stays NaN under the clamp (torch.clamp)."""
    num, a, b = _metric_terms(F, X, Y, homo)
    eps = float(np.float32(eps))
    with np.errstate(divide="ignore", invalid="ignore"):
        e = num ** 2 * (1.0 / (a + eps) + 1.0 / (b + eps))
        if clamp_at is not None:
            cl = float(np.float32(clamp_at))  # the float32 the kernel is given
            e = np.where(e > cl, cl, e)
    return e


def sampson(F, X, Y, homo=False):
    """_sampson_dist (:291-308)."""
    num, a, b = _metric_terms(F, X, Y, homo)
    with np.errstate(divide="ignore", invalid="ignore"):
        return num ** 2 / (a + b)


def epi_distance(F, X, Y, homo=False):
    """_epi_distance (:341-361): [3,B,N] = (d1 + d2) / 2, d1 (y to F x), d2 (x to F^T y)."""
    num, a, b = _metric_terms(F, X, Y, homo)
    with np.errstate(divide="ignore", invalid="ignore"):
        d1, d2 = np.abs(num) / np.sqrt(a), np.abs(num) / np.sqrt(b)
        return np.stack(((d1 + d2) / 2.0, d1, d2))


# ---- the two bounds as plain functions -------------------------------------------------------------------------------------------
def bound_fwd(p, c=C_FWD):
    """c 2^-24 (A S + d) per point, for a PointTerms or a Ref."""
    return (p.pt if isinstance(p, Ref) else p).bound_fwd(c)


def bound_grad(r, c=C_GRAD, G=1.0):
    """c 2^-24 sum_live G mag_rc + sum_flagged G |contribution_rc| per (layer, pair, entry) of a Ref."""
    return r.bound_grad(c, G)
