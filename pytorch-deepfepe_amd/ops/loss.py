"""The losses on the fitted F: F-loss, pose errors, their batch statistics and the fused tail (csrc/floss.hip, pose.hip,
loss_tail.hip)."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from ._base import Tensor, _on, _prep, _ptr, _shape, _stream
from .fit import row_of


# ------------------------------------------------------------------------------------------------
# F-loss (virtual-point epipolar residual sums per layer and pair) and E-from-F
# ------------------------------------------------------------------------------------------------
def _t_arg(T: Tensor, B: int):
    """T given as [3,3] / [1,3,3] (shared) or [B,3,3]; expanded (stride-0) views are collapsed to shared."""
    if T.dim() == 2:
        return _prep(T, "T"), 0
    if T.shape[0] == 1 or (T.stride(0) == 0):
        return _prep(T[0], "T"), 0
    assert T.shape[0] == B
    return _prep(T, "T"), 9


class _FlossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, F_layers, T1, T2, K, virt1, virt2, clamp_at):
        lib = _lib.lib()
        L, B = F_layers.shape[0], F_layers.shape[1]
        M = virt1.shape[1]
        T1c, st1 = _t_arg(T1, B)
        T2c, st2 = _t_arg(T2, B)
        if st1 != st2:
            T1c, T2c, st1 = T1c.expand(B, 3, 3).contiguous(), T2c.expand(B, 3, 3).contiguous(), 9
        loss_sum = torch.empty(L, B, device=F_layers.device, dtype=torch.float32)
        E_layers = torch.empty(L, B, 3, 3, device=F_layers.device, dtype=torch.float32)
        with _on(F_layers.device):
            rc = lib.dfepe_floss_fwd(_ptr(F_layers), L, B, _ptr(T1c), _ptr(T2c), st1, _ptr(K), _ptr(virt1), _ptr(virt2), M,
                                     float(clamp_at), _ptr(loss_sum), _ptr(E_layers), _stream())
        _lib.check(rc, "dfepe_floss_fwd")
        ctx.save_for_backward(F_layers, T1c, T2c, K, virt1, virt2)
        ctx.cfg = (st1, float(clamp_at))
        return loss_sum, E_layers

    @staticmethod
    def backward(ctx, g_loss_sum, g_E):
        F_layers, T1c, T2c, K, virt1, virt2 = ctx.saved_tensors
        st, clamp_at = ctx.cfg
        lib = _lib.lib()
        L, B = F_layers.shape[0], F_layers.shape[1]
        gF = torch.empty_like(F_layers)
        g_loss_sum = None if g_loss_sum is None else g_loss_sum.contiguous().float()
        g_E = None if g_E is None else g_E.contiguous().float()
        with _on(F_layers.device):
            rc = lib.dfepe_floss_bwd(_ptr(F_layers), L, B, _ptr(T1c), _ptr(T2c), st, _ptr(K), _ptr(virt1), _ptr(virt2),
                                     virt1.shape[1], clamp_at, _ptr(g_loss_sum), 0.0, None, _ptr(g_E), _ptr(gF), _stream())
        _lib.check(rc, "dfepe_floss_bwd")
        return gF, None, None, None, None, None, None


def floss(F_layers: Tensor, T1: Tensor, T2: Tensor, K: Tensor, virt1: Tensor, virt2: Tensor, clamp_at: float):
    """F_layers [L,B,3,3] -> (loss_sum [L,B] = sum over virtual points of the clamped residual, E_layers [L,B,3,3])."""
    F_layers, K, virt1, virt2 = _prep(F_layers, "F_layers"), _prep(K, "K"), _prep(virt1, "virt1"), _prep(virt2, "virt2")
    _shape(F_layers, "F_layers", None, None, 3, 3)
    B = F_layers.shape[1]
    _shape(K, "K (one intrinsic matrix per pair)", B, 3, 3)
    _shape(virt1, "virt1 (homogeneous pixel points)", B, None, 3)
    _shape(virt2, "virt2", B, virt1.shape[1], 3)
    for T in (T1, T2):
        if not ((T.dim() == 2 and tuple(T.shape) == (3, 3)) or (T.dim() == 3 and T.shape[0] in (1, B) and tuple(T.shape[1:]) == (3, 3))):
            raise ValueError(f"T1/T2 must be [3,3], [1,3,3] or [{B},3,3], got {tuple(T.shape)}")
    return _FlossFunction.apply(F_layers, T1, T2, K, virt1, virt2, clamp_at)


# ------------------------------------------------------------------------------------------------
# pose loss
# ------------------------------------------------------------------------------------------------
def _sum_opt(a: Optional[Tensor], b: Optional[Tensor]) -> Optional[Tensor]:
    if a is None:
        return b
    return a if b is None else a + b


class _PoseFunction(torch.autograd.Function):
    """Outputs: qt [2,L,B] (q_l2 | t_l2 in one buffer, so that one reduction serves both), its two halves q_l2, t_l2 [L,B] as
    outputs of their own over the same memory, ang [2,L,B] = R_deg | t_deg and sel [L,B] (not differentiable)."""

    @staticmethod
    def forward(ctx, E_layers, q_gt, t_gt, R_gt):
        lib = _lib.lib()
        L, B = E_layers.shape[0], E_layers.shape[1]
        dev = E_layers.device
        ctx.set_materialize_grads(False)
        qt = torch.empty(2, L, B, device=dev, dtype=torch.float32)
        ang = torch.empty(2, L, B, device=dev, dtype=torch.float32)
        sel = torch.empty(L, B, device=dev, dtype=torch.int32)
        q_l2, t_l2 = row_of(qt, 0), row_of(qt, 1)
        with _on(dev):
            rc = lib.dfepe_pose_fwd(_ptr(E_layers), L, B, _ptr(q_gt), _ptr(t_gt), _ptr(R_gt), _ptr(q_l2), _ptr(t_l2),
                                    _ptr(ang[0]), _ptr(ang[1]), _ptr(sel), _stream())
        _lib.check(rc, "dfepe_pose_fwd")
        ctx.save_for_backward(E_layers, q_gt, t_gt)
        ctx.mark_non_differentiable(ang, sel)
        return qt, q_l2, t_l2, ang, sel

    @staticmethod
    def backward(ctx, g_qt, g_q, g_t, _a, _b):
        E_layers, q_gt, t_gt = ctx.saved_tensors
        lib = _lib.lib()
        L, B = E_layers.shape[0], E_layers.shape[1]
        if g_qt is not None:
            g_qt = g_qt.contiguous().float()
            g_q, g_t = _sum_opt(g_q, g_qt[0]), _sum_opt(g_t, g_qt[1])
        if g_q is None and g_t is None:
            return None, None, None, None
        gE = torch.empty_like(E_layers)
        g_q = None if g_q is None else g_q.contiguous().float()
        g_t = None if g_t is None else g_t.contiguous().float()
        with _on(E_layers.device):
            rc = lib.dfepe_pose_bwd(_ptr(E_layers), L, B, _ptr(q_gt), _ptr(t_gt), _ptr(g_q), _ptr(g_t), 0.0, 0.0, 0.0, 0.0, None,
                                    _ptr(gE), _stream())
        _lib.check(rc, "dfepe_pose_bwd")
        return gE, None, None, None


def _pose_args(E_layers: Tensor, q_gt: Tensor, t_gt: Tensor, R_gt: Tensor):
    _shape(E_layers, "E_layers", None, None, 3, 3)
    B = E_layers.shape[1]
    if q_gt.numel() != 4 * B or t_gt.numel() != 3 * B or R_gt.numel() != 9 * B:
        raise ValueError(f"q_gt / t_gt / R_gt must hold {B} quaternions / translations / rotations, got {tuple(q_gt.shape)}, {tuple(t_gt.shape)}, {tuple(R_gt.shape)}")
    return _prep(E_layers, "E_layers"), _prep(q_gt.reshape(B, 4), "q_gt"), _prep(t_gt.reshape(B, 3), "t_gt"), _prep(R_gt.reshape(B, 3, 3), "R_gt")


def pose_errors(E_layers: Tensor, q_gt: Tensor, t_gt: Tensor, R_gt: Tensor):
    """E_layers [L,B,3,3]; q_gt [B,4(,1)], t_gt [B,3(,1)], R_gt [B,3,3] (camera motion).
    Returns q_l2, t_l2 (differentiable w.r.t. E), R_deg, t_deg, sel — all [L,B]."""
    _, q_l2, t_l2, ang, sel = _PoseFunction.apply(*_pose_args(E_layers, q_gt, t_gt, R_gt))
    return q_l2, t_l2, ang[0], ang[1], sel


def pose_errors_packed(E_layers: Tensor, q_gt: Tensor, t_gt: Tensor, R_gt: Tensor):
    """As pose_errors, returning the buffers the kernel filled: (qt [2,L,B] = q_l2 | t_l2, q_l2, t_l2, ang [2,L,B] = R_deg | t_deg,
    sel); qt, q_l2 and t_l2 are differentiable and share memory."""
    return _PoseFunction.apply(*_pose_args(E_layers, q_gt, t_gt, R_gt))


def _slice_of(buf: Tensor, off: int, n: int) -> Tensor:
    """buf[off:off+n] of a contiguous 1-D buffer as a tensor of its own over the same memory (not an autograd view)."""
    t = torch.empty(0, dtype=buf.dtype, device=buf.device)
    t.set_(buf.untyped_storage(), buf.storage_offset() + off, (n,), None)
    return t


def _stats_launch(sets, C: int, want_min: bool):
    """sets: four (tensor [R,C] | None, scale).  One dfepe_loss_stats launch -> (per set: (means [R_k], overall [] scalar) over one
    buffer, or (None, None); row_min; col_min)."""
    dev = next(x for x, _ in sets if x is not None).device
    total = sum(x.shape[0] + 1 for x, _ in sets if x is not None)
    out = torch.empty(total, device=dev, dtype=torch.float32)
    x0 = sets[0][0]
    row_min = torch.empty(x0.shape[0], device=dev, dtype=torch.float32) if want_min else None
    col_min = torch.empty(C, device=dev, dtype=torch.float32) if want_min else None
    args = []
    for x, sc in sets:
        args += [_ptr(x), 0 if x is None else x.shape[0], float(sc)]
    with _on(dev):
        rc = _lib.lib().dfepe_loss_stats(*args, C, _ptr(out), _ptr(row_min), _ptr(col_min), _stream())
    _lib.check(rc, "dfepe_loss_stats")
    blocks, off = [], 0
    for x, _ in sets:
        if x is None:
            blocks.append((None, None))
        else:
            R = x.shape[0]
            blocks.append((_slice_of(out, off, R), _slice_of(out, off + R, 1).view(())))
            off += R + 1
    return blocks, row_min, col_min


def _stat_block_grad(gm: Optional[Tensor], go: Optional[Tensor], R: int, C: int, scale: float) -> Optional[Tensor]:
    """Gradient w.r.t. the [R,C] rows of a dfepe_loss_stats set from the gradients of its R row means and of their mean."""
    if gm is None and go is None:
        return None
    coef = _sum_opt(gm, None if go is None else (go * (1.0 / R)).reshape(1).expand(R)) * (scale / C)
    return coef.unsqueeze(1).expand(R, C)


class _LossStatsFunction(torch.autograd.Function):
    """dfepe_loss_stats as a differentiable op on up to four [R_k, C] row sets (set 0 optionally with its minima, which carry no
    gradient).  Outputs: (means [R_k], overall scalar) per set (None, None for absent sets), then row_min, col_min."""

    @staticmethod
    def forward(ctx, want_min, x0, s0, x1, s1, x2, s2, x3, s3):
        ctx.set_materialize_grads(False)
        sets = [(x0, s0), (x1, s1), (x2, s2), (x3, s3)]
        C = x0.shape[1]
        ctx.meta = [(None if x is None else x.shape[0], float(sc)) for x, sc in sets]
        ctx.C = C
        blocks, row_min, col_min = _stats_launch(sets, C, want_min)
        if want_min:
            ctx.mark_non_differentiable(row_min, col_min)
        return tuple(t for blk in blocks for t in blk) + (row_min, col_min)

    @staticmethod
    def backward(ctx, *gs):
        out = [None]
        for k, (R, sc) in enumerate(ctx.meta):
            out += [None if R is None else _stat_block_grad(gs[2 * k], gs[2 * k + 1], R, ctx.C, sc), None]
        return tuple(out)


def loss_stats(sets, want_min: bool = False):
    """sets: up to four (x [R,C], scale) pairs (None for an absent set), the first one present.  Returns (blocks, row_min, col_min):
    blocks[k] = (means [R_k] = scale_k * mean over C of every row, overall = the mean of those) or (None, None); the minima
    (set 0, times scale_0, no gradient) only with want_min."""
    sets = list(sets) + [None] * (4 - len(sets))
    flat = []
    C = sets[0][0].shape[1]
    for s in sets:
        if s is None:
            flat += [None, 0.0]
        else:
            x = _prep(s[0], "rows")
            _shape(x, "rows", None, C)
            flat += [x, float(s[1])]
    res = _LossStatsFunction.apply(bool(want_min), *flat)
    return [(res[2 * k], res[2 * k + 1]) for k in range(4)], res[8], res[9]


class _TailJacFunction(torch.autograd.Function):
    """get_all_loss_DeepF's per-layer body and get_Rt_loss's loop as ONE launch (dfepe_loss_tail_jac) plus ONE for every batch
    statistic the two functions return (dfepe_loss_stats), with a one-launch adjoint for whatever upstream gradients arrive
    (dfepe_loss_tail_bwd): the reference's callers mix clamps and balances themselves (Train_model_pipeline.py:580-586), so no
    coefficient is baked in.  Outputs (None where absent): loss_sum [L,B], E_layers [L,B,3,3], m_loss [L] / o_loss [] (per-layer
    means of loss_sum / M and loss_F), row_min [L], col_min [B] (loss_min_layers / loss_min_batch), m_x / o_x (statistics of the
    optional fourth row set ``extra`` [n,B]), and -- with ground truth -- qt [2,L,B], q_l2, t_l2, ang [2,L,B], sel as in
    _PoseFunction, m_q / o_q, m_t / o_t."""

    @staticmethod
    def forward(ctx, F_layers, T1c, T2c, t_stride, K, virt1, virt2, clamp_at, q_gt, t_gt, R_gt, want_floss_jac, extra, extra_scale):
        lib = _lib.lib()
        L, B = F_layers.shape[0], F_layers.shape[1]
        M = virt1.shape[1]
        dev = F_layers.device
        ctx.set_materialize_grads(False)
        loss_sum = torch.empty(L, B, device=dev, dtype=torch.float32)
        E_layers = torch.empty(L, B, 3, 3, device=dev, dtype=torch.float32)
        J = torch.empty(L, B, 27, device=dev, dtype=torch.float32)
        pose = q_gt is not None
        qt = torch.empty(2, L, B, device=dev, dtype=torch.float32) if pose else None
        ang = torch.empty(2, L, B, device=dev, dtype=torch.float32) if pose else None
        sel = torch.empty(L, B, device=dev, dtype=torch.int32) if pose else None
        q_l2 = row_of(qt, 0) if pose else None
        t_l2 = row_of(qt, 1) if pose else None
        with _on(dev):
            rc = lib.dfepe_loss_tail_jac(_ptr(F_layers), L, B, _ptr(T1c), _ptr(T2c), t_stride, _ptr(K), _ptr(virt1), _ptr(virt2), M,
                                         float(clamp_at), _ptr(q_gt), _ptr(t_gt), _ptr(R_gt), 1 if want_floss_jac else 0, _ptr(loss_sum),
                                         _ptr(E_layers), _ptr(q_l2), _ptr(t_l2), _ptr(ang[0]) if pose else None,
                                         _ptr(ang[1]) if pose else None, _ptr(sel), _ptr(J), _stream())
        _lib.check(rc, "dfepe_loss_tail_jac")
        ((m_loss, o_loss), (m_q, o_q), (m_t, o_t), (m_x, o_x)), row_min, col_min = _stats_launch(
            [(loss_sum, 1.0 / M), (q_l2, 1.0), (t_l2, 1.0), (extra, extra_scale)], B, True)
        ctx.save_for_backward(J, F_layers, T1c, T2c, K, virt1, virt2)
        ctx.cfg = (t_stride, float(clamp_at), bool(want_floss_jac), 1.0 / M, None if extra is None else (extra.shape[0], float(extra_scale)))
        ctx.mark_non_differentiable(*([row_min, col_min] + ([ang, sel] if pose else [])))  # ONE call: a second one replaces the first
        return loss_sum, E_layers, m_loss, o_loss, row_min, col_min, m_x, o_x, qt, q_l2, t_l2, ang, sel, m_q, o_q, m_t, o_t

    @staticmethod
    def backward(ctx, g_loss_sum, g_E, gm_loss, go_loss, _rm, _cm, gm_x, go_x, g_qt, g_q, g_t, _a, _b, gm_q, go_q, gm_t, go_t):
        J, F_layers, T1c, T2c, K, virt1, virt2 = ctx.saved_tensors
        t_stride, clamp_at, want_floss_jac, loss_scale, extra_meta = ctx.cfg
        lib = _lib.lib()
        L, B = J.shape[0], J.shape[1]
        if g_qt is not None:
            g_qt = g_qt.contiguous().float()
            g_q, g_t = _sum_opt(g_q, g_qt[0]), _sum_opt(g_t, g_qt[1])
        g_extra = None if extra_meta is None else _stat_block_grad(gm_x, go_x, extra_meta[0], B, extra_meta[1])
        if all(g is None for g in (g_loss_sum, g_E, g_q, g_t, gm_loss, go_loss, gm_q, go_q, gm_t, go_t)):
            return (None,) * 12 + (g_extra, None)
        if (g_loss_sum is not None or gm_loss is not None or go_loss is not None) and not want_floss_jac:
            raise _lib.DfepeError("the F-loss Jacobian was switched off for this call (loss_params['floss_grad'] = False) but a gradient "
                                  "arrived on loss_F / loss_layers")
        c = lambda g: None if g is None else g.contiguous().float()
        gF = torch.empty(L, B, 3, 3, device=J.device, dtype=torch.float32)
        with _on(J.device):
            rc = lib.dfepe_loss_tail_bwd(_ptr(J), L, B, _ptr(c(g_loss_sum)), _ptr(c(g_q)), _ptr(c(g_t)), _ptr(c(gm_loss)), _ptr(c(go_loss)),
                                         _ptr(c(gm_q)), _ptr(c(go_q)), _ptr(c(gm_t)), _ptr(c(go_t)), float(loss_scale), _ptr(gF), _stream())
            _lib.check(rc, "dfepe_loss_tail_bwd")
            if g_E is not None:  # a gradient on the E matrices themselves (none of the reference's losses has one): the stand-alone adjoint
                gF2 = torch.empty_like(gF)
                rc = lib.dfepe_floss_bwd(_ptr(F_layers), L, B, _ptr(T1c), _ptr(T2c), t_stride, _ptr(K), _ptr(virt1), _ptr(virt2),
                                         virt1.shape[1], clamp_at, None, 0.0, None, _ptr(c(g_E)), _ptr(gF2), _stream())
                _lib.check(rc, "dfepe_floss_bwd")
                gF = gF + gF2
        return (gF,) + (None,) * 11 + (g_extra, None)


def _floss_args(F_layers, T1, T2, K, virt1, virt2):
    F_layers, K, virt1, virt2 = _prep(F_layers, "F_layers"), _prep(K, "K"), _prep(virt1, "virt1"), _prep(virt2, "virt2")
    _shape(F_layers, "F_layers", None, None, 3, 3)
    B = F_layers.shape[1]
    _shape(K, "K (one intrinsic matrix per pair)", B, 3, 3)
    _shape(virt1, "virt1 (homogeneous pixel points)", B, None, 3)
    _shape(virt2, "virt2", B, virt1.shape[1], 3)
    for T in (T1, T2):
        if not ((T.dim() == 2 and tuple(T.shape) == (3, 3)) or (T.dim() == 3 and T.shape[0] in (1, B) and tuple(T.shape[1:]) == (3, 3))):
            raise ValueError(f"T1/T2 must be [3,3], [1,3,3] or [{B},3,3], got {tuple(T.shape)}")
    T1c, st1 = _t_arg(T1, B)
    T2c, st2 = _t_arg(T2, B)
    if st1 != st2:
        T1c, T2c, st1 = T1c.expand(B, 3, 3).contiguous(), T2c.expand(B, 3, 3).contiguous(), 9
    return F_layers, T1c, T2c, st1, K, virt1, virt2


def loss_tail_jac(F_layers: Tensor, T1: Tensor, T2: Tensor, K: Tensor, virt1: Tensor, virt2: Tensor, clamp_at: float,
                  q_gt: Optional[Tensor] = None, t_gt: Optional[Tensor] = None, R_gt: Optional[Tensor] = None, floss_grad: bool = True,
                  extra: Optional[Tensor] = None, extra_scale: float = 1.0) -> dict:
    """F-loss sums + E-from-F (+ pose errors when the ground truth is given) of every layer in one launch and every batch
    statistic of them in a second one, differentiable for any upstream gradients.  Returns a dict: loss_sum [L,B], E_layers,
    m_loss [L] / o_loss (per-layer means of loss_sum / M, their mean), row_min [L], col_min [B], m_extra / o_extra (statistics of the
    optional row set ``extra`` [n,B], times extra_scale) and, with ground truth, qt, q_l2, t_l2, ang, sel, m_q, o_q, m_t, o_t.
    Needs M <= 112 virtual points (raises DfepeError 'unsupported' otherwise: use floss + pose_errors)."""
    F_layers, T1c, T2c, st, K, virt1, virt2 = _floss_args(F_layers, T1, T2, K, virt1, virt2)
    if q_gt is not None:
        _, q_gt, t_gt, R_gt = _pose_args(F_layers, q_gt, t_gt, R_gt)
    if extra is not None:
        extra = _prep(extra, "extra")
        _shape(extra, "extra rows", None, F_layers.shape[1])
    r = _TailJacFunction.apply(F_layers, T1c, T2c, st, K, virt1, virt2, float(clamp_at), q_gt, t_gt, R_gt, bool(floss_grad), extra,
                               float(extra_scale))
    keys = ("loss_sum", "E_layers", "m_loss", "o_loss", "row_min", "col_min", "m_extra", "o_extra", "qt", "q_l2", "t_l2", "ang", "sel",
            "m_q", "o_q", "m_t", "o_t")
    return dict(zip(keys, r))
