"""Epipolar residuals, distances and their sums, with the adjoints (csrc/geom.hip, epi_adjoint.hip)."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from ._base import Tensor, _on, _prep, _ptr, _shape, _stream


# ------------------------------------------------------------------------------------------------
# stand-alone geometry entry points
# ------------------------------------------------------------------------------------------------
class _EpiResidualFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pts1, pts2, F, clamp_at):
        B, N = pts1.shape[0], pts1.shape[1]
        out = torch.empty(B, N, device=pts1.device, dtype=torch.float32)
        with _on(pts1.device):
            rc = _lib.lib().dfepe_epi_residual_fwd(_ptr(pts1), _ptr(pts2), _ptr(F), B, N, float(clamp_at), _ptr(out), _stream())
        _lib.check(rc, "dfepe_epi_residual_fwd")
        ctx.save_for_backward(pts1, pts2, F)
        ctx.clamp_at = float(clamp_at)
        return out

    @staticmethod
    def backward(ctx, g):
        pts1, pts2, F = ctx.saved_tensors
        B, N = pts1.shape[0], pts1.shape[1]
        g = g.contiguous().float()
        gF = g1 = g2 = None
        if ctx.needs_input_grad[2]:
            gF = torch.empty_like(F)
            with _on(pts1.device):
                rc = _lib.lib().dfepe_epi_residual_bwd(_ptr(pts1), _ptr(pts2), _ptr(F), B, N, ctx.clamp_at, _ptr(g), _ptr(gF), _stream())
            _lib.check(rc, "dfepe_epi_residual_bwd")
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            g1 = torch.empty_like(pts1) if ctx.needs_input_grad[0] else None
            g2 = torch.empty_like(pts2) if ctx.needs_input_grad[1] else None
            with _on(pts1.device):
                rc = _lib.lib().dfepe_epi_residual_bwd_pts(_stream(), _ptr(pts1), _ptr(pts2), _ptr(F), B, N, ctx.clamp_at, _ptr(g), _ptr(g1),
                                                           _ptr(g2))
            _lib.check(rc, "dfepe_epi_residual_bwd_pts")
        return g1, g2, gF, None


def epi_residual(pts1: Tensor, pts2: Tensor, F: Tensor, clamp_at: float = 0.5) -> Tensor:
    """pts [B,N,3], F [B,3,3] -> [B,N]; differentiable w.r.t. F (dfepe_epi_residual_bwd) and the points
    (dfepe_epi_residual_bwd_pts); only what is asked for is computed."""
    pts1, pts2, F = _prep(pts1, "pts1"), _prep(pts2, "pts2"), _prep(F, "F")
    _shape(pts1, "pts1 (homogeneous points)", None, None, 3)
    _shape(pts2, "pts2", pts1.shape[0], pts1.shape[1], 3)
    _shape(F, "F", pts1.shape[0], 3, 3)
    return _EpiResidualFunction.apply(pts1, pts2, F, clamp_at)


def _epi_metrics_launch(kind: int, F: Tensor, X: Tensor, Y: Tensor, clamp_at: float, eps: float) -> Tensor:
    B, N = X.shape[0], X.shape[1]
    out = torch.empty((3, B, N) if (kind & 7) == 2 else (B, N), device=X.device, dtype=torch.float32)
    with _on(X.device):
        rc = _lib.lib().dfepe_epi_metrics(int(kind), _ptr(F), _ptr(X), _ptr(Y), B, N, float(clamp_at), float(eps), _ptr(out), _stream())
    _lib.check(rc, "dfepe_epi_metrics")
    return out


def _epi_adjoint_workspace(B: int, N: int, dev) -> Optional[Tensor]:
    """Per-call scratch of the chunked g_F / loss sums (dfepe_epi_adjoint_workspace_bytes): None while a pair is one chunk."""
    n = int(_lib.lib().dfepe_epi_adjoint_workspace_bytes(B, N))
    return torch.empty(n // 8, dtype=torch.float64, device=dev) if n else None


class _EpiMetricsFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, F, X, Y, kind, clamp_at, eps):
        ctx.save_for_backward(F, X, Y)
        ctx.cfg = (kind, clamp_at, eps)
        return _epi_metrics_launch(kind, F, X, Y, clamp_at, eps)

    @staticmethod
    def backward(ctx, g):
        F, X, Y = ctx.saved_tensors
        kind, clamp_at, eps = ctx.cfg
        B, N = X.shape[0], X.shape[1]
        g = g.contiguous().float()
        gF = torch.empty_like(F) if ctx.needs_input_grad[0] else None
        gX = torch.empty_like(X) if ctx.needs_input_grad[1] else None
        gY = torch.empty_like(Y) if ctx.needs_input_grad[2] else None
        ws = _epi_adjoint_workspace(B, N, X.device) if gF is not None else None
        with _on(X.device):
            rc = _lib.lib().dfepe_epi_metrics_bwd(_stream(), kind, _ptr(F), _ptr(X), _ptr(Y), B, N, clamp_at, eps, _ptr(g), _ptr(gF),
                                                  _ptr(gX), _ptr(gY), _ptr(ws))
        _lib.check(rc, "dfepe_epi_metrics_bwd")
        return gF, gX, gY, None, None, None


def _epi_args(what: str, kind: int, F: Tensor, X: Tensor, Y: Tensor, clamp_at: Optional[float]):
    F, X, Y = _prep(F, "F"), _prep(X, "X"), _prep(Y, "Y")
    if X.dim() != 3 or X.shape != Y.shape or X.shape[2] not in (2, 3) or F.shape != (X.shape[0], 3, 3):
        raise ValueError(f"{what}: F [B,3,3], X and Y [B,N,2|3] expected, got {tuple(F.shape)}, {tuple(X.shape)}, {tuple(Y.shape)}")
    kind = int(kind) | (_lib.EPI_HOMOGENEOUS if X.shape[2] == 3 else 0)
    return F, X, Y, kind, (-1.0 if clamp_at is None else float(clamp_at))


def epi_metrics(kind: int, F: Tensor, X: Tensor, Y: Tensor, clamp_at: Optional[float] = None, eps: float = 0.0) -> Tensor:
    """kind 0 sym-epi (squared), 1 Sampson, 2 epi-distance (3 planes).  F [B,3,3]; X, Y [B,N,2], or [B,N,3] homogeneous points
    that are used as they are; clamp_at None = no clamp.  Differentiable w.r.t. F, X and Y (dfepe_epi_metrics_bwd: one more launch
    in the backward, two when a pair spans several chunks); with nothing requiring grad it is the forward launch alone."""
    F, X, Y, kind, clamp_at = _epi_args("epi_metrics", kind, F, X, Y, clamp_at)
    if torch.is_grad_enabled() and (F.requires_grad or X.requires_grad or Y.requires_grad):
        return _EpiMetricsFunction.apply(F, X, Y, kind, clamp_at, float(eps))
    return _epi_metrics_launch(kind, F, X, Y, clamp_at, eps)


class _EpiLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, F, X, Y, w, kind, clamp_at, eps):
        B, N = X.shape[0], X.shape[1]
        out = torch.zeros(B, device=X.device, dtype=torch.float32) if N == 0 else torch.empty(B, device=X.device, dtype=torch.float32)
        ws = _epi_adjoint_workspace(B, N, X.device)
        with _on(X.device):
            rc = _lib.lib().dfepe_epi_loss_fwd(_stream(), kind, _ptr(F), _ptr(X), _ptr(Y), _ptr(w), B, N, clamp_at, eps, _ptr(out), _ptr(ws))
        _lib.check(rc, "dfepe_epi_loss_fwd")
        ctx.save_for_backward(F, X, Y, w)
        ctx.cfg = (kind, clamp_at, eps)
        return out

    @staticmethod
    def backward(ctx, g):
        F, X, Y, w = ctx.saved_tensors
        kind, clamp_at, eps = ctx.cfg
        B, N = X.shape[0], X.shape[1]
        g = g.contiguous().float()
        need = ctx.needs_input_grad
        gF = (torch.zeros_like(F) if N == 0 else torch.empty_like(F)) if need[0] else None
        gX = torch.empty_like(X) if need[1] else None
        gY = torch.empty_like(Y) if need[2] else None
        gw = torch.empty_like(w) if (w is not None and need[3]) else None
        ws = _epi_adjoint_workspace(B, N, X.device) if gF is not None else None
        with _on(X.device):
            rc = _lib.lib().dfepe_epi_loss_bwd(_stream(), kind, _ptr(F), _ptr(X), _ptr(Y), _ptr(w), B, N, clamp_at, eps, _ptr(g), _ptr(gF),
                                               _ptr(gX), _ptr(gY), _ptr(gw), _ptr(ws))
        _lib.check(rc, "dfepe_epi_loss_bwd")
        return gF, gX, gY, gw, None, None, None


def epi_loss(kind: int, F: Tensor, X: Tensor, Y: Tensor, weights: Optional[Tensor] = None, clamp_at: Optional[float] = None,
             eps: float = 0.0, reduction: str = "sum") -> Tensor:
    """sum_n weights[b,n] e[b,n] of an epipolar distance without writing the per-point values: e is kind 0 (sym-epi, squared,
    clamped at clamp_at), kind 1 (Sampson) or the first plane of kind 2 ((d1 + d2) / 2).  One launch forward and one backward (two
    each when a pair spans several chunks); differentiable w.r.t. F, X, Y and weights.  reduction: "none" the per-pair sums [B],
    "sum" their sum, "mean" that divided by B * N, as losses.mean() gives (get_loss_softmax, HLoss)."""
    if reduction not in ("sum", "mean", "none"):
        raise ValueError(f"epi_loss: reduction must be 'sum', 'mean' or 'none', got {reduction!r}")
    F, X, Y, kind, clamp_at = _epi_args("epi_loss", kind, F, X, Y, clamp_at)
    B, N = X.shape[0], X.shape[1]
    if weights is not None:
        weights = _prep(weights, "weights")
        _shape(weights, "weights", B, N)
    sums = _EpiLossFunction.apply(F, X, Y, weights, kind, clamp_at, float(eps))
    if reduction == "none":
        return sums
    return sums.sum() if reduction == "sum" else sums.sum() / (B * N)
