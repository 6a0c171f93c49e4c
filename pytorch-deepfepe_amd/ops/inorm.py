"""The weight estimator's fused normalisation layer (csrc/inorm.hip)."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from ._base import Tensor, _on, _prep, _ptr, _stream


# ------------------------------------------------------------------------------------------------
# InstanceNorm1d(affine) + LeakyReLU on channel-major activations (weight-estimator fusion, "next" row f-1)
# ------------------------------------------------------------------------------------------------
class _InormLReLUFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Y, gamma, beta, eps, slope, skipped_bias):
        C, R, N = Y.shape
        A = torch.empty_like(Y)
        stats = torch.empty(C * R, 2, device=Y.device, dtype=torch.float32)
        with _on(Y.device):
            rc = _lib.lib().dfepe_inorm_lrelu_fwd(_ptr(Y), _ptr(gamma), _ptr(beta), C, R, N, float(eps), float(slope), _ptr(A),
                                                  _ptr(stats), _stream())
        _lib.check(rc, "dfepe_inorm_lrelu_fwd")
        ctx.save_for_backward(Y, gamma, beta, stats)
        ctx.slope = float(slope)
        ctx.bias_like = skipped_bias
        return A

    @staticmethod
    def backward(ctx, gA):
        Y, gamma, beta, stats = ctx.saved_tensors
        C, R, N = Y.shape
        gA = gA.contiguous()
        gY = torch.empty_like(Y)
        rg = torch.empty(C, R, device=Y.device, dtype=torch.float32)
        rb = torch.empty(C, R, device=Y.device, dtype=torch.float32)
        with _on(Y.device):
            rc = _lib.lib().dfepe_inorm_lrelu_bwd(_ptr(Y), _ptr(gA), _ptr(gamma), _ptr(beta), _ptr(stats), C, R, N, ctx.slope,
                                                  _ptr(gY), _ptr(rg), _ptr(rb), _stream())
        _lib.check(rc, "dfepe_inorm_lrelu_bwd")
        # the bias of the convolution that feeds this normalisation cancels in it: its gradient is exactly zero, and it is
        # returned as such so that the parameter stays in the graph (DistributedDataParallel, optimizer state, weight decay)
        gb = None if ctx.bias_like is None else torch.zeros_like(ctx.bias_like)
        return gY, rg.sum(dim=1), rb.sum(dim=1), None, None, gb


def inorm_lrelu(Y: Tensor, gamma: Tensor, beta: Tensor, eps: float = 1e-5, slope: float = 0.01,
                skipped_bias: Optional[Tensor] = None) -> Tensor:
    """Y [C,R,N] channel-major (contiguous) -> LeakyReLU(InstanceNorm over N with affine gamma/beta [C]).
    ``skipped_bias``: the [C] bias of the convolution that produced Y without it (a per-channel constant cancels in the
    instance normalisation); it receives an exact zero gradient instead of none."""
    return _InormLReLUFunction.apply(_prep(Y, "Y"), _prep(gamma, "gamma"), _prep(beta, "beta"), eps, slope, skipped_bias)
