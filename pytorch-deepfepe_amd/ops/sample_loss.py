"""The sample-loss branch (csrc/sample_loss.hip): multisets drawn in proportion to the weights, the top-K pick, the fits of the drawn
sets with their adjoint back to the weights, and the epipolar loss of every set's F on the virtual points."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from ._base import Tensor, _n_valid_arg, _on, _on_gpu, _prep, _ptr, _shape, _stream, _workspace
from .fit import w8pt_backward, w8pt_forward
from .loss import _t_arg
from .sampler import _MASK64, _counter_arg


def sample_multisets(weights: Optional[Tensor], H: int = 100, K: int = 20, *, seed: int, offset: int = 0, counter: Optional[Tensor] = None,
                     n_valid: Optional[Tensor] = None, B: Optional[int] = None, N: Optional[int] = None, device=None,
                     want_fallback: bool = False):
    """idx [B,H,K] int32 drawn on the current stream WITH replacement in proportion to ``weights`` [B,N] on the GPU
    (dfepe_sample_multisets, include/dfepe.h): the law of the reference's np.random.choice(n, topK, p=p), H times per pair, under the
    Philox streams of ops.sample_sets (``seed``, ``offset``, the device ``counter``).  NaN, +-inf, <= 0 and weights below 2^-30 of the
    pair's largest are never drawn; a pair without a drawable weight is drawn uniformly and flagged.  ``n_valid`` [B] int32 on the GPU:
    only the first clamp(n_valid[b], K, N) correspondences.  ``weights`` None (then B, N and the device are given): uniform with
    replacement.  Returns idx, or (idx, fallback [B] int32) with ``want_fallback``.  No host synchronisation; capturable."""
    H, K = int(H), int(K)
    if weights is not None:
        weights = _prep(weights.detach(), "sample_multisets: weights")
        if weights.dim() != 2:
            raise ValueError(f"sample_multisets: weights must be [B,N], got {tuple(weights.shape)}")
        B, N = weights.shape
        dev = weights.device
    else:
        if B is None or N is None:
            raise ValueError("sample_multisets: without weights B and N must be given")
        if int(B) < 0 or H < 1 or not _lib.SAMPLE_MIN_DRAWS <= K <= _lib.SAMPLE_MAX_DRAWS or int(N) < K:  # before any device is asked for
            raise ValueError(f"sample_multisets: needs B >= 0, H >= 1 and {_lib.SAMPLE_MIN_DRAWS} <= K <= {_lib.SAMPLE_MAX_DRAWS} <= N, "
                             f"got B={B}, H={H}, K={K}, N={N}")
        given = [t for t in (n_valid, counter) if torch.is_tensor(t) and t.is_cuda]
        dev = given[0].device if given else torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if dev.type != "cuda":
            raise _lib.DfepeError("sample_multisets: the device must be a GPU (this package has no CPU path)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
    B, N = int(B), int(N)
    if B < 0 or H < 1 or not _lib.SAMPLE_MIN_DRAWS <= K <= _lib.SAMPLE_MAX_DRAWS or N < K:
        raise ValueError(f"sample_multisets: needs B >= 0, H >= 1 and {_lib.SAMPLE_MIN_DRAWS} <= K <= {_lib.SAMPLE_MAX_DRAWS} <= N, "
                         f"got B={B}, H={H}, K={K}, N={N}")
    if weights is not None and N > _lib.SAMPLER_MAX_WEIGHTED_N:
        raise ValueError(f"sample_multisets: takes N <= {_lib.SAMPLER_MAX_WEIGHTED_N}, got {N}")
    if counter is not None:
        counter = _counter_arg(counter, "sample_multisets")
    n_valid = _n_valid_arg(n_valid, B, dev, "sample_multisets")
    L = _lib.lib()
    idx = torch.empty(B, H, K, device=dev, dtype=torch.int32)
    fallback = torch.zeros(B, device=dev, dtype=torch.int32) if want_fallback else None
    if B > 0:
        ws = _workspace(L.dfepe_sample_sets_workspace_bytes(B, N, 1), dev) if weights is not None else None
        with _on(dev):
            rc = L.dfepe_sample_multisets(_stream(), B, N, H, K, int(seed) & _MASK64, int(offset) & 0xFFFFFFFF, _ptr(counter), _ptr(weights),
                                          _ptr(n_valid), _ptr(idx), _ptr(fallback), _ptr(ws))
        _lib.check(rc, "dfepe_sample_multisets")
    return (idx, fallback) if want_fallback else idx


def topk_select(x: Tensor, K: int, n_valid: Optional[Tensor] = None, want_values: bool = False):
    """idx [B,K] int32: the K largest of x[b, :clamp(n_valid[b], K, N)] in descending order (dfepe_topk_select): values compare as
    floats, equal values (+-0 included) go lowest index first, NaN is greatest (as torch.topk orders it), lowest index first among
    NaNs.  Not differentiable: gather x with idx for the values' gradient.  Returns idx, or (idx, values) with ``want_values``."""
    x = _prep(x.detach(), "topk_select: x")
    if x.dim() != 2:
        raise ValueError(f"topk_select: x must be [B,N], got {tuple(x.shape)}")
    B, N = x.shape
    K = int(K)
    if not 1 <= K <= N:
        raise ValueError(f"topk_select: needs 1 <= K <= N, got K={K}, N={N}")
    n_valid = _n_valid_arg(n_valid, B, x.device, "topk_select")
    idx = torch.empty(B, K, device=x.device, dtype=torch.int32)
    values = torch.empty(B, K, device=x.device, dtype=torch.float32) if want_values else None
    if B > 0:
        with _on(x.device):
            rc = _lib.lib().dfepe_topk_select(_stream(), _ptr(x), _ptr(n_valid), B, N, K, _ptr(idx), _ptr(values))
        _lib.check(rc, "dfepe_topk_select")
    return (idx, values) if want_values else idx


def _idx_arg(idx, B: int, name: str) -> Tensor:
    _on_gpu(idx, f"{name}: idx")
    if idx.dim() != 3 or idx.shape[0] != B or idx.dtype != torch.int32:
        raise ValueError(f"{name}: idx must be int32 [{B},H,K], got {idx.dtype} {tuple(idx.shape)}")
    return idx.contiguous()


def sample_gather(pts1: Tensor, pts2: Tensor, weights: Tensor, idx: Tensor, want_accu: bool = True):
    """Raw launch of dfepe_sample_gather: (pts1_sel, pts2_sel [B H,K,3], w_sel [B H,K], accu [B,H] | None)."""
    B, N = weights.shape
    H, K = idx.shape[1], idx.shape[2]
    dev = weights.device
    p1 = torch.empty(B * H, K, 3, device=dev, dtype=torch.float32)
    p2 = torch.empty(B * H, K, 3, device=dev, dtype=torch.float32)
    ws = torch.empty(B * H, K, device=dev, dtype=torch.float32)
    accu = torch.empty(B, H, device=dev, dtype=torch.float32) if want_accu else None
    if B > 0:
        with _on(dev):
            rc = _lib.lib().dfepe_sample_gather(_stream(), _ptr(pts1), _ptr(pts2), _ptr(weights), _ptr(idx), B, N, H, K, _ptr(p1), _ptr(p2),
                                                _ptr(ws), _ptr(accu))
        _lib.check(rc, "dfepe_sample_gather")
    return p1, p2, ws, accu


def sample_scatter_bwd(g_w_sel: Optional[Tensor], g_accu: Optional[Tensor], weights: Tensor, accu: Optional[Tensor], idx: Tensor) -> Tensor:
    """Raw launch of dfepe_sample_scatter_bwd: g_w [B,N] from g_w_sel [B,H,K] (or None) and g_accu [B,H] (or None)."""
    B, N = weights.shape
    H, K = idx.shape[1], idx.shape[2]
    g_w = torch.empty(B, N, device=weights.device, dtype=torch.float32)
    if B > 0:
        with _on(weights.device):
            rc = _lib.lib().dfepe_sample_scatter_bwd(_stream(), _ptr(g_w_sel), _ptr(g_accu), _ptr(weights), _ptr(accu), _ptr(idx), B, N, H, K,
                                                     _ptr(g_w))
        _lib.check(rc, "dfepe_sample_scatter_bwd")
    return g_w


class _SampleFitsFunction(torch.autograd.Function):
    """Gather, the existing fit forward with its `save` record; backward: the existing fit adjoint, then the scatter."""

    @staticmethod
    def forward(ctx, pts1, pts2, weights, idx, extra_flags):
        ctx.set_materialize_grads(False)
        B, H = idx.shape[0], idx.shape[1]
        p1, p2, ws, accu = sample_gather(pts1, pts2, weights, idx)
        F, _, _, save, _ = w8pt_forward(p1, p2, ws, False, 0.0, 0.0, 0.5, False, True, extra_flags=extra_flags)
        ctx.save_for_backward(p1, p2, ws, save, F, weights, accu, idx)
        ctx.extra_flags = extra_flags
        return F.view(B, H, 3, 3), accu.view(B, H, 1)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gF, gAccu):
        p1, p2, ws, save, F, weights, accu, idx = ctx.saved_tensors
        if gF is None and gAccu is None:
            return None, None, None, None, None
        g_w_sel = None
        if gF is not None:
            g_w_sel = w8pt_backward(p1, p2, ws, False, 0.0, 0.0, 0.5, save, F, gF.reshape(-1, 3, 3).contiguous().float(), None, None,
                                    extra_flags=ctx.extra_flags)
        g_accu = None if gAccu is None else gAccu.reshape(accu.shape).contiguous().float()
        return None, None, sample_scatter_bwd(g_w_sel, g_accu, weights, accu, idx), None, None


def sample_fits(pts1: Tensor, pts2: Tensor, weights: Tensor, idx: Tensor, normalize_rows: bool = True):
    """The fits of the drawn sets: pts1, pts2 [B,N,3], weights [B,N] or [B,1,N], idx [B,H,K] int32 (ops.sample_multisets) ->
    (F_sel [B,H,3,3], accu [B,H,1]): out_sample_selected_batch and weights_sample_selected_accu_batch of the reference's Fit.forward
    (DeepFNetSampleLoss.py:399-429).  One gather launch, one launch of the existing fit on B H problems of K; the backward is the
    existing fit adjoint and one scatter launch.  Differentiable w.r.t. ``weights`` only: the points are constants, and a point
    tensor that requires grad raises.  accu is prod(1000 w) / (sum + 1e-10) in fp64 (dfepe_sample_gather)."""
    pts1, pts2 = _prep(pts1, "sample_fits: pts1"), _prep(pts2, "sample_fits: pts2")
    if torch.is_grad_enabled() and (pts1.requires_grad or pts2.requires_grad):
        raise _lib.DfepeError("sample_fits: gradients w.r.t. the points are not built (the points are constants of the sample loss)")
    w = _prep(weights.reshape(weights.shape[0], -1), "sample_fits: weights")
    B, N = w.shape
    _shape(pts1, "pts1 (homogeneous points)", B, N, 3)
    _shape(pts2, "pts2 (homogeneous points)", B, N, 3)
    idx = _idx_arg(idx, B, "sample_fits")
    return _SampleFitsFunction.apply(pts1, pts2, w, idx, 0 if normalize_rows else _lib.W8PT_NO_ROWNORM)


class _SampleFlossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, F_sel, T1c, T2c, st, virt1, virt2, clamp_at):
        B, H = F_sel.shape[0], F_sel.shape[1]
        M = virt1.shape[1]
        loss_sum = torch.empty(B, H, device=F_sel.device, dtype=torch.float32)
        if B > 0:
            with _on(F_sel.device):
                rc = _lib.lib().dfepe_sample_floss_fwd(_stream(), _ptr(F_sel), B, H, _ptr(T1c), _ptr(T2c), st, _ptr(virt1), _ptr(virt2), M,
                                                       float(clamp_at), _ptr(loss_sum))
            _lib.check(rc, "dfepe_sample_floss_fwd")
        ctx.save_for_backward(F_sel, T1c, T2c, virt1, virt2)
        ctx.cfg = (st, float(clamp_at))
        return loss_sum

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        F_sel, T1c, T2c, virt1, virt2 = ctx.saved_tensors
        st, clamp_at = ctx.cfg
        B, H = F_sel.shape[0], F_sel.shape[1]
        gF = torch.empty_like(F_sel)
        g = g.contiguous().float()
        if B > 0:
            with _on(F_sel.device):
                rc = _lib.lib().dfepe_sample_floss_bwd(_stream(), _ptr(F_sel), B, H, _ptr(T1c), _ptr(T2c), st, _ptr(virt1), _ptr(virt2),
                                                       virt1.shape[1], clamp_at, _ptr(g), _ptr(gF))
            _lib.check(rc, "dfepe_sample_floss_bwd")
        return gF, None, None, None, None, None, None


def sample_floss(F_sel: Tensor, T1: Tensor, T2: Tensor, virt1: Tensor, virt2: Tensor, clamp_at: float = 0.02) -> Tensor:
    """F_sel [B,H,3,3] -> loss_sum [B,H]: the sum over the M virtual points of compute_epi_residual(T1 virt1, T2 virt2, F_sel[b,h],
    clamp_at) (train_good_utils.py:402-407), one launch for all pairs and sets.  T1, T2 [3,3], [1,3,3] or [B,3,3]; virt1, virt2
    [B,M,3].  Differentiable in F_sel."""
    F_sel, virt1, virt2 = _prep(F_sel, "sample_floss: F_sel"), _prep(virt1, "sample_floss: virt1"), _prep(virt2, "sample_floss: virt2")
    _shape(F_sel, "F_sel", None, None, 3, 3)
    B = F_sel.shape[0]
    _shape(virt1, "virt1 (homogeneous pixel points)", B, None, 3)
    _shape(virt2, "virt2", B, virt1.shape[1], 3)
    if virt1.shape[1] > _lib.lib().dfepe_sample_loss_max_virt():
        raise ValueError(f"sample_floss: takes M <= {_lib.lib().dfepe_sample_loss_max_virt()} virtual points, got {virt1.shape[1]}")
    for T in (T1, T2):
        if not ((T.dim() == 2 and tuple(T.shape) == (3, 3)) or (T.dim() == 3 and T.shape[0] in (1, B) and tuple(T.shape[1:]) == (3, 3))):
            raise ValueError(f"T1/T2 must be [3,3], [1,3,3] or [{B},3,3], got {tuple(T.shape)}")
    T1c, st1 = _t_arg(T1.detach(), B)
    T2c, st2 = _t_arg(T2.detach(), B)
    if st1 != st2:
        T1c, T2c, st1 = T1c.expand(B, 3, 3).contiguous(), T2c.expand(B, 3, 3).contiguous(), 9
    return _SampleFlossFunction.apply(F_sel, T1c, T2c, st1, virt1, virt2, clamp_at)
