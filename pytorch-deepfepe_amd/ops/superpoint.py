"""SuperPoint output processing (csrc/sp_process.hip)."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from ._base import Tensor, _on, _on_gpu, _prep, _ptr, _shape, _stream, _workspace


# ------------------------------------------------------------------------------------------------
# SuperPoint output processing (process_SP_output, train_good_utils.py:727-755): heatmap, NMS, soft-argmax, descriptors
# ------------------------------------------------------------------------------------------------
def _sp_pixels(H: int, W: int, what: str) -> None:
    if H * W > _lib.SP_MAX_PIXELS:
        raise _lib.DfepeError(f"{what}: {H}x{W} pixels per image; at most {_lib.SP_MAX_PIXELS}")


class _SpFlattenFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, semi):
        B, _, Hc, Wc = semi.shape
        heat = torch.empty(B, 1, 8 * Hc, 8 * Wc, device=semi.device, dtype=torch.float32)
        with _on(semi.device):
            rc = _lib.lib().dfepe_sp_flatten(_ptr(semi), B, 8 * Hc, 8 * Wc, _ptr(heat), _stream())
        _lib.check(rc, "dfepe_sp_flatten")
        ctx.save_for_backward(semi)
        return heat

    @staticmethod
    def backward(ctx, g):
        (semi,) = ctx.saved_tensors
        B, _, Hc, Wc = semi.shape
        g = g.contiguous().float()
        g_semi = torch.empty_like(semi)
        with _on(semi.device):
            rc = _lib.lib().dfepe_sp_flatten_bwd(_ptr(semi), _ptr(g), B, 8 * Hc, 8 * Wc, _ptr(g_semi), _stream())
        _lib.check(rc, "dfepe_sp_flatten_bwd")
        return g_semi


def sp_flatten(semi: Tensor) -> Tensor:
    """semi [B,65,Hc,Wc] -> heatmap [B,1,8Hc,8Wc]: the softmax over the 65 channels without the dustbin, channel c of a cell at
    pixel (c//8, c%8) of its 8x8 block; a NaN logit is read as 0 and receives no gradient (flattenDetection after set_nan2zero,
    train_good_utils.py:741-743).  Differentiable w.r.t. semi."""
    semi = _prep(semi, "semi")
    _shape(semi, "semi", None, 65, None, None)
    if semi.shape[2] < 1 or semi.shape[3] < 1:
        raise ValueError(f"semi must have at least one cell, got {tuple(semi.shape)}")
    _sp_pixels(8 * semi.shape[2], 8 * semi.shape[3], "sp_flatten")
    return _SpFlattenFunction.apply(semi)


def sp_nms_capacity(H: int, W: int, nms_dist: int) -> int:
    """Rows of the point list of sp_nms: ceil(H/(d+1)) ceil(W/(d+1)), which no greedy NMS result exceeds."""
    return int(_lib.lib().dfepe_sp_nms_capacity(int(H), int(W), int(nms_dist)))


def sp_nms(heatmap: Tensor, conf_thresh: float, nms_dist: int, border_remove: Optional[int] = None) -> dict:
    """heatmap [B,1,H,W] -> the greedy nms_fast of every image (heatmap_to_nms, train_good_utils.py:745): candidates h >=
    conf_thresh visited by (confidence descending, row-major index ascending), kept iff no kept candidate lies within Chebyshev
    distance nms_dist, border points (border_remove, default nms_dist) removed afterwards.  Returns dict(nms_map [B,1,H,W] of 0/1,
    pts [B,cap,2] int32 (x, y) in row-major order, conf [B,cap], count [B] int32) with cap = sp_nms_capacity(H, W, nms_dist); rows
    from count[b] on are 0.  Exact for any input; no host synchronisation; nothing differentiable."""
    h = _prep(heatmap.detach(), "heatmap")
    _shape(h, "heatmap", None, 1, None, None)
    B, _, H, W = h.shape
    d = int(nms_dist)
    r = d if border_remove is None else int(border_remove)
    if d < 0 or r < 0 or H < 1 or W < 1:
        raise ValueError("sp_nms: nms_dist and border_remove must be >= 0 and the heatmap not empty")
    _sp_pixels(H, W, "sp_nms")
    L = _lib.lib()
    dev = h.device
    cap = int(L.dfepe_sp_nms_capacity(H, W, d))
    out = {
        "nms_map": torch.empty(B, 1, H, W, device=dev, dtype=torch.float32),
        "pts": torch.empty(B, cap, 2, device=dev, dtype=torch.int32),
        "conf": torch.empty(B, cap, device=dev, dtype=torch.float32),
        "count": torch.empty(B, device=dev, dtype=torch.int32),
    }
    ws = _workspace(L.dfepe_sp_nms_workspace_bytes(B, H, W), dev)
    with _on(dev):
        rc = L.dfepe_sp_nms(_ptr(h), B, H, W, float(conf_thresh), d, r, _ptr(ws), _ptr(out["nms_map"]), _ptr(out["pts"]), _ptr(out["conf"]),
                            _ptr(out["count"]), _stream())
    _lib.check(rc, "dfepe_sp_nms")
    return out


def _sp_list(pts: Tensor, count: Tensor, B: int, what: str):
    for t in (pts, count):
        _on_gpu(t, what + ": pts and count")
    if pts.dim() != 3 or pts.shape[0] != B or pts.shape[2] != 2 or pts.dtype != torch.int32 or count.shape != (B,) or count.dtype != torch.int32:
        raise ValueError(f"{what}: pts must be int32 [B,cap,2] and count int32 [B], the outputs of sp_nms")
    return pts.contiguous(), count.contiguous()


class _SpSoftArgmaxFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, heat, pts, count, p, r, want_patches):
        B, _, H, W = heat.shape
        cap = pts.shape[1]
        dev = heat.device
        pred = torch.empty(B, cap, 2, device=dev, dtype=torch.float32)
        patches = torch.empty(B, cap, p, p, device=dev, dtype=torch.float32) if want_patches else None
        with _on(dev):
            rc = _lib.lib().dfepe_sp_soft_argmax(_ptr(heat), _ptr(pts), _ptr(count), B, H, W, cap, p, r, _ptr(pred), _ptr(patches), _stream())
        _lib.check(rc, "dfepe_sp_soft_argmax")
        ctx.save_for_backward(heat, pts, count)
        ctx.p, ctx.r = p, r
        if patches is None:
            return pred
        ctx.mark_non_differentiable(patches)
        return pred, patches

    @staticmethod
    def backward(ctx, g_pred, *_):
        heat, pts, count = ctx.saved_tensors
        B, _, H, W = heat.shape
        cap = pts.shape[1]
        dev = heat.device
        g_pred = g_pred.contiguous().float()
        L = _lib.lib()
        ws = _workspace(L.dfepe_sp_soft_argmax_bwd_workspace_bytes(B, H, W, cap), dev)
        g_heat = torch.empty_like(heat)
        with _on(dev):
            rc = L.dfepe_sp_soft_argmax_bwd(_ptr(heat), _ptr(pts), _ptr(count), _ptr(g_pred), B, H, W, cap, ctx.p, ctx.r, _ptr(ws), _ptr(g_heat),
                                            _stream())
        _lib.check(rc, "dfepe_sp_soft_argmax_bwd")
        return g_heat, None, None, None, None, None


def sp_soft_argmax(heatmap: Tensor, pts: Tensor, count: Tensor, patch_size: int, border_remove: int, want_patches: bool = False):
    """heatmap [B,1,H,W], pts [B,cap,2] int32 (x, y) and count [B] int32 from sp_nms -> pred [B,cap,2]: the sub-pixel offset (x, y) of
    every listed point from the patch_size x patch_size patch around it (pred_soft_argmax, train_good_utils.py:747), 0 for rows
    not listed and for a patch whose sum is not positive; with want_patches also the normalised patches [B,cap,p,p] (no gradient).
    patch_size must be odd and <= 2 border_remove + 1, the border that sp_nms removed, so that every patch lies inside the image.
    Differentiable w.r.t. the heatmap; the adjoint is a gather, bit-identical from run to run."""
    h = _prep(heatmap, "heatmap")
    _shape(h, "heatmap", None, 1, None, None)
    B, _, H, W = h.shape
    pts, count = _sp_list(pts, count, B, "sp_soft_argmax")
    p, r = int(patch_size), int(border_remove)
    if p < 1 or p % 2 == 0 or r < 0 or p > 2 * r + 1:
        raise ValueError(f"sp_soft_argmax: patch_size must be odd and in [1, 2 border_remove + 1], got {p} with border_remove {r}")
    if p > _lib.SP_MAX_PATCH:
        raise _lib.DfepeError(f"sp_soft_argmax: patch_size {p}; at most {_lib.SP_MAX_PATCH}")
    _sp_pixels(H, W, "sp_soft_argmax")
    return _SpSoftArgmaxFunction.apply(h, pts, count, p, r, bool(want_patches))


def sp_sample_desc(desc: Tensor, pts: Tensor, pred: Optional[Tensor], count: Tensor, align_corners: bool = True) -> Tensor:
    """desc [B,D,Hc,Wc] coarse descriptors, positions pts + pred in pixels of the [8Hc,8Wc] image -> [B,cap,D]: the bilinear sample
    (zero padding) at every listed position divided by its L2 norm, zeros for a zero norm and for rows not listed
    (sample_desc_from_points).  align_corners=True is grid_sample's rule in the torch version that the reference pins.  Forward
    only: the reference hands these descriptors to the matcher detached (train_good_utils.py:664, 686-688)."""
    d = _prep(desc.detach(), "desc")
    if d.dim() != 4 or min(d.shape[1:]) < 1:
        raise ValueError(f"desc must be [B,D,Hc,Wc], got {tuple(d.shape)}")
    B, D, Hc, Wc = d.shape
    pts, count = _sp_list(pts, count, B, "sp_sample_desc")
    cap = pts.shape[1]
    pr = None
    if pred is not None:
        pr = _prep(pred.detach(), "pred")
        _shape(pr, "pred", B, cap, 2)
    _sp_pixels(8 * Hc, 8 * Wc, "sp_sample_desc")
    out = torch.empty(B, cap, D, device=d.device, dtype=torch.float32)
    with _on(d.device):
        rc = _lib.lib().dfepe_sp_sample_desc(_ptr(d), _ptr(pts), _ptr(pr), _ptr(count), B, D, 8 * Hc, 8 * Wc, cap, int(bool(align_corners)),
                                             _ptr(out), _stream())
    _lib.check(rc, "dfepe_sp_sample_desc")
    return out
