"""Descriptor matching and the gather of the chosen matches (csrc/match.hip, knn_match.hip)."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from ._base import Tensor, _on, _prep, _ptr, _shape, _stream


# ------------------------------------------------------------------------------------------------
# match construction ("next" row f-3): two-way nearest-neighbour matching of descriptors + crop/pad gather
# ------------------------------------------------------------------------------------------------
def nn_match_two_way(desc1: Tensor, desc2: Tensor, nn_thresh: float):
    """desc1 [B,N1,D], desc2 [B,N2,D] unit-norm descriptors -> (m_idx1 [B,N1] int32, m_idx2 [B,N1] int32, score [B,N1],
    count [B] int32): the first count[b] entries of row b are pair b's mutual nearest neighbours closer than ``nn_thresh``
    in increasing m_idx1 order (PointTracker.nn_match_two_way as called at train_good_utils.py:687-691, for all pairs)."""
    if nn_thresh < 0.0:
        raise ValueError("'nn_thresh' should be non-negative")
    d1, d2 = _prep(desc1, "desc1"), _prep(desc2, "desc2")
    if d1.dim() != 3 or d2.dim() != 3 or d1.shape[0] != d2.shape[0] or d1.shape[2] != d2.shape[2]:
        raise ValueError("descriptors must be [B,N1,D] and [B,N2,D]")
    B, N1, D = d1.shape
    N2 = d2.shape[1]
    L = _lib.lib()
    dev = d1.device
    m1 = torch.empty(B, max(N1, 1), device=dev, dtype=torch.int32)
    m2 = torch.empty(B, max(N1, 1), device=dev, dtype=torch.int32)
    sc = torch.empty(B, max(N1, 1), device=dev, dtype=torch.float32)
    cnt = torch.empty(B, device=dev, dtype=torch.int32)
    ws = torch.empty(max(int(L.dfepe_nn_match_workspace_bytes(B, N1, N2)) // 8, 1), device=dev, dtype=torch.int64)
    with _on(dev):
        rc = L.dfepe_nn_match_two_way(_ptr(d1), _ptr(d2), B, N1, N2, D, float(nn_thresh), _ptr(ws), _ptr(m1), _ptr(m2), _ptr(sc),
                                      _ptr(cnt), _stream())
    _lib.check(rc, "dfepe_nn_match_two_way")
    return m1, m2, sc, cnt


def knn_match(desc1: Tensor, desc2: Tensor, ratio: float = 0.8, ratio_test: bool = True):
    """desc1 [B,N1,D], desc2 [B,N2,D] descriptors of any norm -> (nn1, nn2 [B,N1] int32, dist1, dist2 [B,N1], m_idx1, m_idx2
    [B,N1] int32, score [B,N1], count [B] int32): per row the two nearest columns of desc2 by (L2 distance, column index) and
    their distances; the first count[b] entries of m_idx1 / m_idx2 / score are the rows that pass Lowe's ratio test
    ``float64(dist1) < ratio * float64(dist2)`` (all rows with ``ratio_test=False``) in increasing row order, in the layout
    ``gather_matches`` takes (KNN_match with if_BF=True, dsac_tools/utils_opencv.py:39-90, for all pairs)."""
    d1, d2 = _prep(desc1, "desc1"), _prep(desc2, "desc2")
    if d1.dim() != 3 or d2.dim() != 3 or d1.shape[0] != d2.shape[0] or d1.shape[2] != d2.shape[2]:
        raise ValueError("descriptors must be [B,N1,D] and [B,N2,D]")
    B, N1, D = d1.shape
    N2 = d2.shape[1]
    if N2 < 2:
        raise ValueError("knn_match needs at least two descriptors in desc2 (k = 2)")
    L = _lib.lib()
    dev = d1.device
    n = max(N1, 1)
    nn1, nn2, m1, m2 = (torch.empty(B, n, device=dev, dtype=torch.int32) for _ in range(4))
    dist1, dist2, sc = (torch.empty(B, n, device=dev, dtype=torch.float32) for _ in range(3))
    cnt = torch.empty(B, device=dev, dtype=torch.int32)
    ws = torch.empty(max(int(L.dfepe_knn_match_workspace_bytes(B, N1, N2)) // 8, 1), device=dev, dtype=torch.int64)
    with _on(dev):
        rc = L.dfepe_knn_match(_ptr(d1), _ptr(d2), B, N1, N2, D, float(ratio), int(bool(ratio_test)), _ptr(ws), _ptr(nn1), _ptr(nn2),
                               _ptr(dist1), _ptr(dist2), _ptr(m1), _ptr(m2), _ptr(sc), _ptr(cnt), _stream())
    _lib.check(rc, "dfepe_knn_match")
    return nn1, nn2, dist1, dist2, m1, m2, sc, cnt


class _GatherOffsetsFunction(torch.autograd.Function):
    """gather_matches with the offsets attached to off1 / off2: the same launch, and dfepe_gather_offsets_bwd on the way back."""

    @staticmethod
    def forward(ctx, o1, o2, p1, p2, m_idx1, m_idx2, score, choice):
        xs, offs, q = _gather_launch(p1, p2, o1, o2, m_idx1, m_idx2, score, choice)
        ctx.save_for_backward(m_idx1, m_idx2, choice)
        ctx.sizes = (p1.shape[0], p1.shape[1], p2.shape[1])
        ctx.mark_non_differentiable(xs, q)
        return xs, offs, q

    @staticmethod
    def backward(ctx, _gx, g_offs, _gq):
        m_idx1, m_idx2, choice = ctx.saved_tensors
        B, N1, N2 = ctx.sizes
        g = g_offs.contiguous().float()
        g1 = torch.empty(B, N1, 2, device=g.device, dtype=torch.float32)
        g2 = torch.empty(B, N2, 2, device=g.device, dtype=torch.float32)
        with _on(g.device):
            rc = _lib.lib().dfepe_gather_offsets_bwd(_ptr(g), B, N1, N2, _ptr(m_idx1), _ptr(m_idx2), _ptr(choice), choice.shape[1], _ptr(g1),
                                                     _ptr(g2), _stream())
        _lib.check(rc, "dfepe_gather_offsets_bwd")
        return g1, g2, None, None, None, None, None, None


def gather_matches(pts1: Tensor, pts2: Tensor, off1: Optional[Tensor], off2: Optional[Tensor], m_idx1: Tensor, m_idx2: Tensor,
                   score: Tensor, choice: Tensor):
    """choice [B,n_out] int32 positions into each pair's match list -> xs [B,n_out,4], offsets [B,n_out,4] | None,
    quality [B,n_out,1]  (train_good_utils.py:698-716).  Where off1 or off2 requires a gradient, offsets carries it back to them
    (rows that name the same keypoint are added in ascending row order); xs and quality carry none."""
    p1, p2 = _prep(pts1, "pts1"), _prep(pts2, "pts2")
    B, N1, N2 = p1.shape[0], p1.shape[1], p2.shape[1]
    o1 = None if off1 is None else _prep(off1, "off1")
    o2 = None if off2 is None else _prep(off2, "off2")
    if m_idx1.shape != (B, N1) or m_idx1.dtype != torch.int32 or choice.dtype != torch.int32 or not choice.is_contiguous():
        raise ValueError("m_idx1/m_idx2 must be the [B,N1] int32 outputs of nn_match_two_way and choice a contiguous int32 [B,n_out]")
    if o1 is not None and o2 is not None and torch.is_grad_enabled() and (o1.requires_grad or o2.requires_grad):
        _shape(o1, "off1", B, N1, 2)
        _shape(o2, "off2", B, N2, 2)
        if m_idx2.shape != (B, N1) or m_idx2.dtype != torch.int32:
            raise ValueError("m_idx2 must be the [B,N1] int32 output of nn_match_two_way")
        return _GatherOffsetsFunction.apply(o1, o2, p1.detach(), p2.detach(), m_idx1.contiguous(), m_idx2.contiguous(), score, choice)
    return _gather_launch(p1, p2, o1, o2, m_idx1, m_idx2, score, choice)


def _gather_launch(p1, p2, o1, o2, m_idx1, m_idx2, score, choice):
    B, N1, N2 = p1.shape[0], p1.shape[1], p2.shape[1]
    n_out = choice.shape[1]
    dev = p1.device
    xs = torch.empty(B, n_out, 4, device=dev)
    offs = torch.empty(B, n_out, 4, device=dev) if o1 is not None else None
    q = torch.empty(B, n_out, 1, device=dev)
    with _on(dev):
        rc = _lib.lib().dfepe_gather_matches(_ptr(p1), _ptr(p2), _ptr(o1), _ptr(o2), B, N1, N2, _ptr(m_idx1), _ptr(m_idx2), _ptr(score),
                                             _ptr(choice), n_out, _ptr(xs), _ptr(offs), _ptr(q), _stream())
    _lib.check(rc, "dfepe_gather_matches")
    return xs, offs, q
