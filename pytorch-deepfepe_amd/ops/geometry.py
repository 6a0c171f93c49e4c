"""The small pose helpers, the model's input builders, the cheirality check and the fit that ends in it (csrc/geom.hip,
cheirality_body.h; dfepe_w8pt_pose_fwd of csrc/w8pt16.hip)."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from ._base import Tensor, _on, _prep, _ptr, _shape, _stream
from .fit import _flags


_GEO_OUT = {0: 4, 1: 1, 2: 1, 3: 9, 4: 21, 5: 9, 6: 9}


def geo_misc(kind: int, in0: Tensor, in1: Optional[Tensor] = None) -> Tensor:
    in0 = _prep(in0, "in0")
    in1 = None if in1 is None else _prep(in1, "in1")
    n = in0.shape[0]
    out = torch.empty(n, _GEO_OUT[kind], device=in0.device, dtype=torch.float32)
    with _on(in0.device):
        rc = _lib.lib().dfepe_geo_misc(int(kind), _ptr(in0), _ptr(in1), n, _ptr(out), _stream())
    _lib.check(rc, "dfepe_geo_misc")
    return out


def rot_to_quat(R: Tensor) -> Tensor:
    return geo_misc(0, R.reshape(-1, 9))


def rot_angle_deg(R0: Tensor, R1: Tensor) -> Tensor:
    return geo_misc(1, R0.reshape(-1, 9), R1.reshape(-1, 9))[:, 0]


def vector_angle_deg(v1: Tensor, v2: Tensor) -> Tensor:
    return geo_misc(2, v1.reshape(-1, 3), v2.reshape(-1, 3))[:, 0]


def project_essential(E: Tensor) -> Tensor:
    return geo_misc(3, E.reshape(-1, 9)).reshape(-1, 3, 3)


def congruence(F: Tensor, A: Tensor) -> Tensor:
    """A^T F A for batches of 3x3 matrices: E = K^T T^T F T K with A = T K (train_good_utils.py:356-358), or K^T F K."""
    return geo_misc(5, F.reshape(-1, 9), A.reshape(-1, 9)).reshape(-1, 3, 3)


class _RowDotFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        ctx.set_materialize_grads(False)
        n, B, N = a.shape
        out = torch.empty(n, B, device=a.device, dtype=torch.float32)
        with _on(a.device):
            rc = _lib.lib().dfepe_row_dot(_ptr(a), a.stride(0), _ptr(b), b.stride(0), n, B, N, _ptr(out), _stream())
        _lib.check(rc, "dfepe_row_dot")
        ctx.save_for_backward(a, b)
        return out

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None
        a, b = ctx.saved_tensors
        g = g.unsqueeze(2)
        return (g * b if ctx.needs_input_grad[0] else None), (g * a if ctx.needs_input_grad[1] else None)


def row_dot(a: Tensor, b: Tensor) -> Tensor:
    """out[l,b] = sum_n a[l,b,n] * b[l,b,n] for two [n,B,N] stacks whose layers are contiguous [B,N] blocks (any distance apart:
    the strided stacks of alias_rows are taken as they are).  One launch; differentiable (plain torch products in the backward)."""
    if a.shape != b.shape or a.dim() != 3:
        raise ValueError(f"row_dot: two [n,B,N] stacks expected, got {tuple(a.shape)}, {tuple(b.shape)}")
    fix = lambda t: t if (t.is_cuda and t.dtype == torch.float32 and t.stride(2) == 1 and t.stride(1) == t.shape[2]) else _prep(t, "stack")
    return _RowDotFunction.apply(fix(a), fix(b))


class _CongruenceFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, F, A):
        ctx.save_for_backward(A)
        return geo_misc(5, F.reshape(-1, 9), A.reshape(-1, 9)).reshape(-1, 3, 3)

    @staticmethod
    def backward(ctx, g):
        A, = ctx.saved_tensors
        return geo_misc(5, g.reshape(-1, 9), A.transpose(1, 2).reshape(-1, 9)).reshape(-1, 3, 3), None  # A g A^T


def congruence_diff(F: Tensor, A: Tensor) -> Tensor:
    """A^T F A like congruence, differentiable w.r.t. F (F_ests = T^T F_est T of get_all_loss_DeepF, train_good_utils.py:366)."""
    return _CongruenceFunction.apply(_prep(F, "F"), _prep(A, "A"))


def camera_rotation(delta_4x4: Tensor) -> Tensor:
    """inv(delta)[:, :3, :3] for scene motions delta [B,4,4]: the ground-truth camera rotation of get_Rt_loss
    (train_good_utils.py:134,170), one launch, no LAPACK round trip / host synchronisation."""
    d = _prep(delta_4x4, "delta_Rtijs_4_4")
    _shape(d, "delta_Rtijs_4_4", None, 4, 4)
    return geo_misc(6, d.reshape(-1, 16)).reshape(-1, 3, 3)


def deepf_input(matches: Tensor, image_w: float, image_h: float, quality: Optional[Tensor] = None, want_pts: bool = True,
                recurrent_copies: int = 0, recurrent_channels: int = 3):
    """DeepFNet.get_input in one launch (DeepFNet.py:362-391): matches [B,N,4] pixels (+ quality [B,N,Q]) ->
    (weight_in [B,4+Q,N], pts1 [B,N,3], pts2 [B,N,3], stores); not differentiable (the matches are data).
    ``recurrent_copies`` = n > 0: the same launch also fills the point (and quality) channels of n channel-major buffers
    ``stores`` [n, 4+Q+recurrent_channels, B, N] -- the inputs of the later estimator calls (DeepFNet.py:484-489), whose remaining
    channels the fit kernels write as plain [B,N] blocks; weight_in then is a [B,4+Q,N] view of one more such buffer."""
    m = _prep(matches, "matches")
    _shape(m, "matches (pixel x1,y1,x2,y2)", None, None, 4)
    B, N = m.shape[0], m.shape[1]
    Q = 0
    if quality is not None:
        quality = _prep(quality, "quality")
        _shape(quality, "quality", B, N, None)
        Q = quality.shape[2]
    dev = m.device
    p1 = torch.empty(B, N, 3, device=dev, dtype=torch.float32) if want_pts else None
    p2 = torch.empty(B, N, 3, device=dev, dtype=torch.float32) if want_pts else None
    lib = _lib.lib()
    if recurrent_copies > 0:
        C = 4 + Q + recurrent_channels
        buf = torch.empty(recurrent_copies + 1, C, B, N, device=dev, dtype=torch.float32)  # copy 0 serves the first estimator call
        with _on(dev):
            rc = lib.dfepe_deepf_input(_ptr(m), _ptr(quality), B, N, Q, float(image_w), float(image_h), _ptr(buf), B * N, N,
                                       recurrent_copies + 1, C * B * N, _ptr(p1), _ptr(p2), _stream())
        _lib.check(rc, "dfepe_deepf_input")
        return buf[0, :4 + Q].permute(1, 0, 2), p1, p2, buf[1:]
    w_in = torch.empty(B, 4 + Q, N, device=dev, dtype=torch.float32)
    with _on(dev):
        rc = lib.dfepe_deepf_input(_ptr(m), _ptr(quality), B, N, Q, float(image_w), float(image_h), _ptr(w_in), N, (4 + Q) * N, 1, 0,
                                   _ptr(p1), _ptr(p2), _stream())
    _lib.check(rc, "dfepe_deepf_input")
    return w_in, p1, p2, None


class _EstimatorInputFunction(torch.autograd.Function):
    """The [B,C,N] input of an update_weights call (DeepFNet.py:484-489: cat of the point channels, weights, epipolar residual,
    residual) WITHOUT the cat: ``store`` [C,B,N] already holds the point channels (deepf_input) and the three recurrent channels
    (the fit kernel wrote its outputs there: ``rec`` are those very rows); the result is the channel-major buffer seen as [B,C,N].
    Backward: the gradient's three recurrent channels go to the rows."""

    @staticmethod
    def forward(ctx, store, first, *rec):
        ctx.first = first
        out = torch.empty(0, dtype=store.dtype, device=store.device)
        C, B, N = store.shape
        out.set_(store.untyped_storage(), store.storage_offset(), (B, C, N), (N, B * N, 1))
        return out

    @staticmethod
    def backward(ctx, g):
        return (None, None) + tuple(g[:, ctx.first + k, :] for k in range(g.shape[1] - ctx.first))


def estimator_input(store: Tensor, first: int, rec_rows) -> Tensor:
    """See _EstimatorInputFunction: store [C,B,N] channel-major, rec_rows = the [B,N] tensors living in store[first:], in order."""
    for k, r in enumerate(rec_rows):
        if r.data_ptr() != store[first + k].data_ptr() or r.shape != store.shape[1:]:
            raise ValueError("estimator_input: the recurrent rows must be the channels of the store they were written into")
    return _EstimatorInputFunction.apply(store, first, *rec_rows)


def decompose_essential(E: Tensor):
    o = geo_misc(4, E.reshape(-1, 9))
    return o[:, 0:9].reshape(-1, 3, 3), o[:, 9:18].reshape(-1, 3, 3), o[:, 18:21]


def _cheirality_workspace(B: int, dev) -> Tensor:
    """Per-call scratch of dfepe_cheirality_ex (the per-pair constants its preparation launch leaves for the main kernel)."""
    return torch.empty((_lib.lib().dfepe_cheirality_workspace_bytes(B) + 7) // 8, dtype=torch.float64, device=dev)


def cheirality(E: Tensor, K: Tensor, matches: Tensor, depth_thres: float = 50.0, pre: Optional[Tensor] = None, fp64_only: bool = False,
               prepared: Optional[bool] = None):
    """E, K [B,3,3], matches [B,N,4] pixels -> (Rt_cam [B,3,4], winner [B] int32, counts [B,4] int32).
    ``pre`` [B,3,3]: decompose pre^T E pre instead (E = F and pre = T K fuses E-from-F into the launch).
    ``fp64_only``: every correspondence through the fp64 route (DFEPE_CHEIR_FP64_ONLY: the reference the adaptive default is
    tested against for exact equality of the counts).  ``prepared``: form the per-pair constants in a preparation launch (one lane
    per pair) instead of in the main kernel; same outputs bit for bit.  Default: from 2048 pairs on (measured 93.8 vs 98.7 us at
    4096 x 1000; below, where a pair's workgroup forms them once and shares them through LDS, the second launch costs more than it
    saves: 22.9 vs 21.1 us at 512 x 1000)."""
    E, K, m = _prep(E, "E"), _prep(K, "K"), _prep(matches, "matches")
    pre = None if pre is None else _prep(pre, "pre")
    _shape(m, "matches (pixel x1,y1,x2,y2)", None, None, 4)
    B, N = m.shape[0], m.shape[1]
    _shape(E, "E", B, 3, 3)
    _shape(K, "K (one intrinsic matrix per pair)", B, 3, 3)
    if pre is not None:
        _shape(pre, "pre", B, 3, 3)
    Rt = torch.empty(B, 3, 4, device=m.device, dtype=torch.float32)
    win = torch.empty(B, device=m.device, dtype=torch.int32)
    cnt = torch.empty(B, 4, device=m.device, dtype=torch.int32)
    ws = _cheirality_workspace(B, m.device) if (prepared if prepared is not None else B >= 2048) else None
    with _on(m.device):
        rc = _lib.lib().dfepe_cheirality_ex(_ptr(E), _ptr(pre), _ptr(K), _ptr(m), B, N, float(depth_thres),
                                            _lib.CHEIR_FP64_ONLY if fp64_only else 0, _ptr(ws), _ptr(Rt), _ptr(win), _ptr(cnt), _stream())
    _lib.check(rc, "dfepe_cheirality_ex")
    return Rt, win, cnt


def fit_pose(matches: Tensor, weights: Tensor, K: Tensor, image_w: float, image_h: float, depth_thres: float = 50.0,
             pre: Optional[Tensor] = None, clamp_at: float = 0.5, want_epi: bool = True, logits: bool = False, row_per_pair: bool = False):
    """One weighted 8-point fit and the cheirality-checked pose of its F (BASELINE config 5): w8pt_forward followed by
    cheirality(F, K, matches, depth_thres, pre=pre), same numbers, ONE launch when a cooperative workgroup serves the pair
    (128 < N <= 2048 up to 1280 pairs: the forward fit's rule for pixel matches, csrc/fit_plan.h; the backward fit keeps the
    cooperative workgroup up to 3072 pairs).  Returns (F, residual, epi | None, weights_out | None, Rt_cam, winner, counts)."""
    m, w, K = _prep(matches, "matches"), _prep(weights, "weights"), _prep(K, "K")
    pre = None if pre is None else _prep(pre, "pre")
    _shape(m, "matches (pixel x1,y1,x2,y2)", None, None, 4)
    B, N = m.shape[0], m.shape[1]
    _shape(w, "weights", B, N)
    _shape(K, "K (one intrinsic matrix per pair)", B, 3, 3)
    if pre is not None:
        _shape(pre, "pre", B, 3, 3)
    dev = m.device
    F = torch.empty(B, 3, 3, device=dev)
    residual = torch.empty(B, N, device=dev)
    epi = torch.empty(B, N, device=dev) if want_epi else None
    w_out = torch.empty(B, N, device=dev) if logits else None
    Rt = torch.empty(B, 3, 4, device=dev)
    win = torch.empty(B, device=dev, dtype=torch.int32)
    cnt = torch.empty(B, 4, device=dev, dtype=torch.int32)
    ws = _cheirality_workspace(B, dev) if B >= 2048 else None
    with _on(dev):
        rc = _lib.lib().dfepe_w8pt_pose_fwd(_ptr(m), _ptr(w), B, N, _flags(True, logits, row_per_pair), float(image_w), float(image_h), float(clamp_at),
                                            _ptr(K), _ptr(pre), float(depth_thres), _ptr(F), _ptr(residual), _ptr(epi), _ptr(w_out), _ptr(Rt), _ptr(win),
                                            _ptr(cnt), _ptr(ws), _stream())
    _lib.check(rc, "dfepe_w8pt_pose_fwd")
    return F, residual, epi, w_out, Rt, win, cnt
