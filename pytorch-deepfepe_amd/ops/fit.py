"""The weighted eight-point fits and their adjoints (csrc/w8pt*.hip, eight_point_adjoint.hip), and the per-layer row stacks their
outputs are written into."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from ._base import Tensor, _on, _prep, _ptr, _shape, _stream


def save_floats() -> int:
    return _lib.lib().dfepe_save_floats()


# ------------------------------------------------------------------------------------------------
# per-layer stacks without copies.  The reference's API speaks in python lists of per-layer tensors (out_layers,
# E_ests_layers, q_l2_error_layers_list ...; DeepFNet.py:534-548, train_good_utils.py:272-293) and glues them with
# torch.stack; the kernels want one [L, ...] buffer.  These helpers let both views share the memory: the rows of a stack are
# handed out as separate autograd outputs (no SelectBackward that would zero-fill and copy a full stack per row in the
# backward), and a list whose tensors turn out to be the rows of one buffer is re-assembled without a copy kernel.
# ------------------------------------------------------------------------------------------------
def row_of(stack: Tensor, l: int) -> Tensor:
    """Row l of a contiguous [L, ...] buffer as a tensor of its own over the same memory (not an autograd view of it)."""
    n = stack[0].numel()
    t = torch.empty(0, dtype=stack.dtype, device=stack.device)
    t.set_(stack.untyped_storage(), stack.storage_offset() + l * n, tuple(stack.shape[1:]), None)
    return t


def alias_rows(rows) -> Optional[Tensor]:
    """[len(rows), *shape] tensor over the memory of ``rows`` when they are equally shaped contiguous tensors lying at a uniform
    distance from each other in one buffer, in order (back to back: the result is contiguous; further apart -- e.g. the same
    channel of consecutive per-layer buffers -- it is a strided view); None otherwise (the caller then copies)."""
    if len(rows) == 0 or rows[0] is None:
        return None
    r0 = rows[0]
    n = r0.numel()
    if n == 0:
        return None
    base = r0.untyped_storage().data_ptr()
    step = n if len(rows) == 1 else (rows[1].storage_offset() - r0.storage_offset() if rows[1] is not None else -1)
    if step < n:
        return None
    for l, r in enumerate(rows):
        if (r is None or r.shape != r0.shape or r.dtype != r0.dtype or r.device != r0.device or not r.is_contiguous()
                or r.untyped_storage().data_ptr() != base or r.storage_offset() != r0.storage_offset() + l * step):
            return None
    t = torch.empty(0, dtype=r0.dtype, device=r0.device)
    t.set_(r0.untyped_storage(), r0.storage_offset(), (len(rows),) + tuple(r0.shape), (step,) + tuple(r0.stride()))
    return t


class _StackRowsFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *rows):
        ctx.set_materialize_grads(False)  # an unused stack must not send rows of zeros back (a zero-fill, and kernels that then
        ctx.n = len(rows)                 # run their gradient paths for nothing)
        a = alias_rows(rows)
        if a is None:
            return torch.stack(rows)
        # the result is a tensor of its own over the rows' memory, so autograd's version counters of the rows do not cover it.
        # The rows are therefore saved: an in-place write to any of them between here and the backward makes the saved-tensor
        # check below raise ("modified by an inplace operation") instead of silently corrupting what a kernel saved of the stack
        ctx.save_for_backward(*rows)
        return a

    @staticmethod
    def backward(ctx, g):
        ctx.saved_tensors  # the version check of every aliased row (no-op when the rows were copied)
        return (None,) * ctx.n if g is None else tuple(g.unbind(0))


class _UnstackRowsFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.meta = (x.shape, x.dtype, x.device)
        ctx.set_materialize_grads(False)
        x = x if x.is_contiguous() else x.contiguous()
        # real views of x: they share x's version counter, and autograd forbids in-place writes to the outputs of a function that
        # returns several views ("...is a view and is being modified inplace"), so a caller cannot silently overwrite a row of a
        # stack that some kernel saved for its backward.  Their grad_fn is still THIS node (no SelectBackward per row).
        return tuple(x[l] for l in range(x.shape[0]))

    @staticmethod
    def backward(ctx, *gs):
        shape, dtype, dev = ctx.meta
        if all(g is None for g in gs):
            return None
        a = alias_rows(gs)  # torch.stack's backward hands out the rows of one gradient buffer: taken as it is
        if a is not None:
            return a
        return torch.stack([torch.zeros(shape[1:], dtype=dtype, device=dev) if g is None else g for g in gs])


def stack_rows(rows) -> Tensor:
    """torch.stack(rows) without the copy when the rows already are the consecutive slices of one buffer."""
    rows = list(rows)
    return _StackRowsFunction.apply(*rows)


def unstack_rows(x: Tensor):
    """The rows of x [L, ...] as a tuple of L views of x, each an autograd output of its own (and, like the outputs of
    torch.unbind, not writable in place while gradients are tracked)."""
    return _UnstackRowsFunction.apply(x)


# ------------------------------------------------------------------------------------------------
# weighted 8-point fit
# ------------------------------------------------------------------------------------------------
def _flags(raw: bool, logits: bool, row_per_pair: bool = False, extra: int = 0) -> int:
    return ((_lib.W8PT_RAW_MATCHES if raw else 0) | (_lib.W8PT_LOGITS if logits else 0) |
            (_lib.W8PT_ROW_PER_PAIR if row_per_pair else 0) | int(extra))


def w8pt_forward(pts1: Tensor, pts2: Optional[Tensor], weights: Tensor, raw: bool, image_w: float, image_h: float,
                 clamp_at: float, want_epi: bool, want_save: bool, logits: bool = False, F_out: Optional[Tensor] = None,
                 row_per_pair: bool = False, extra_flags: int = 0, dst: Optional[dict] = None, hartley: Optional[tuple] = None):
    """Raw (non-differentiable) launch.  weights (or logits when ``logits``) [B,N].
    Returns F [B,3,3], residual [B,N], epi [B,N]|None, save|None, weights_out [B,N]|None.  ``F_out`` lets the caller
    provide the destination (e.g. one [B,3,3] slice of a per-layer stack).  ``row_per_pair`` forces one 16-lane row per pair
    where a cooperative workgroup per pair (N > 128 at small batch) would run: same function, same ``save`` record.
    ``dst``: {"F" | "residual" | "epi" | "weights": (stack, l)} writes that output into row l of the caller's per-layer stack.
    ``hartley``: (buffer, mode) -- the Hartley record of dfepe_w8pt_fwd_shared (``hartley_record(B, device)``) and
    _lib.HARTLEY_WRITE / HARTLEY_READ: a fit of the same correspondences, image size and Hartley flags as an earlier one on this
    stream takes the transforms of Fit.normalize from it; the outputs are the same bit for bit."""
    L = _lib.lib()
    B, N = weights.shape
    dev = weights.device
    dst = dst or {}
    hbuf, hmode = (None, _lib.HARTLEY_NONE) if hartley is None else hartley
    if hbuf is not None and (hbuf.dtype != torch.float64 or hbuf.device != dev or not hbuf.is_contiguous() or
                             hbuf.numel() < pts1.shape[0] * _lib.HARTLEY_DOUBLES):
        raise ValueError(f"hartley buffer must be a contiguous float64 [{pts1.shape[0]}, {_lib.HARTLEY_DOUBLES}] tensor on {dev}")

    def out(name, shape, want=True):
        if not want:
            return None
        if name in dst:
            stack, l = dst[name]
            if tuple(stack.shape[1:]) != tuple(shape) or stack.dtype != torch.float32 or not stack.is_contiguous():
                raise ValueError(f"dst[{name!r}] must be a contiguous float32 stack of {tuple(shape)} rows, got {tuple(stack.shape)}")
            return row_of(stack, l)
        return torch.empty(*shape, device=dev, dtype=torch.float32)

    F = out("F", (B, 3, 3)) if F_out is None else F_out
    residual = out("residual", (B, N))
    epi = out("epi", (B, N), want_epi)
    save = torch.empty(B, L.dfepe_save_floats(), device=dev, dtype=torch.float32) if want_save else None
    w_out = out("weights", (B, N), logits)
    with _on(dev):
        rc = L.dfepe_w8pt_fwd_shared(_ptr(pts1), _ptr(pts2), _ptr(weights), B, N, 1, _flags(raw, logits, row_per_pair, extra_flags),
                                     float(image_w), float(image_h), float(clamp_at), _ptr(F), _ptr(residual), _ptr(epi), _ptr(save),
                                     _ptr(w_out), _ptr(hbuf), int(hmode), _stream())
    _lib.check(rc, "dfepe_w8pt_fwd_shared")
    return F, residual, epi, save, w_out


def hartley_record(B: int, device) -> Tensor:
    """A Hartley record for B pairs (w8pt_forward(hartley=...)): from the caching allocator, so a captured step owns it."""
    return torch.empty(B, _lib.HARTLEY_DOUBLES, device=device, dtype=torch.float64)


def w8pt_backward(pts1, pts2, weights, raw, image_w, image_h, clamp_at, save, F, gF, gRes, gEpi, logits=False, gW_extra=None,
                  out: Optional[Tensor] = None, want_pts: bool = False, row_per_pair: bool = False, g_scale: Optional[Tensor] = None,
                  pending_loss_head: Optional[Tensor] = None, extra_flags: int = 0):
    """Raw launch of the adjoint; returns d/d(weights) (or d/d(logits) when ``logits``; then ``weights`` must be the
    forward's weights_out) and, when ``want_pts``, the gradients w.r.t. the points ([B,N,3] x 2, or [B,N,4] for raw matches)."""
    L = _lib.lib()
    B, N = weights.shape
    gW = torch.empty_like(weights) if out is None else out
    gP1 = gP2 = None
    if want_pts:
        gP1 = torch.empty_like(pts1)
        gP2 = None if raw else torch.empty_like(pts2)
    with _on(weights.device):
        rc = L.dfepe_w8pt_bwd(_ptr(pts1), _ptr(pts2), _ptr(weights), B, N, 1, _flags(raw, logits, row_per_pair, extra_flags), float(image_w), float(image_h),
                              float(clamp_at), _ptr(save), _ptr(F), _ptr(gF), _ptr(gRes), _ptr(gEpi), _ptr(gW_extra), _ptr(g_scale), _ptr(gW),
                              _ptr(gP1), _ptr(gP2), _ptr(pending_loss_head), _stream())
    _lib.check(rc, "dfepe_w8pt_bwd")
    return (gW, gP1, gP2) if want_pts else gW


def _eight_point_flags(essential: bool, normalize: bool) -> int:
    return (_lib.W8PT_SQRT2 | _lib.W8PT_NO_ROWNORM | (_lib.W8PT_FORCE_110 if essential else 0) |
            (0 if normalize else _lib.W8PT_NO_HARTLEY))


def _eight_point_launch(X: Tensor, Y: Tensor, w: Optional[Tensor], S: int, essential: bool, normalize: bool) -> Tensor:
    """The forward fit: X, Y [B,N,2] and w [S,B,N] (None = ones, S = 1), prepared -> F [S,B,3,3]."""
    B, N = X.shape[0], X.shape[1]
    ones = torch.ones(B, N, 1, device=X.device)
    p1 = torch.cat((X, ones), 2).contiguous()
    p2 = torch.cat((Y, ones), 2).contiguous()
    wt = torch.ones(B, N, device=X.device) if w is None else w
    L = _lib.lib()
    F = torch.empty(S, B, 3, 3, device=X.device)
    residual = torch.empty(S, B, N, device=X.device)
    with _on(X.device):
        rc = L.dfepe_w8pt_fwd(_ptr(p1), _ptr(p2), _ptr(wt), B, N, S, _eight_point_flags(essential, normalize), 0.0, 0.0, 0.5, _ptr(F),
                              _ptr(residual), None, None, None, _stream())
    _lib.check(rc, "dfepe_w8pt_fwd")
    return F


class _EightPointFunction(torch.autograd.Function):
    """The fit with its adjoint (dfepe_eight_point_bwd: the fit is recomputed in fp64, nothing but the inputs and F is saved)."""

    @staticmethod
    def forward(ctx, X, Y, w, S, essential, normalize):
        F = _eight_point_launch(X, Y, w, S, essential, normalize)
        ctx.save_for_backward(X, Y, w, F)
        ctx.cfg = (S, essential, normalize)
        return F

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        X, Y, w, F = ctx.saved_tensors
        S, essential, normalize = ctx.cfg
        B, N = X.shape[0], X.shape[1]
        g = g.contiguous().float()
        need = ctx.needs_input_grad
        gX = torch.empty_like(X) if need[0] else None
        gY = torch.empty_like(Y) if need[1] else None
        gw = torch.empty_like(w) if (w is not None and need[2]) else None
        L = _lib.lib()
        nbytes = int(L.dfepe_eight_point_bwd_workspace_bytes(B, N, S)) if (gX is not None or gY is not None) else 0
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=X.device) if nbytes else None
        with _on(X.device):
            rc = L.dfepe_eight_point_bwd(_stream(), _ptr(X), _ptr(Y), _ptr(w), B, N, S, _eight_point_flags(essential, normalize), _ptr(F),
                                         _ptr(g), _ptr(gX), _ptr(gY), _ptr(gw), _ptr(ws))
        _lib.check(rc, "dfepe_eight_point_bwd")
        return gX, gY, gw, None, None, None


def eight_point(X: Tensor, Y: Tensor, w: Optional[Tensor], essential: bool, normalize: bool = True) -> Tensor:
    """Textbook normalised 8-point on 2-D points X, Y [B,N,2] with optional per-correspondence weights [B,N]
    (utils_F._F_from_XY / _E_from_XY after the K^-1 step): sqrt(2) Hartley (none when ``normalize`` is False),
    unnormalised rows, S3 -> 0 or (1,1,0).  Returns F [B,3,3].
    w [S,B,N] with S > 1: S weightings of the same B pairs in one launch; returns [S,B,3,3] (a leading dimension of 1 is the
    single weighting it always was and returns [B,3,3]).
    Differentiable w.r.t. X, Y and w (dfepe_eight_point_bwd; with several weightings the point gradients are their sum).  The
    Hartley transforms are constants of the adjoint, as the reference's own autograd has them (utils_F.py:25,35).  With nothing
    requiring grad it is the forward launch alone."""
    X, Y = _prep(X, "X"), _prep(Y, "Y")
    B, N = X.shape[0], X.shape[1]
    sets = w is not None and w.dim() == 3 and w.shape[0] > 1 and tuple(w.shape[1:]) == (B, N)
    S = w.shape[0] if sets else 1
    wt = None if w is None else _prep(w if sets else w.reshape(B, N), "w").reshape(S, B, N)
    if torch.is_grad_enabled() and (X.requires_grad or Y.requires_grad or (wt is not None and wt.requires_grad)):
        if X.dim() != 3 or X.shape[2] != 2 or Y.shape != X.shape:
            raise ValueError(f"eight_point: X and Y [B,N,2] expected, got {tuple(X.shape)}, {tuple(Y.shape)}")
        # the adjoint reads the points as 8-byte pairs: a contiguous view that starts at an odd element of its buffer is copied
        X, Y = (t.clone() if t.data_ptr() % 8 else t for t in (X, Y))
        F = _EightPointFunction.apply(X, Y, wt, S, essential, normalize)
    else:
        F = _eight_point_launch(X, Y, wt, S, essential, normalize)
    return F if sets else F[0]


def eight_point_rows(rows: Tensor, T1: Optional[Tensor], T2: Optional[Tensor], essential: bool) -> Tensor:
    """Closing steps of the textbook solvers on an explicit design matrix rows [B,N,9] (the dense-W form,
    utils_F.py:129-155,245-275): smallest right singular vector, S3 -> 0 or (1,1,0), T2^T F T1 (T1, T2 [B,3,3] or None)."""
    rows = _prep(rows, "rows")
    _shape(rows, "rows (design matrix)", None, None, 9)
    B, N = rows.shape[0], rows.shape[1]
    if (T1 is None) != (T2 is None):
        raise ValueError("T1 and T2 come together")
    if T1 is not None:
        T1, T2 = _prep(T1, "T1"), _prep(T2, "T2")
        _shape(T1, "T1", B, 3, 3)
        _shape(T2, "T2", B, 3, 3)
    F = torch.empty(B, 3, 3, device=rows.device)
    with _on(rows.device):
        rc = _lib.lib().dfepe_w8pt_rows_fwd(_ptr(rows), B, N, _lib.W8PT_FORCE_110 if essential else 0, _ptr(T1), _ptr(T2), _ptr(F), _stream())
    _lib.check(rc, "dfepe_w8pt_rows_fwd")
    return F


def _cf(t: Optional[Tensor]) -> Optional[Tensor]:
    return None if t is None else t.contiguous().float()


class _W8ptFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pts1, pts2, weights, raw, image_w, image_h, clamp_at, want_epi, logits, extra_flags=0, dst=None, hartley=None):
        ctx.set_materialize_grads(False)  # unused outputs (e.g. the last layer's epi) must not cost a zero-fill
        F, residual, epi, save, w_out = w8pt_forward(pts1, pts2, weights, raw, image_w, image_h, clamp_at, want_epi,
                                                     want_save=True, logits=logits, extra_flags=extra_flags, dst=dst, hartley=hartley)
        ctx.extra_flags = extra_flags
        ctx.save_for_backward(pts1, pts2 if pts2 is not None else pts1.new_empty(0), w_out if logits else weights, save, F)
        ctx.cfg = (raw, image_w, image_h, clamp_at, want_epi, logits)
        outs = [F, residual]
        if want_epi:
            outs.append(epi)
        if logits:
            outs.append(w_out)
        return tuple(outs)

    @staticmethod
    def backward(ctx, gF, gRes, *rest):
        pts1, pts2, weights, save, F = ctx.saved_tensors
        raw, image_w, image_h, clamp_at, want_epi, logits = ctx.cfg
        rest = list(rest)
        gEpi = rest.pop(0) if want_epi else None
        gWout = rest.pop(0) if logits else None
        if gF is None and gRes is None and gEpi is None and gWout is None:
            return (None,) * 12
        want_pts = ctx.needs_input_grad[0] or (not raw and ctx.needs_input_grad[1])
        res = w8pt_backward(pts1, pts2 if pts2.numel() else None, weights, raw, image_w, image_h, clamp_at, save, F,
                            _cf(gF), _cf(gRes), _cf(gEpi), logits=logits, gW_extra=_cf(gWout), want_pts=want_pts,
                            extra_flags=ctx.extra_flags)
        if want_pts:
            gW, gP1, gP2 = res
            return gP1, gP2, gW, None, None, None, None, None, None, None, None, None
        return None, None, res, None, None, None, None, None, None, None, None, None


def w8pt(pts1: Tensor, pts2: Tensor, weights: Tensor, clamp_at: float = 0.5, want_epi: bool = False, normalize_rows: bool = True):
    """Differentiable fit on homogeneous points [B,N,3]; weights [B,N] or [B,1,N].  Gradients flow to the weights and,
    when the point tensors require grad, to both point sets.  ``normalize_rows=False`` = Fit(normalize_SVD=False)
    (DeepFNet.py:211): the design rows enter X un-normalised; gradients then flow to the weights only."""
    pts1, pts2 = _prep(pts1, "pts1"), _prep(pts2, "pts2")
    w = _prep(weights.reshape(weights.shape[0], -1), "weights")
    B, N = w.shape
    _shape(pts1, "pts1 (homogeneous points)", B, N, 3)
    _shape(pts2, "pts2 (homogeneous points)", B, N, 3)
    if not normalize_rows and torch.is_grad_enabled() and (pts1.requires_grad or pts2.requires_grad):
        raise _lib.DfepeError("w8pt(normalize_rows=False): gradients w.r.t. the points are not built for un-normalised rows")
    return _W8ptFunction.apply(pts1, pts2, w, False, 0.0, 0.0, clamp_at, want_epi, False, 0 if normalize_rows else _lib.W8PT_NO_ROWNORM)


def w8pt_raw(matches: Tensor, weights: Tensor, image_w: float, image_h: float, clamp_at: float = 0.5,
             want_epi: bool = True, hartley: Optional[tuple] = None):
    """Differentiable fit straight from pixel matches [B,N,4] (image-size normalisation fused).  ``hartley``: see w8pt_forward."""
    m = _prep(matches, "matches")
    w = _prep(weights.reshape(weights.shape[0], -1), "weights")
    _shape(m, "matches (pixel x1,y1,x2,y2)", w.shape[0], w.shape[1], 4)
    return _W8ptFunction.apply(m, None, w, True, float(image_w), float(image_h), clamp_at, want_epi, False, 0, None, hartley)


def w8pt_raw_logits(matches: Tensor, logits: Tensor, image_w: float, image_h: float, clamp_at: float = 0.5,
                    want_epi: bool = True, dst: Optional[dict] = None, hartley: Optional[tuple] = None):
    """As w8pt_raw but takes the estimator's logits and fuses F.softmax(dim=N); additionally returns the weights
    (differentiable: the next estimator layer consumes them).  Returns (F, residual[, epi], weights).
    ``dst`` (see w8pt_forward): rows of the caller's per-layer stacks to write the outputs into.
    ``hartley`` (see w8pt_forward): (record, mode), for a model that fits the same matches at every layer."""
    m = _prep(matches, "matches")
    l = _prep(logits.reshape(logits.shape[0], -1), "logits")
    _shape(m, "matches (pixel x1,y1,x2,y2)", l.shape[0], l.shape[1], 4)
    return _W8ptFunction.apply(m, None, l, True, float(image_w), float(image_h), clamp_at, want_epi, True, 0, dst, hartley)
