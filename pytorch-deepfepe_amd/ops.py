"""torch.autograd wrappers over the C ABI (device memory and streams come from PyTorch-ROCm; the
arithmetic is entirely in libdfepe_hip.so)."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib

Tensor = torch.Tensor


def _ptr(t: Optional[Tensor]):
    return None if t is None else t.data_ptr()


# Host cost of a launch (scripts/eager_profile.py: the reference's eager call sequence is host-bound, ~50 launches per step):
# torch.cuda.current_stream().cuda_stream builds a Stream object per call (~10 us) and torch.cuda.device() is a python context
# manager doing two device queries (~8 us) -- the raw C entry points below do the same in well under a microsecond each.
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream() -> int:
    """The current HIP stream of the current device, as the integer handle the C ABI takes."""
    if _raw_stream is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream


class _NoGuard:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_GUARD = _NoGuard()


def _on(dev):
    """`with _on(t.device):` = `with torch.cuda.device(t.device):` without the context-manager cost when that device is already
    the current one (every call of a single-GPU process, and of a rank that called torch.cuda.set_device)."""
    if _cur_device is not None and dev.index is not None and dev.index == _cur_device():
        return _NO_GUARD
    return torch.cuda.device(dev)


def _prep(t: Tensor, name: str) -> Tensor:
    if not t.is_cuda:
        raise _lib.DfepeError(f"{name} must live on the GPU (this package has no CPU path)")
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _shape(t: Tensor, name: str, *dims) -> None:
    """Raise ValueError unless t has the given shape (None = any size): the kernels index raw pointers, so a wrong
    layout would be a silent out-of-bounds read, not an exception."""
    if t.dim() != len(dims) or any(d is not None and t.shape[i] != d for i, d in enumerate(dims)):
        want = "[" + ",".join("?" if d is None else str(d) for d in dims) + "]"
        raise ValueError(f"{name} must have shape {want}, got {tuple(t.shape)}")


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


def ransac_fundamental(matches: Tensor, threshold: float = 0.1, confidence: float = 0.99, max_iters: int = 1000, seed: int = 0,
                       want_hyp_counts: bool = False, want_masked: bool = False):
    """matches [B,N,4] pixels -> robust F of every pair by OpenCV 3.4's findFundamentalMat(FM_RANSAC) algorithm (the validation
    baseline, utils_opencv.py:157; include/dfepe.h spells out the sampler, the 7-point solve, the error and the stopping rule).
    Returns dict(F [B,3,3] (F22 = 1; zeros without a model), mask [B,N] uint8, n_inliers [B], iters_run [B], best_hyp [B,2]
    (iteration, root; -1 without a model), hyp_counts [B,max_iters,3] | None (-1: no root, -2: no sample), masked [B,N,4] | None
    (non-inlier rows NaN)).  No host synchronisation.  15 <= N <= 4096: below 15 OpenCV runs LMedS, which is lmeds_fundamental."""
    m = _prep(matches, "matches")
    _shape(m, "matches (pixel x1,y1,x2,y2)", None, None, 4)
    B, N = m.shape[0], m.shape[1]
    if N < _lib.RANSAC_MIN_N:
        raise _lib.DfepeError(f"ransac_fundamental: {N} correspondences per pair; the RANSAC estimator needs at least "
                              f"{_lib.RANSAC_MIN_N} (OpenCV switches to LMedS below that, which is not built into this entry: see lmeds_fundamental)")
    L = _lib.lib()
    dev = m.device
    ws = torch.empty(max(1, (int(L.dfepe_ransac_workspace_bytes(B, N, int(max_iters))) + 15) // 16), 2, dtype=torch.float64, device=dev)
    out = {
        "F": torch.empty(B, 3, 3, device=dev),
        "mask": torch.empty(B, N, device=dev, dtype=torch.uint8),
        "n_inliers": torch.empty(B, device=dev, dtype=torch.int32),
        "iters_run": torch.empty(B, device=dev, dtype=torch.int32),
        "best_hyp": torch.empty(B, 2, device=dev, dtype=torch.int32),
        "hyp_counts": torch.empty(B, int(max_iters), 3, device=dev, dtype=torch.int32) if want_hyp_counts else None,
        "masked": torch.empty(B, N, 4, device=dev) if want_masked else None,
    }
    with _on(dev):
        rc = L.dfepe_ransac_fundamental(_ptr(m), B, N, float(threshold), float(confidence), int(max_iters), int(seed) & ((1 << 64) - 1),
                                        _ptr(ws), _ptr(out["F"]), _ptr(out["mask"]), _ptr(out["n_inliers"]), _ptr(out["iters_run"]),
                                        _ptr(out["best_hyp"]), _ptr(out["hyp_counts"]), _ptr(out["masked"]), _stream())
    _lib.check(rc, "dfepe_ransac_fundamental")
    return out


def ransac_in_front(E: Tensor, K: Tensor, matches: Tensor, winner: Tensor, depth_thres: float = 50.0) -> Tensor:
    """[B,N] uint8: the correspondences the winning candidate of cheirality(E, K, matches, depth_thres) sees in front of both
    cameras (cv2.recoverPose's mask output); a row sums to that call's counts[winner]."""
    E, K, m = _prep(E, "E"), _prep(K, "K"), _prep(matches, "matches")
    _shape(m, "matches (pixel x1,y1,x2,y2)", None, None, 4)
    B, N = m.shape[0], m.shape[1]
    _shape(E, "E", B, 3, 3)
    _shape(K, "K (one intrinsic matrix per pair)", B, 3, 3)
    if winner.shape != (B,) or winner.dtype != torch.int32 or not winner.is_contiguous():
        raise ValueError("winner must be the contiguous [B] int32 output of cheirality")
    mask = torch.empty(B, N, device=m.device, dtype=torch.uint8)
    with _on(m.device):
        rc = _lib.lib().dfepe_ransac_in_front(_ptr(E), _ptr(K), _ptr(m), B, N, float(depth_thres), _ptr(winner), _ptr(mask), _stream())
    _lib.check(rc, "dfepe_ransac_in_front")
    return mask


def ransac_pose(matches: Tensor, K: Tensor, threshold: float = 0.1, confidence: float = 0.99, max_iters: int = 1000, seed: int = 0,
                depth_thres: float = 50.0, K_pose: Optional[Tensor] = None):
    """The 8-point baseline of utils_opencv.recover_camera_opencv (utils_opencv.py:157-177) for every pair: ransac_fundamental,
    E = K^T F K projected onto singular values (1, 1, 0), then cv2.recoverPose(E, x1, x2, camera K_pose, mask=inliers): the
    unchanged cheirality kernel on the matches with the non-inlier rows set to NaN (a NaN row passes no depth test).
    K_pose: the camera recoverPose is given (default K; the reference passes focal K[0,0] and principal point (K[0,2], K[1,2])).
    Returns the ransac_fundamental dict with E [B,3,3], Rt_cam [B,3,4], winner [B], counts [B,4] and in_front [B,N] uint8 added."""
    K = _prep(K, "K")
    out = ransac_fundamental(matches, threshold, confidence, max_iters, seed, want_masked=True)
    B = out["F"].shape[0]
    _shape(K, "K (one intrinsic matrix per pair)", B, 3, 3)
    Kp = K if K_pose is None else _prep(K_pose, "K_pose")
    E = project_essential(congruence(out["F"], K))
    Rt, win, cnt = cheirality(E, Kp, out["masked"], depth_thres)
    out.update({"E": E, "Rt_cam": Rt, "winner": win, "counts": cnt, "in_front": ransac_in_front(E, Kp, out["masked"], win, depth_thres)})
    return out


def ransac_essential(matches: Tensor, K: Tensor, threshold: float = 1.0, confidence: float = 0.999, max_iters: int = 1000, seed: int = 0,
                     want_hyp_counts: bool = False, want_hyp_E: bool = False, want_masked: bool = False):
    """matches [B,N,4] pixels, K [B,3,3] -> robust E of every pair by OpenCV 3.4's findEssentialMat(RANSAC) algorithm, the
    five-point baseline (utils_opencv.py:147-151; include/dfepe.h spells out the normalisation, the sampler, the five-point solve,
    the Sampson score and the stopping rule).  The defaults are cv2's own for findEssentialMat.
    Returns dict(E [B,3,3] (unit Frobenius norm, largest entry positive; zeros without a model), mask [B,N] uint8, n_inliers [B],
    iters_run [B], best_hyp [B,2] (iteration, root; -1 without a model), hyp_counts [B,max_iters,10] | None (-1: no root), hyp_E
    [B,max_iters,10,3,3] float64 | None (the hypotheses; unused slots zero), masked [B,N,4] | None (non-inlier rows NaN)).
    No host synchronisation.  6 <= N <= 4096."""
    m, K = _prep(matches, "matches"), _prep(K, "K")
    _shape(m, "matches (pixel x1,y1,x2,y2)", None, None, 4)
    B, N = m.shape[0], m.shape[1]
    _shape(K, "K (one intrinsic matrix per pair)", B, 3, 3)
    if N < _lib.RANSAC5_MIN_N:
        raise _lib.DfepeError(f"ransac_essential: {N} correspondences per pair; the five-point RANSAC estimator needs at least "
                              f"{_lib.RANSAC5_MIN_N}")
    L = _lib.lib()
    dev = m.device
    T = int(max_iters)
    ws = torch.empty(max(1, (int(L.dfepe_ransac5_workspace_bytes(B, N, T)) + 15) // 16), 2, dtype=torch.float64, device=dev)
    out = {
        "E": torch.empty(B, 3, 3, device=dev),
        "mask": torch.empty(B, N, device=dev, dtype=torch.uint8),
        "n_inliers": torch.empty(B, device=dev, dtype=torch.int32),
        "iters_run": torch.empty(B, device=dev, dtype=torch.int32),
        "best_hyp": torch.empty(B, 2, device=dev, dtype=torch.int32),
        "hyp_counts": torch.empty(B, T, 10, device=dev, dtype=torch.int32) if want_hyp_counts else None,
        "hyp_E": torch.empty(B, T, 10, 3, 3, device=dev, dtype=torch.float64) if want_hyp_E else None,
        "masked": torch.empty(B, N, 4, device=dev) if want_masked else None,
    }
    with _on(dev):
        rc = L.dfepe_ransac_essential(_ptr(m), _ptr(K), B, N, float(threshold), float(confidence), T, int(seed) & ((1 << 64) - 1),
                                      _ptr(ws), _ptr(out["E"]), _ptr(out["mask"]), _ptr(out["n_inliers"]), _ptr(out["iters_run"]),
                                      _ptr(out["best_hyp"]), _ptr(out["hyp_counts"]), _ptr(out["hyp_E"]), _ptr(out["masked"]), _stream())
    _lib.check(rc, "dfepe_ransac_essential")
    return out


def ransac_essential_pose(matches: Tensor, K: Tensor, threshold: float = 1.0, confidence: float = 0.999, max_iters: int = 1000,
                          seed: int = 0, depth_thres: float = 50.0):
    """The five-point baseline of utils_opencv.recover_camera_opencv(five_point=True) (utils_opencv.py:147-151,177) for every
    pair: ransac_essential with the camera recover_pose_camera(K) -- the reference gives findEssentialMat and recoverPose the same
    focal length and principal point -- then cv2.recoverPose(E, x1, x2, that camera, mask=inliers): E goes to the unchanged
    cheirality kernel as it is (no K^T F K, no projection), on the matches with the non-inlier rows set to NaN.
    Returns the ransac_essential dict with Rt_cam [B,3,4], winner [B], counts [B,4] and in_front [B,N] uint8 added."""
    K = _prep(K, "K")
    Kp = torch.zeros_like(K)  # compat.utils_opencv.recover_pose_camera: focal K00, principal point (K02, K12)
    Kp[:, 0, 0] = Kp[:, 1, 1] = K[:, 0, 0]
    Kp[:, 0, 2], Kp[:, 1, 2], Kp[:, 2, 2] = K[:, 0, 2], K[:, 1, 2], 1.0
    out = ransac_essential(matches, Kp, threshold, confidence, max_iters, seed, want_masked=True)
    Rt, win, cnt = cheirality(out["E"], Kp, out["masked"], depth_thres)
    out.update({"Rt_cam": Rt, "winner": win, "counts": cnt, "in_front": ransac_in_front(out["E"], Kp, out["masked"], win, depth_thres)})
    return out


def _lmeds(name: str, m: Tensor, K: Optional[Tensor], model_points: int, confidence: float, max_iters: int, seed: int,
           want_hyp_medians: bool, want_masked: bool):
    """The common body of lmeds_fundamental (K None, model_points 7) and lmeds_essential (model_points 5)."""
    B, N = m.shape[0], m.shape[1]
    L = _lib.lib()
    dev = m.device
    niters = int(L.dfepe_lmeds_num_iters(model_points, float(confidence), int(max_iters)))
    if niters < 0:
        _lib.check(niters, "dfepe_lmeds_num_iters")
    roots = 3 if model_points == 7 else 10
    ws = torch.empty(max(1, (int(L.dfepe_lmeds_workspace_bytes(B, model_points, float(confidence), int(max_iters))) + 15) // 16), 2,
                     dtype=torch.float64, device=dev)
    out = {
        name: torch.empty(B, 3, 3, device=dev),
        "mask": torch.empty(B, N, device=dev, dtype=torch.uint8),
        "n_inliers": torch.empty(B, device=dev, dtype=torch.int32),
        "iters_run": torch.empty(B, device=dev, dtype=torch.int32),
        "best_hyp": torch.empty(B, 2, device=dev, dtype=torch.int32),
        "min_median": torch.empty(B, device=dev, dtype=torch.float64),
        "sigma": torch.empty(B, device=dev, dtype=torch.float64),
        "hyp_medians": torch.empty(B, niters, roots, device=dev, dtype=torch.float64) if want_hyp_medians else None,
        "masked": torch.empty(B, N, 4, device=dev) if want_masked else None,
    }
    tail = (B, N, float(confidence), int(max_iters), int(seed) & ((1 << 64) - 1), _ptr(ws), _ptr(out[name]), _ptr(out["mask"]),
            _ptr(out["n_inliers"]), _ptr(out["iters_run"]), _ptr(out["best_hyp"]), _ptr(out["min_median"]), _ptr(out["sigma"]),
            _ptr(out["hyp_medians"]), _ptr(out["masked"]), _stream())
    with _on(dev):
        rc = L.dfepe_lmeds_fundamental(_ptr(m), *tail) if K is None else L.dfepe_lmeds_essential(_ptr(m), _ptr(K), *tail)
    _lib.check(rc, "dfepe_lmeds_fundamental" if K is None else "dfepe_lmeds_essential")
    return out


def lmeds_fundamental(matches: Tensor, confidence: float = 0.99, max_iters: int = 1000, seed: int = 0, want_hyp_medians: bool = False,
                      want_masked: bool = False):
    """matches [B,N,4] pixels -> least-median-of-squares F of every pair: OpenCV 3.4's LMedS, which cv2.findFundamentalMat(..,
    cv2.RANSAC, ..) runs instead of RANSAC below 15 correspondences (utils_opencv.py:157; include/dfepe.h spells out the six
    steps).  No threshold: the inlier bound comes from the winning median.
    Returns dict(F [B,3,3] (F22 = 1; zeros without a model), mask [B,N] uint8, n_inliers [B], iters_run [B], best_hyp [B,2]
    (iteration, root; -1 without a model), min_median [B] float64, sigma [B] float64, hyp_medians [B,niters,3] float64 | None
    (-1: no root, -2: no sample; niters = 300 for the default confidence), masked [B,N,4] | None (non-inlier rows NaN)).
    No host synchronisation.  8 <= N <= 4096."""
    m = _prep(matches, "matches")
    _shape(m, "matches (pixel x1,y1,x2,y2)", None, None, 4)
    if m.shape[1] < _lib.LMEDS_MIN_N:
        raise _lib.DfepeError(f"lmeds_fundamental: {m.shape[1]} correspondences per pair; the LMedS estimator needs at least "
                              f"{_lib.LMEDS_MIN_N} (with 7 OpenCV solves the one sample directly, which is not built)")
    return _lmeds("F", m, None, 7, confidence, max_iters, seed, want_hyp_medians, want_masked)


def lmeds_pose(matches: Tensor, K: Tensor, confidence: float = 0.99, max_iters: int = 1000, seed: int = 0, depth_thres: float = 50.0,
               K_pose: Optional[Tensor] = None):
    """ransac_pose with lmeds_fundamental in place of ransac_fundamental: what utils_opencv.recover_camera_opencv computes for a
    pair with fewer than 15 correspondences (utils_opencv.py:157-177).  Returns the lmeds_fundamental dict with E [B,3,3], Rt_cam
    [B,3,4], winner [B], counts [B,4] and in_front [B,N] uint8 added."""
    K = _prep(K, "K")
    out = lmeds_fundamental(matches, confidence, max_iters, seed, want_masked=True)
    B = out["F"].shape[0]
    _shape(K, "K (one intrinsic matrix per pair)", B, 3, 3)
    Kp = K if K_pose is None else _prep(K_pose, "K_pose")
    E = project_essential(congruence(out["F"], K))
    Rt, win, cnt = cheirality(E, Kp, out["masked"], depth_thres)
    out.update({"E": E, "Rt_cam": Rt, "winner": win, "counts": cnt, "in_front": ransac_in_front(E, Kp, out["masked"], win, depth_thres)})
    return out


def lmeds_essential(matches: Tensor, K: Tensor, confidence: float = 0.999, max_iters: int = 1000, seed: int = 0,
                    want_hyp_medians: bool = False, want_masked: bool = False):
    """matches [B,N,4] pixels, K [B,3,3] -> least-median-of-squares E of every pair by five-point models: OpenCV 3.4's
    findEssentialMat(method=LMEDS) (include/dfepe.h, dfepe_lmeds_essential).  Returns the dict of lmeds_fundamental with E [B,3,3]
    (unit Frobenius norm; zeros without a model) in place of F and hyp_medians [B,niters,10].  No host synchronisation.
    6 <= N <= 4096."""
    m, K = _prep(matches, "matches"), _prep(K, "K")
    _shape(m, "matches (pixel x1,y1,x2,y2)", None, None, 4)
    _shape(K, "K (one intrinsic matrix per pair)", m.shape[0], 3, 3)
    if m.shape[1] < _lib.LMEDS5_MIN_N:
        raise _lib.DfepeError(f"lmeds_essential: {m.shape[1]} correspondences per pair; the five-point LMedS estimator needs at least "
                              f"{_lib.LMEDS5_MIN_N}")
    return _lmeds("E", m, K, 5, confidence, max_iters, seed, want_hyp_medians, want_masked)


def lmeds_essential_pose(matches: Tensor, K: Tensor, confidence: float = 0.999, max_iters: int = 1000, seed: int = 0,
                         depth_thres: float = 50.0):
    """ransac_essential_pose with lmeds_essential in place of ransac_essential (the same camera recover_pose_camera(K) for the
    estimate and for the pose).  Returns the lmeds_essential dict with Rt_cam [B,3,4], winner [B], counts [B,4] and in_front [B,N]
    uint8 added."""
    K = _prep(K, "K")
    Kp = torch.zeros_like(K)  # compat.utils_opencv.recover_pose_camera: focal K00, principal point (K02, K12)
    Kp[:, 0, 0] = Kp[:, 1, 1] = K[:, 0, 0]
    Kp[:, 0, 2], Kp[:, 1, 2], Kp[:, 2, 2] = K[:, 0, 2], K[:, 1, 2], 1.0
    out = lmeds_essential(matches, Kp, confidence, max_iters, seed, want_masked=True)
    Rt, win, cnt = cheirality(out["E"], Kp, out["masked"], depth_thres)
    out.update({"Rt_cam": Rt, "winner": win, "counts": cnt, "in_front": ransac_in_front(out["E"], Kp, out["masked"], win, depth_thres)})
    return out


def correct_matches(F: Tensor, pts1: Tensor, pts2: Tensor, want_cost: bool = False):
    """The optimal correction of correspondences onto an epipolar geometry (Hartley & Sturm), cv2.correctMatches(F, pts1, pts2)
    for a batch: new1, new2 [B,M,2] float32 with new2^T F new1 = 0 and |pts1 - new1|^2 + |pts2 - new2|^2 minimal; with want_cost
    also that minimum [B,M] in px^2.  F [B,3,3], or [3,3] for all pairs, of any float dtype: it is converted to float64, which the
    kernel reads (include/dfepe.h says why).  pts1, pts2 [B,M,2] pixels on the GPU.  A point on an epipole gives NaN, as in cv2.
    One launch, no host synchronisation, no autograd: these are ground-truth data."""
    p, q = _prep(pts1.detach(), "pts1"), _prep(pts2.detach(), "pts2")
    _shape(p, "pts1 (pixel x, y)", None, None, 2)
    B, M = p.shape[0], p.shape[1]
    _shape(q, "pts2", B, M, 2)
    if not F.is_cuda:
        raise _lib.DfepeError("F must live on the GPU (this package has no CPU path)")
    Fd = F.detach().to(torch.float64).contiguous()
    if Fd.dim() == 2:
        _shape(Fd, "F", 3, 3)
    else:
        _shape(Fd, "F", B, 3, 3)
    dev = p.device
    new1, new2 = torch.empty(B, M, 2, device=dev), torch.empty(B, M, 2, device=dev)
    cost = torch.empty(B, M, device=dev) if want_cost else None
    with _on(dev):
        rc = _lib.lib().dfepe_correct_matches(_stream(), _ptr(Fd), 0 if Fd.dim() == 2 else 9, _ptr(p), _ptr(q), B, M, _ptr(new1),
                                              _ptr(new2), _ptr(cost))
    _lib.check(rc, "dfepe_correct_matches")
    return (new1, new2, cost) if want_cost else (new1, new2)


# ------------------------------------------------------------------------------------------------
# two-view structure: triangulation, depths, reprojection (csrc/triangulate.hip)
# ------------------------------------------------------------------------------------------------
def _per_pair(t: Tensor, name: str, B: int, *row) -> int:
    """t is [*row] (one matrix for all pairs: stride 0) or [B, *row]; returns the stride in floats."""
    if t.dim() == len(row):
        _shape(t, name, *row)
        return 0
    _shape(t, name, B, *row)
    n = 1
    for d in row:
        n *= d
    return n


def triangulate(P1: Tensor, P2: Tensor, matches: Tensor) -> Tensor:
    """cv2.triangulatePoints for a batch: P1, P2 [3,4] or [B,3,4] projection matrices, matches [B,N,4] pixels (x1, y1, x2, y2)
    -> Xh [B,N,4] float32, per correspondence the unit null vector of the DLT matrix with w = Xh[..., 3] >= 0 (include/dfepe.h:
    fp64 arithmetic, one rounding; a non-finite row gives NaNs).  One launch, no host synchronisation, no autograd."""
    m = _prep(matches.detach(), "matches")
    _shape(m, "matches (pixel x1,y1,x2,y2)", None, None, 4)
    B, N = m.shape[0], m.shape[1]
    P1, P2 = _prep(P1.detach(), "P1"), _prep(P2.detach(), "P2")
    s1, s2 = _per_pair(P1, "P1", B, 3, 4), _per_pair(P2, "P2", B, 3, 4)
    Xh = torch.empty(B, N, 4, device=m.device)
    with _on(m.device):
        rc = _lib.lib().dfepe_triangulate(_ptr(P1), s1, _ptr(P2), s2, _ptr(m), B, N, _ptr(Xh), _stream())
    _lib.check(rc, "dfepe_triangulate")
    return Xh


def two_view_structure(Rt: Tensor, K: Tensor, matches: Tensor, camera_motion: bool = True, winner: Optional[Tensor] = None,
                       scale: Optional[Tensor] = None, clamp: Optional[float] = None, want=("X", "z1", "z2")) -> dict:
    """The 3-D points of a pose's correspondences and their depths in both cameras (the reference's get_depth after
    cv2.recoverPose): Rt [B,3,4] (camera motion as cheirality() returns it, or scene motion with camera_motion=False), K [B,3,3],
    matches [B,N,4] pixels -> dict of the entries named in ``want``: X [B,N,3] in the frame of camera 1, z1, z2 [B,N].
    ``winner`` [B] int32 (cheirality's): a pair with winner < 0 gets NaN rows.  ``scale`` [B] multiplies X, z1 and z2
    (t_scene_scale); ``clamp`` > 0 clamps the scaled depths to [-clamp, clamp].  One launch, no host synchronisation."""
    m = _prep(matches.detach(), "matches")
    _shape(m, "matches (pixel x1,y1,x2,y2)", None, None, 4)
    B, N = m.shape[0], m.shape[1]
    Rt, K = _prep(Rt.detach(), "Rt"), _prep(K.detach(), "K")
    _shape(Rt, "Rt", B, 3, 4)
    _shape(K, "K (one intrinsic matrix per pair)", B, 3, 3)
    want = tuple(want)
    if not want or any(w not in ("X", "z1", "z2") for w in want):
        raise ValueError(f"want must name at least one of X, z1, z2, got {want}")
    if winner is not None and (winner.shape != (B,) or winner.dtype != torch.int32 or not winner.is_contiguous() or not winner.is_cuda):
        raise ValueError("winner must be the contiguous [B] int32 output of cheirality")
    if scale is not None:
        scale = _prep(scale.detach(), "scale").reshape(-1)
        _shape(scale, "scale", B)
    dev = m.device
    out = {k: torch.empty((B, N, 3) if k == "X" else (B, N), device=dev) for k in want}
    with _on(dev):
        rc = _lib.lib().dfepe_two_view_structure(_ptr(Rt), _lib.POSE_CAMERA_MOTION if camera_motion else 0, _ptr(K), _ptr(m), B, N,
                                                 _ptr(winner), _ptr(scale), float(clamp) if clamp else 0.0, _ptr(out.get("X")),
                                                 _ptr(out.get("z1")), _ptr(out.get("z2")), _stream())
    _lib.check(rc, "dfepe_two_view_structure")
    return out


def reproject(X: Tensor, Rt: Tensor, K: Tensor, image_w: float, image_h: float, camera_motion: bool = False) -> dict:
    """Project points into an image (utils_vis.reproj_and_scatter without the drawing): X [B,M,3], Rt [3,4] or [B,3,4] (scene
    motion, or camera motion with camera_motion=True), K [3,3] or [B,3,3] -> dict(x [B,M,2] pixels, z [B,M] depth, inside [B,M]
    uint8 = utils_misc.within(x, y, image_w, image_h) of the float32 x; no depth test).  One launch, no host synchronisation."""
    X = _prep(X.detach(), "X")
    _shape(X, "X", None, None, 3)
    B, M = X.shape[0], X.shape[1]
    Rt, K = _prep(Rt.detach(), "Rt"), _prep(K.detach(), "K")
    sr, sk = _per_pair(Rt, "Rt", B, 3, 4), _per_pair(K, "K", B, 3, 3)
    dev = X.device
    out = {"x": torch.empty(B, M, 2, device=dev), "z": torch.empty(B, M, device=dev), "inside": torch.empty(B, M, device=dev, dtype=torch.uint8)}
    with _on(dev):
        rc = _lib.lib().dfepe_reproject(_ptr(X), _ptr(Rt), sr, _lib.POSE_CAMERA_MOTION if camera_motion else 0, _ptr(K), sk, B, M,
                                        float(image_w), float(image_h), _ptr(out["x"]), _ptr(out["z"]), _ptr(out["inside"]), _stream())
    _lib.check(rc, "dfepe_reproject")
    return out


# ------------------------------------------------------------------------------------------------
# odometry evaluation: pose chain and snippet ATE / RE (deepFEPE/utils/eval_tools.py:252-375)
# ------------------------------------------------------------------------------------------------
def _pose12(t: Tensor, name: str, lead: int) -> Tensor:
    """[..., 3, 4] or [..., 12] with `lead` leading dimensions -> contiguous float64 [..., 12] on the GPU."""
    if not t.is_cuda:
        raise _lib.DfepeError(f"{name} must live on the GPU (this package has no CPU path)")
    t = t.detach().to(torch.float64)
    if t.dim() == lead + 2:
        if tuple(t.shape[-2:]) != (3, 4):
            raise ValueError(f"{name}: poses are 3x4 (or 12 numbers, row-major), got {tuple(t.shape)}")
        t = t.reshape(*t.shape[:-2], 12)
    if t.dim() != lead + 1 or t.shape[-1] != 12:
        raise ValueError(f"{name}: expected {lead} leading dimension(s) and 3x4 poses, got {tuple(t.shape)}")
    return t.contiguous()


def _lengths_arg(lengths, S: int, hi: int, dev, name: str):
    """lengths as a device int32 [S] -- and, when they are host values, checked against [0, hi] here (a device tensor cannot be
    checked without a synchronisation: its range is the caller's contract, and the kernels clamp it to their buffers)."""
    if lengths is None:
        return None
    if isinstance(lengths, Tensor) and lengths.is_cuda:
        _shape(lengths, name, S)
        return lengths.to(torch.int32).contiguous()
    host = [int(v) for v in (lengths.tolist() if isinstance(lengths, Tensor) else lengths)]
    if len(host) != S or any(v < 0 or v > hi for v in host):
        raise ValueError(f"{name} must be {S} values in [0, {hi}], got {host}")
    return torch.tensor(host, dtype=torch.int32, device=dev)


def pose_chain(rel: Tensor, lengths=None, cam2body: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """Relative poses -> trajectory, Exp_table_processor.get_abs_poses for a batch of sequences: rel [S,n,3,4] (or [S,n,12])
    -> abs [S,n+1,3,4] float64 with abs[s,0] the identity and abs[s,k] = inv(P_k ... P_1) (general inverse).  cam2body
    [S,3,4] (one per sequence) or [S,n,3,4] (one per pose): P_k is first taken to body coordinates, inv(C) P_k C
    (relative_pose_cam_to_body).  lengths [S] (host values or a device tensor) for a padded batch: entries past lengths[s]
    are not written (they keep what `out` held; without `out` they are zero).  One launch, no host synchronisation."""
    r = _pose12(rel, "rel", 2)
    S, n = r.shape[0], r.shape[1]
    dev = r.device
    c, stride = None, 0
    if cam2body is not None:
        if cam2body.dim() == 2 or (cam2body.dim() == 3 and cam2body.shape[-1] == 4):  # [S,12] or [S,3,4]: one per sequence
            c = _pose12(cam2body, "cam2body", 1)
            _shape(c, "cam2body", S, 12)
        else:
            c, stride = _pose12(cam2body, "cam2body", 2), 12
            _shape(c, "cam2body", S, n, 12)
    ln = _lengths_arg(lengths, S, n, dev, "lengths")
    if out is None:
        out = torch.zeros(S, n + 1, 12, device=dev, dtype=torch.float64) if ln is not None else \
            torch.empty(S, n + 1, 12, device=dev, dtype=torch.float64)
    elif out.dtype != torch.float64 or not out.is_contiguous() or out.numel() != S * (n + 1) * 12 or out.device != dev:
        raise ValueError("out must be a contiguous float64 tensor of S (n + 1) 12 elements on rel's device")
    with _on(dev):
        rc = _lib.lib().dfepe_pose_chain(_stream(), _ptr(r), _ptr(ln), _ptr(c), stride, S, n, _ptr(out))
    _lib.check(rc, "dfepe_pose_chain")
    return out.view(S, n + 1, 3, 4)


def snippet_errors(est: Tensor, gt: Tensor, seq_length: int = 5, windows=None, compensate: bool = True,
                   want_compensated: bool = False, capacity: Optional[int] = None) -> dict:
    """The snippet ATE / RE of Exp_table_processor.pose_seq_ate for a batch of trajectories: est, gt [S,m,3,4] (or [S,m,12])
    absolute poses; window w of a sequence covers poses w .. w + seq_length - 1.  windows [S] (host values, checked here, or a
    device tensor, the caller's contract: windows[s] + seq_length - 1 <= the sequence's number of poses): how many windows each
    sequence has; default m - seq_length, the reference's count (it never scores the last window).  capacity: rows in the
    outputs (default: the largest host value of windows, or m - seq_length + 1 for a device tensor).
    compensate=False scores the poses as given (a stand-alone compute_pose_error).
    -> dict: errors [S,W,2] float32 (ATE, RE), scale_factors [S,W] float64, aligned_poses [S,W,3,4] float64, stats [S,4] float64
    (ATE mean, ATE std, RE mean, RE std; NaN without windows), with want_compensated also compensated [S,W,L,3,4] (the
    estimate's snippets after compensate_poses).  Rows past windows[s] are zero.  One launch, no host synchronisation."""
    L = int(seq_length)
    if not 1 <= L <= _lib.SNIPPET_MAX_L:
        raise _lib.DfepeError(f"seq_length must be in [1, {_lib.SNIPPET_MAX_L}], got {L}")
    e, g = _pose12(est, "est", 2), _pose12(gt, "gt", 2)
    S, m = e.shape[0], e.shape[1]
    _shape(g, "gt", S, m, 12)
    dev = e.device
    most = max(m - L + 1, 0)
    if windows is None:
        windows = [max(m - L, 0)] * S
    wn = _lengths_arg(windows, S, most, dev, "windows")
    if capacity is None:
        capacity = most if isinstance(windows, Tensor) and windows.is_cuda else max([int(v) for v in windows], default=0)
    W = int(capacity)
    errors = torch.zeros(S, W, 2, device=dev, dtype=torch.float32)
    scale = torch.zeros(S, W, device=dev, dtype=torch.float64)
    aligned = torch.zeros(S, W, 12, device=dev, dtype=torch.float64)
    comp = torch.zeros(S, W, L, 12, device=dev, dtype=torch.float64) if want_compensated else None
    stats = torch.empty(S, 4, device=dev, dtype=torch.float64)
    with _on(dev):
        rc = _lib.lib().dfepe_snippet_errors(_stream(), _ptr(e), _ptr(g), _ptr(wn), S, m, W, L, 0 if compensate else 1,
                                             _ptr(errors), _ptr(scale), _ptr(aligned), _ptr(comp), _ptr(stats))
    _lib.check(rc, "dfepe_snippet_errors")
    out = {"errors": errors, "scale_factors": scale, "aligned_poses": aligned.view(S, W, 3, 4), "stats": stats}
    if want_compensated:
        out["compensated"] = comp.view(S, W, L, 3, 4)
    return out


# ------------------------------------------------------------------------------------------------
# KITTI odometry table: alignment, segment errors, ATE, RPE (the KITTI devkit / kitti-odom-eval evaluation)
# ------------------------------------------------------------------------------------------------
def _traj_args(est: Tensor, gt: Tensor, est_lengths, gt_lengths):
    e, g = _pose12(est, "est", 2), _pose12(gt, "gt", 2)
    S, n = g.shape[0], g.shape[1]
    if e.shape[0] != S or e.shape[1] > n:
        raise ValueError(f"est must have gt's batch and at most its frames, got {tuple(e.shape)} against {tuple(g.shape)}")
    dev = g.device
    m = e.shape[1]
    if m < n:  # the kernels take one n_max: the estimate is padded and its length says so
        e = torch.cat([e, torch.zeros(S, n - m, 12, device=dev, dtype=torch.float64)], dim=1)
        if est_lengths is None:
            est_lengths = torch.full((S,), m, dtype=torch.int32, device=dev)
    return e, g, S, n, _lengths_arg(est_lengths, S, m, dev, "est_lengths"), _lengths_arg(gt_lengths, S, n, dev, "gt_lengths")


def trajectory_align(est: Tensor, gt: Tensor, mode: str = "scale_7dof", est_lengths=None, gt_lengths=None) -> dict:
    """Steps 1 and 2 of the KITTI odometry evaluation for a batch of sequences: est [S,m,3,4], gt [S,n,3,4] (or [..,12]) absolute
    poses, m <= n, frame i of one corresponding to frame i of the other; est_lengths, gt_lengths [S] (host values, checked here,
    or device tensors, clamped by the kernel) for padded batches.  Both trajectories are re-based on their first pose; mode is
    one of _lib.TRAJ_MODES: "none", "scale" (least-squares scale of the translations), "scale_7dof" (Umeyama's scale only),
    "7dof", "6dof" (Umeyama's similarity / rigid transform applied to every pose).
    -> dict: est [S,n,3,4] (aligned; zero past a sequence's m), gt [S,n,3,4] (re-based; zero past its n), r [S,3,3], t [S,3],
    c [S] float64.  One launch, no host synchronisation."""
    if mode not in _lib.TRAJ_MODES:
        raise ValueError(f"mode must be one of {_lib.TRAJ_MODES}, got {mode!r}")
    e, g, S, n, el, gl = _traj_args(est, gt, est_lengths, gt_lengths)
    dev = g.device
    eo = torch.zeros(S, n, 12, device=dev, dtype=torch.float64)
    go = torch.zeros(S, n, 12, device=dev, dtype=torch.float64)
    rtc = torch.empty(S, 13, device=dev, dtype=torch.float64)
    with _on(dev):
        rc = _lib.lib().dfepe_trajectory_align(_stream(), _ptr(e), _ptr(g), _ptr(el), _ptr(gl), S, n, _lib.TRAJ_MODES.index(mode),
                                               _ptr(eo), _ptr(go), _ptr(rtc))
    _lib.check(rc, "dfepe_trajectory_align")
    return {"est": eo.view(S, n, 3, 4), "gt": go.view(S, n, 3, 4), "r": rtc[:, :9].reshape(S, 3, 3), "t": rtc[:, 9:12], "c": rtc[:, 12]}


def kitti_odometry_errors(est: Tensor, gt: Tensor, step: int = 10, est_lengths=None, gt_lengths=None) -> dict:
    """Steps 3 to 5 of the KITTI odometry evaluation on aligned trajectories (trajectory_align's est and gt): est [S,m,3,4],
    gt [S,n,3,4], lengths as there (trajectory_align returns a shorter estimate padded to n frames: its length goes in est_lengths
    here, as compat.eval_tools does).  For every first frame 0, step, 2 step, ... and every length 100 .. 800 m the segment's
    rotation and translation error per metre, then the whole-trajectory ATE and the RPE.
    -> dict: rows [S,F,8,5] float64 with F = ceil(n / step): [first, r_err, t_err, len, speed] (zero where not valid), valid
    [S,F,8] bool, count [S] int32, summary [S,5] float64: t_rel (%), r_rel (deg / 100 m), ATE (m), RPE (m), RPE (deg), and dist
    [S,n] float64, the ground truth's path length.  One launch, no host synchronisation."""
    step = int(step)
    if step < 1:
        raise ValueError(f"step must be at least 1, got {step}")
    e, g, S, n, el, gl = _traj_args(est, gt, est_lengths, gt_lengths)
    dev = g.device
    F = (n + step - 1) // step
    dist = torch.zeros(S, n, device=dev, dtype=torch.float64)
    rows = torch.zeros(S, F, 8, 5, device=dev, dtype=torch.float64)
    valid = torch.zeros(S, F, 8, device=dev, dtype=torch.uint8)
    count = torch.empty(S, device=dev, dtype=torch.int32)
    summary = torch.empty(S, 5, device=dev, dtype=torch.float64)
    with _on(dev):
        rc = _lib.lib().dfepe_kitti_odometry_errors(_stream(), _ptr(e), _ptr(g), _ptr(el), _ptr(gl), S, n, step, F, _ptr(dist),
                                                    _ptr(rows), _ptr(valid), _ptr(count), _ptr(summary))
    _lib.check(rc, "dfepe_kitti_odometry_errors")
    return {"rows": rows, "valid": valid.view(torch.bool), "count": count, "summary": summary, "dist": dist}


# ------------------------------------------------------------------------------------------------
# validation summary reductions ("next" row f-2)
# ------------------------------------------------------------------------------------------------
METRIC_THS = (0.0, 0.01, 0.03, 0.05, 0.1, 0.3, 0.5, 1.0, 2.0, 5.0, 10.0, 90.0, 180.0)


def metrics_summary(epi_est: Tensor, epi_gt: Optional[Tensor], err_q: Tensor, err_t: Tensor) -> dict:
    """Device-side reductions of write_metrics_summary (train_good_utils.py:758-856) for one experiment tag: epi_est / epi_gt
    = epipolar distances of every correspondence (any shape, same numel), err_q / err_t [B] pose errors in degrees.
    Two launches and ONE device-to-host copy of 288 bytes.  Returns python floats: ratio_0.1, ratio_1, F1_0.1, F1_1 (None
    without epi_gt), median / max of err_q and err_t, and ratio_q / ratio_t = cumulative fractions below METRIC_THS[1:].
    The median is np.median of the errors widened to float64: the float64 mean of the two middle float32 order statistics, not
    rounded back to float32.  The maximum is np.amax for any vector with an entry >= 0 or NaN (NaN wins, -0.0 never does).  Empty
    inputs give zeros.  tests/metrics_ref.py restates all of it; tests/test_metrics_edges_gpu.py compares exactly."""
    import numpy as np

    e = _prep(epi_est.reshape(-1), "epi_est")
    g = None if epi_gt is None else _prep(epi_gt.reshape(-1), "epi_gt")
    q, t = _prep(err_q.reshape(-1), "err_q"), _prep(err_t.reshape(-1), "err_t")
    if g is not None and g.numel() != e.numel():
        raise ValueError("epi_gt must have as many entries as epi_est")
    if q.numel() != t.numel():
        raise ValueError("err_q and err_t must have the same length")
    L = _lib.lib()
    nbytes = int(L.dfepe_metrics_summary_bytes())
    out = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=e.device)
    with _on(e.device):
        rc = L.dfepe_metrics_summary(_ptr(e) if e.numel() else None, _ptr(g), e.numel(), _ptr(q), _ptr(t), q.numel(), _ptr(out), _stream())
    _lib.check(rc, "dfepe_metrics_summary")
    raw = out.cpu().numpy().tobytes()[:nbytes]
    counts = np.frombuffer(raw, dtype=np.uint64, count=8).astype(np.float64)
    hist = np.frombuffer(raw, dtype=np.uint64, count=24, offset=64).astype(np.float64).reshape(2, 12)
    mx = np.frombuffer(raw, dtype=np.float32, count=2, offset=64 + 192)
    mids = np.frombuffer(raw, dtype=np.float32, count=4, offset=64 + 192 + 8).reshape(2, 2)
    n, B = max(e.numel(), 1), max(q.numel(), 1)

    def f1(tp, fp, fn):
        return float(2 * tp / (2 * tp + fp + fn)) if (2 * tp + fp + fn) > 0 else 0.0

    res = {"ratio_0.1": float(counts[0] / n), "ratio_1": float(counts[1] / n),
           "F1_0.1": f1(*counts[2:5]) if g is not None else None, "F1_1": f1(*counts[5:8]) if g is not None else None,
           "median_err_q": float(0.5 * (float(mids[0, 0]) + float(mids[0, 1]))), "median_err_t": float(0.5 * (float(mids[1, 0]) + float(mids[1, 1]))),
           "max_err_q": float(mx[0]), "max_err_t": float(mx[1]),
           "ratio_q": (np.cumsum(hist[0]) / B).tolist(), "ratio_t": (np.cumsum(hist[1]) / B).tolist()}
    return res


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


def _n_valid_arg(n_valid, B: int, dev, name: str) -> Optional[Tensor]:
    if n_valid is None:
        return None
    if not torch.is_tensor(n_valid) or not n_valid.is_cuda:
        raise _lib.DfepeError(f"{name}: n_valid must be an int32 [B] tensor on the GPU (the counts stay on the device)")
    if n_valid.shape != (B,):
        raise ValueError(f"{name}: n_valid must have shape [{B}], got {tuple(n_valid.shape)}")
    return n_valid.to(device=dev, dtype=torch.int32).contiguous()


def _h9(H: Tensor, name: str, B: int) -> Tensor:
    if not H.is_cuda:
        raise _lib.DfepeError(f"{name} must live on the GPU (this package has no CPU path)")
    if H.shape not in ((B, 3, 3), (B, 9)):
        raise ValueError(f"{name} must have shape [{B},3,3], got {tuple(H.shape)}")
    return H.to(torch.float64).contiguous()


def ransac_homography(matches: Tensor, n_valid: Optional[Tensor] = None, threshold: float = 3.0, confidence: float = 0.995,
                      max_iters: int = 2000, seed: int = 0, refine: bool = True, all_points: bool = False,
                      want_hyp_counts: bool = False, want_model: bool = False) -> dict:
    """matches [B,N,4] pixels (x1, y1, x2, y2) -> robust homography of every pair by OpenCV 3.4's findHomography(RANSAC) algorithm
    (descriptor_evaluation.py:93, evaluate_frontend.py:234; include/dfepe.h spells out the sampler, the 4-point solve, the error,
    the stopping rule, the refit over the inliers and the Levenberg-Marquardt refinement).  n_valid [B] int32 on the device or
    None: pair b uses its first n_valid[b] rows.  all_points: cv2's method = 0 (least squares over all points, mask all ones);
    refine=False leaves out the refinement.  Returns dict(H [B,3,3] float64 (H22 = 1; zeros without a model), mask [B,N] uint8,
    n_inliers [B], iters_run [B], best_iter [B] (-1 without a sampled winner), hyp_counts [B,max_iters] | None (-1: no model,
    -2: no sample), H_model [B,3,3] float64 | None (the winning sample's H before the refit)).  No host synchronisation;
    capturable.  1 <= N <= 4096."""
    m = _prep(matches, "matches")
    _shape(m, "matches (pixel x1,y1,x2,y2)", None, None, 4)
    B, N = m.shape[0], m.shape[1]
    if N < 1 or N > _lib.HOMOGRAPHY_MAX_N:
        raise _lib.DfepeError(f"ransac_homography: {N} correspondences per pair; the estimator takes 1 .. {_lib.HOMOGRAPHY_MAX_N}")
    L = _lib.lib()
    dev = m.device
    nv = _n_valid_arg(n_valid, B, dev, "ransac_homography")
    flags = (_lib.HOMOGRAPHY_ALL_POINTS if all_points else 0) | (0 if refine else _lib.HOMOGRAPHY_NO_REFINE)
    ws = torch.empty(max(1, (int(L.dfepe_homography_workspace_bytes(B, N, int(max_iters))) + 15) // 16), 2, dtype=torch.float64, device=dev)
    out = {
        "H": torch.empty(B, 3, 3, device=dev, dtype=torch.float64),
        "mask": torch.empty(B, N, device=dev, dtype=torch.uint8),
        "n_inliers": torch.empty(B, device=dev, dtype=torch.int32),
        "iters_run": torch.empty(B, device=dev, dtype=torch.int32),
        "best_iter": torch.empty(B, device=dev, dtype=torch.int32),
        "hyp_counts": torch.empty(B, int(max_iters), device=dev, dtype=torch.int32) if want_hyp_counts else None,
        "H_model": torch.empty(B, 3, 3, device=dev, dtype=torch.float64) if want_model else None,
    }
    with _on(dev):
        rc = L.dfepe_ransac_homography(_ptr(m), _ptr(nv), B, N, float(threshold), float(confidence), int(max_iters), int(seed) & ((1 << 64) - 1),
                                       flags, _ptr(ws), _ptr(out["H"]), _ptr(out["H_model"]), _ptr(out["mask"]), _ptr(out["n_inliers"]),
                                       _ptr(out["iters_run"]), _ptr(out["best_iter"]), _ptr(out["hyp_counts"]), _stream())
    _lib.check(rc, "dfepe_ransac_homography")
    return out


def homography_transfer(H: Tensor, matches: Tensor, n_valid: Optional[Tensor] = None, epi: float = 3.0):
    """H [B,3,3], matches [B,N,4] -> (dist [B,N] fp32 = |H x1 - x2|, mask [B,N] uint8 = dist < epi): evaluate_frontend.getInliers
    (evaluate_frontend.py:210-228) for B pairs, evaluated in fp64.  Rows past n_valid get 0 and 0.  No host synchronisation."""
    m = _prep(matches, "matches")
    _shape(m, "matches (pixel x1,y1,x2,y2)", None, None, 4)
    B, N = m.shape[0], m.shape[1]
    Hd = _h9(H, "H", B)
    dev = m.device
    nv = _n_valid_arg(n_valid, B, dev, "homography_transfer")
    dist = torch.empty(B, N, device=dev)
    mask = torch.empty(B, N, device=dev, dtype=torch.uint8)
    with _on(dev):
        rc = _lib.lib().dfepe_homography_transfer(_ptr(Hd), _ptr(m), _ptr(nv), B, N, float(epi), _ptr(dist), _ptr(mask), _stream())
    _lib.check(rc, "dfepe_homography_transfer")
    return dist, mask


def homography_corners(H_est: Tensor, H_gt: Tensor, height: int, width: int, thresh: Tensor):
    """H_est, H_gt [B,3,3]; thresh [T] on the device -> (mean_dist [B] float64, correct [B,T] uint8): the mean distance of the
    four image corners warped by both homographies and `mean_dist <= thresh` (descriptor_evaluation.compute_homography, lines
    104-123).  An all-zero H_est (no model) gives NaN and 0.  No host synchronisation."""
    if not H_est.is_cuda:
        raise _lib.DfepeError("H_est must live on the GPU (this package has no CPU path)")
    B = H_est.shape[0]
    He, Hg = _h9(H_est, "H_est", B), _h9(H_gt, "H_gt", B)
    dev = He.device
    if not torch.is_tensor(thresh) or not thresh.is_cuda or thresh.dim() != 1:
        raise _lib.DfepeError("homography_corners: thresh must be a 1-D tensor on the GPU")
    th = thresh.to(torch.float64).contiguous()
    T = th.shape[0]
    md = torch.empty(B, device=dev, dtype=torch.float64)
    ok = torch.empty(B, T, device=dev, dtype=torch.uint8)
    with _on(dev):
        rc = _lib.lib().dfepe_homography_corners(_ptr(He), _ptr(Hg), B, int(height), int(width), _ptr(th), T, _ptr(md), _ptr(ok), _stream())
    _lib.check(rc, "dfepe_homography_corners")
    return md, ok


# ------------------------------------------------------------------------------------------------
# front-end detector evaluation: repeatability, localization error, matching score, nn mean AP
# ------------------------------------------------------------------------------------------------
def _f64(t: Tensor, name: str) -> Tensor:
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _lib.DfepeError(f"{name} must live on the GPU (this package has no CPU path)")
    return t.to(torch.float64).contiguous()  # float32 -> float64 is exact


def keypoint_repeatability(kp1: Tensor, kp2: Tensor, H: Tensor, height: int, width: int, keep_k: int, thresh: Tensor,
                           n1: Optional[Tensor] = None, n2: Optional[Tensor] = None) -> dict:
    """kp1 [B,N1,C], kp2 [B,N2,C] rows (x, y[, prob]) of image 1 and image 2, C in {2, 3}; H [B,3,3] image 1 -> image 2; thresh [T]
    on the device -> compute_repeatability (evaluations/detector_evaluation.py:150-279) of every pair at every threshold, in fp64
    (float32 inputs are upcast, which is exact).  n1, n2 [B] int32 on the device or None: pair b uses its first n[b] rows.
    Returns dict(repeatability, loc_err [B,T] float64 (0 and -1 where nothing is counted), count1, count2 [B,T] int32, kept1, kept2
    [B] int32 (the set sizes after the filter and select_k_best), n_unwarped [B] int32 (the matching score's count of image-2
    points whose inverse warp lies in the image, both ends inclusive)).  Equal probabilities at the k-th place: the higher index
    is kept; keep_k = 0 keeps every point (numpy's [-0:]).  The inputs are not written to.  No host synchronisation.
    N1, N2 <= 4096."""
    a, b = _f64(kp1, "kp1"), _f64(kp2, "kp2")
    if a.dim() != 3 or b.dim() != 3 or a.shape[0] != b.shape[0] or a.shape[2] != b.shape[2] or a.shape[2] not in (2, 3):
        raise ValueError(f"keypoints must be [B,N1,C] and [B,N2,C] with C in (2, 3), got {tuple(a.shape)} and {tuple(b.shape)}")
    B, N1, C = a.shape
    N2 = b.shape[1]
    if max(N1, N2) > _lib.DETECTOR_EVAL_MAX_N:
        raise _lib.DfepeError(f"keypoint_repeatability: {max(N1, N2)} keypoints per image; at most {_lib.DETECTOR_EVAL_MAX_N}")
    if int(keep_k) < 0 or int(height) < 1 or int(width) < 1:
        raise ValueError("keypoint_repeatability: keep_k must be >= 0, height and width >= 1")
    Hd = _h9(H, "H", B)
    dev = a.device
    if not torch.is_tensor(thresh) or not thresh.is_cuda or thresh.dim() != 1:
        raise _lib.DfepeError("keypoint_repeatability: thresh must be a 1-D tensor on the GPU")
    th = thresh.to(torch.float64).contiguous()
    T = th.shape[0]
    c1, c2 = _n_valid_arg(n1, B, dev, "keypoint_repeatability"), _n_valid_arg(n2, B, dev, "keypoint_repeatability")
    L = _lib.lib()
    ws = torch.empty(max(1, (int(L.dfepe_keypoint_repeatability_workspace_bytes(B, N1, N2)) + 15) // 16), 2, dtype=torch.float64, device=dev)
    out = {
        "repeatability": torch.empty(B, T, device=dev, dtype=torch.float64),
        "loc_err": torch.empty(B, T, device=dev, dtype=torch.float64),
        "count1": torch.empty(B, T, device=dev, dtype=torch.int32),
        "count2": torch.empty(B, T, device=dev, dtype=torch.int32),
        "kept1": torch.empty(B, device=dev, dtype=torch.int32),
        "kept2": torch.empty(B, device=dev, dtype=torch.int32),
        "n_unwarped": torch.empty(B, device=dev, dtype=torch.int32),
    }
    with _on(dev):
        rc = L.dfepe_keypoint_repeatability(_ptr(a), _ptr(b), _ptr(c1), _ptr(c2), _ptr(Hd), B, N1, N2, C, int(height), int(width), int(keep_k),
                                            _ptr(th), T, _ptr(ws), _ptr(out["repeatability"]), _ptr(out["loc_err"]), _ptr(out["count1"]),
                                            _ptr(out["count2"]), _ptr(out["kept1"]), _ptr(out["kept2"]), _ptr(out["n_unwarped"]), _stream())
    _lib.check(rc, "dfepe_keypoint_repeatability")
    return out


def average_precision(labels: Tensor, scores: Tensor, n_valid: Optional[Tensor] = None, want_counts: bool = False) -> dict:
    """labels [B,M] (non-zero: positive), scores [B,M] -> sklearn.metrics.average_precision_score of every pair
    (evaluate_frontend.py:244-275) as AP = (1/P) sum over positives of TP(s_i) / CNT(s_i), which groups tied scores as scikit-learn
    does and needs no sort.  n_valid [B] int32 on the device or None.  Returns dict(ap [B] float64 (0 without a valid entry or a
    positive), n_pos [B] int32, tp_at, cnt_at [B,M] int32 | None (want_counts; 0 past n_valid)).  No host synchronisation.
    M <= 4096."""
    sc = _f64(scores, "scores")
    if not torch.is_tensor(labels) or not labels.is_cuda:
        raise _lib.DfepeError("labels must live on the GPU (this package has no CPU path)")
    if sc.dim() != 2 or labels.shape != sc.shape:
        raise ValueError(f"labels and scores must both be [B,M], got {tuple(labels.shape)} and {tuple(sc.shape)}")
    B, M = sc.shape
    if M > _lib.DETECTOR_EVAL_MAX_N:
        raise _lib.DfepeError(f"average_precision: {M} entries per pair; at most {_lib.DETECTOR_EVAL_MAX_N}")
    lb = (labels != 0).to(torch.uint8).contiguous()
    dev = sc.device
    nv = _n_valid_arg(n_valid, B, dev, "average_precision")
    out = {
        "ap": torch.empty(B, device=dev, dtype=torch.float64),
        "n_pos": torch.empty(B, device=dev, dtype=torch.int32),
        "tp_at": torch.empty(B, M, device=dev, dtype=torch.int32) if want_counts else None,
        "cnt_at": torch.empty(B, M, device=dev, dtype=torch.int32) if want_counts else None,
    }
    with _on(dev):
        rc = _lib.lib().dfepe_average_precision(_ptr(lb), _ptr(sc), _ptr(nv), B, M, _ptr(out["ap"]), _ptr(out["n_pos"]), _ptr(out["tp_at"]),
                                                _ptr(out["cnt_at"]), _stream())
    _lib.check(rc, "dfepe_average_precision")
    return out


def matching_score(n_inliers: Tensor, n_kp1: Tensor, n_unwarped: Tensor) -> Tensor:
    """n_inliers, n_kp1, n_unwarped [B] integer tensors on the device -> mscore [B] float64 = 2 n_inliers / (n_kp1 + n_unwarped)
    (evaluate_frontend.py:181); a zero denominator gives what the division gives.  No host synchronisation."""
    args = []
    for t, name in ((n_inliers, "n_inliers"), (n_kp1, "n_kp1"), (n_unwarped, "n_unwarped")):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise _lib.DfepeError(f"{name} must live on the GPU (this package has no CPU path)")
        if t.dim() != 1 or t.shape != n_inliers.shape or t.dtype.is_floating_point:
            raise ValueError(f"{name} must be an integer tensor of shape [{n_inliers.shape[0]}], got {t.dtype} {tuple(t.shape)}")
        args.append(t.to(torch.int32).contiguous())
    B = args[0].shape[0]
    dev = args[0].device
    out = torch.empty(B, device=dev, dtype=torch.float64)
    with _on(dev):
        rc = _lib.lib().dfepe_matching_score(_ptr(args[0]), _ptr(args[1]), _ptr(args[2]), B, _ptr(out), _stream())
    _lib.check(rc, "dfepe_matching_score")
    return out


# ------------------------------------------------------------------------------------------------
# SuperPoint output processing (process_SP_output, train_good_utils.py:727-755): heatmap, NMS, soft-argmax, descriptors
# ------------------------------------------------------------------------------------------------
def _sp_pixels(H: int, W: int, what: str) -> None:
    if H * W > _lib.SP_MAX_PIXELS:
        raise _lib.DfepeError(f"{what}: {H}x{W} pixels per image; at most {_lib.SP_MAX_PIXELS}")


def _sp_bytes(n: int, dev) -> Tensor:
    """n bytes of 16-byte aligned device memory (at least one cell)."""
    return torch.empty(max(1, (int(n) + 15) // 16), 2, dtype=torch.float64, device=dev)


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
    ws = _sp_bytes(L.dfepe_sp_nms_workspace_bytes(B, H, W), dev)
    with _on(dev):
        rc = L.dfepe_sp_nms(_ptr(h), B, H, W, float(conf_thresh), d, r, _ptr(ws), _ptr(out["nms_map"]), _ptr(out["pts"]), _ptr(out["conf"]),
                            _ptr(out["count"]), _stream())
    _lib.check(rc, "dfepe_sp_nms")
    return out


def _sp_list(pts: Tensor, count: Tensor, B: int, what: str):
    if not torch.is_tensor(pts) or not pts.is_cuda or not torch.is_tensor(count) or not count.is_cuda:
        raise _lib.DfepeError(f"{what}: pts and count must live on the GPU (this package has no CPU path)")
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
        ws = _sp_bytes(L.dfepe_sp_soft_argmax_bwd_workspace_bytes(B, H, W, cap), dev)
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


# ------------------------------------------------------------------------------------------------
# correspondence evaluation (evaluation_epiDist.py val_feature, eval_tools.Result_processor): inlier ratios by match score
# ------------------------------------------------------------------------------------------------
INLIER_TABLE_OUTPUTS = ("cnt", "num", "ratio", "dist_out")


def _thds_arg(thds, dev, name: str) -> Tensor:
    """A threshold list as a float64 [T] device tensor: a device tensor is taken as it is; host values are uploaded (inside a
    graph capture pass a device tensor)."""
    if torch.is_tensor(thds):
        if not thds.is_cuda:
            raise _lib.DfepeError(f"{name} must live on the GPU when it is a tensor (this package has no CPU path)")
        t = thds.to(device=dev, dtype=torch.float64).contiguous()
    else:
        t = torch.tensor([float(v) for v in thds], dtype=torch.float64).to(dev)
    if t.dim() != 1 or not 1 <= t.shape[0] <= _lib.INLIER_TABLE_MAX_THDS:
        raise ValueError(f"{name} must hold 1 .. {_lib.INLIER_TABLE_MAX_THDS} thresholds, got shape {tuple(t.shape)}")
    return t


def inlier_table(matches: Optional[Tensor] = None, F: Optional[Tensor] = None, scores: Optional[Tensor] = None,
                 n_valid: Optional[Tensor] = None, inlier_thds=(1.0,), mask_thds=None, want=("cnt", "num", "ratio"),
                 dist: Optional[Tensor] = None) -> dict:
    """matches [B,N,4] pixels (x1, y1, x2, y2) with F [B,3,3], or dist [B,N] (a distance computed before), exactly one of the two;
    scores [B,N] or None (no mask: every match is kept, and mask_thds must be None or hold one value); n_valid [B] int32 on the
    device or None: pair b uses its first clamp(n_valid[b], 0, N) rows; inlier_thds [Ti], mask_thds [Tm] (1 .. 16 each; device
    tensors, or host values that are uploaded) -> dict of the outputs named in ``want``:
      cnt [B,Tm,Ti] int32 = #{score < mask_thd and dist < inlier_thd}, num [B,Tm] int32 = #{score < mask_thd} (num_corrs),
      ratio [B,Tm,Ti] float64 = cnt / num (NaN for a pair with nothing kept), dist_out [B,N] float32 (0 past n_valid)
    Result_processor.inlier_ratio (deepFEPE/utils/eval_tools.py:70-104) over epi_distance_np's dist3 (dsac_tools/utils_F.py:363-385)
    for B pairs, Tm mask thresholds and Ti inlier thresholds in one launch; the distance and both strict comparisons are fp64.
    No host synchronisation; capturable."""
    if (matches is None) == (dist is None):
        raise ValueError("inlier_table takes matches (with F) or dist, exactly one of the two")
    want = tuple(want)
    if not want or any(w not in INLIER_TABLE_OUTPUTS for w in want):
        raise ValueError(f"want must name at least one of {INLIER_TABLE_OUTPUTS}, got {want}")
    if matches is not None:
        m = _prep(matches, "matches")
        _shape(m, "matches (pixel x1,y1,x2,y2)", None, None, 4)
        B, N = m.shape[0], m.shape[1]
        if F is None:
            raise ValueError("inlier_table: matches need F")
        Fd, d, dev = _h9(F, "F", B), None, m.device
    else:
        d = _prep(dist, "dist")
        _shape(d, "dist", None, None)
        B, N = d.shape
        m, Fd, dev = None, None, d.device
    sc = None
    if scores is not None:
        sc = _prep(scores, "scores")
        _shape(sc, "scores", B, N)
    elif mask_thds is not None and len(mask_thds) != 1:
        raise ValueError("inlier_table: without scores nothing is masked; mask_thds must be None or hold one value")
    nv = _n_valid_arg(n_valid, B, dev, "inlier_table")
    it = _thds_arg(inlier_thds, dev, "inlier_thds")
    mt = _thds_arg(mask_thds, dev, "mask_thds") if sc is not None and mask_thds is not None else None
    if sc is not None and mt is None:
        raise ValueError("inlier_table: scores need mask_thds")
    Ti, Tm = it.shape[0], (mt.shape[0] if mt is not None else 1)
    out = {
        "cnt": torch.empty(B, Tm, Ti, device=dev, dtype=torch.int32) if "cnt" in want else None,
        "num": torch.empty(B, Tm, device=dev, dtype=torch.int32) if "num" in want else None,
        "ratio": torch.empty(B, Tm, Ti, device=dev, dtype=torch.float64) if "ratio" in want else None,
        "dist_out": torch.empty(B, N, device=dev, dtype=torch.float32) if "dist_out" in want else None,
    }
    with _on(dev):
        rc = _lib.lib().dfepe_inlier_table(_ptr(m), _ptr(Fd), _ptr(d), _ptr(sc), _ptr(nv), B, N, _ptr(it), Ti, _ptr(mt), Tm, _ptr(out["cnt"]),
                                           _ptr(out["num"]), _ptr(out["ratio"]), _ptr(out["dist_out"]), _stream())
    _lib.check(rc, "dfepe_inlier_table")
    return {k: v for k, v in out.items() if v is not None}


def inlier_table_mean(ratio: Tensor, num: Tensor):
    """ratio [B,Tm,Ti] float64, num [B,Tm] int32 (inlier_table's) -> (mean [Tm,Ti] float64, num_T [Tm,B] int32): the table's mean
    over the pairs, added in index order and NaN-propagating as numpy's table.mean(axis=0) is (eval_tools.py:99-100), and the
    counts in the layout ap_inlier_thd returns.  B == 0 gives a NaN mean.  One launch, no host synchronisation; capturable."""
    for t, name in ((ratio, "ratio"), (num, "num")):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise _lib.DfepeError(f"{name} must live on the GPU (this package has no CPU path)")
    _shape(ratio, "ratio", None, None, None)
    B, Tm, Ti = ratio.shape
    _shape(num, "num", B, Tm)
    if not (1 <= Tm <= _lib.INLIER_TABLE_MAX_THDS and 1 <= Ti <= _lib.INLIER_TABLE_MAX_THDS):
        raise ValueError(f"ratio must be [B,Tm,Ti] with 1 .. {_lib.INLIER_TABLE_MAX_THDS} thresholds each, got {tuple(ratio.shape)}")
    r = ratio.to(torch.float64).contiguous()
    n = num.to(torch.int32).contiguous()
    dev = r.device
    mean = torch.empty(Tm, Ti, device=dev, dtype=torch.float64)
    num_T = torch.empty(Tm, B, device=dev, dtype=torch.int32)
    with _on(dev):
        rc = _lib.lib().dfepe_inlier_table_mean(_ptr(r), _ptr(n), B, Tm, Ti, _ptr(mean), _ptr(num_T), _stream())
    _lib.check(rc, "dfepe_inlier_table_mean")
    return mean, num_T


# ------------------------------------------------------------------------------------------------
# DSAC: the hypothesis loop of dsac_tools/dsac.py, batched over pairs and hypotheses
# ------------------------------------------------------------------------------------------------
DSAC_LOSS_KINDS = {None: 0, "none": 0, "hloss": 1, "hloss_F": 2}


_DSAC_OUT = ("E_sample", "soft", "sampson", "score", "E_refit", "loss", "quality", "counts", "best", "exp_loss", "top_loss")
_DSAC_DIFF = ("E_sample", "score", "E_refit", "loss", "quality", "exp_loss")  # what dfepe_dsac_bwd takes an upstream gradient for


def _dsac_launch(X, Y, K, idx, thresh, beta, alpha, kind, want) -> dict:
    """dfepe_dsac on prepared tensors -> every output by name, None where ``want`` does not name it."""
    B, N = X.shape[0], X.shape[1]
    H, S = idx.shape[1], idx.shape[2]
    dev = X.device
    L = _lib.lib()

    def f32(*shape, name=None):
        return torch.empty(*shape, device=dev, dtype=torch.float32) if name is None or name in want else None

    out = {"E_sample": f32(B, H, 3, 3), "soft": f32(B, H, N, name="soft"), "sampson": f32(B, H, N, name="sampson"), "score": f32(B, H),
           "E_refit": f32(B, H, 3, 3), "loss": f32(B, H), "quality": f32(B, N), "counts": f32(B, N),
           "best": torch.empty(B, device=dev, dtype=torch.int32), "exp_loss": f32(B, name="exp_loss"), "top_loss": f32(B, name="top_loss")}
    if B == 0:
        return out
    ws = torch.empty(L.dfepe_dsac_workspace_bytes(B, N, H, S) // 4, device=dev, dtype=torch.float32)
    with _on(dev):
        rc = L.dfepe_dsac(_stream(), _ptr(X), _ptr(Y), _ptr(K), _ptr(idx), B, N, H, S, float(thresh), float(beta),
                          float(alpha), kind, _ptr(out["E_sample"]), _ptr(out["soft"]), _ptr(out["sampson"]), _ptr(out["score"]),
                          _ptr(out["E_refit"]), _ptr(out["loss"]), _ptr(out["quality"]), _ptr(out["counts"]), _ptr(out["best"]),
                          _ptr(out["exp_loss"]), _ptr(out["top_loss"]), _ptr(ws))
    _lib.check(rc, "dfepe_dsac")
    return out


def dsac_bwd(X: Tensor, Y: Tensor, K: Tensor, idx: Tensor, inlier_thresh: float, inlier_beta: float, inlier_alpha: float, kind: int,
             fwd: dict, grads: dict, want_x: bool = True, want_y: bool = True, totals: bool = False):
    """dfepe_dsac_bwd on prepared tensors: ``fwd`` holds the forward's E_sample, soft, score, E_refit, loss and counts as written,
    ``grads`` the upstream gradients by output name (E_sample, score, E_refit, loss, quality, exp_loss; missing or None = 0, not all).
    Returns (g_X, g_Y) [B,N,2] (None where not asked for), and with ``totals`` a third item: the dict of the stage totals t_score,
    t_loss [B,H], t_E_refit, t_E_sample [B,H,3,3], t_w [H,B,N] (include/dfepe.h)."""
    B, N = X.shape[0], X.shape[1]
    H, S = idx.shape[1], idx.shape[2]
    dev = X.device
    L = _lib.lib()
    g = {k: (None if grads.get(k) is None else grads[k].contiguous().float()) for k in _DSAC_DIFF}
    gX = torch.empty_like(X) if want_x else None
    gY = torch.empty_like(Y) if want_y else None
    t = {}
    if totals:
        t = {"t_score": torch.empty(B, H, device=dev), "t_loss": torch.empty(B, H, device=dev), "t_E_refit": torch.empty(B, H, 3, 3, device=dev),
             "t_w": torch.empty(H, B, N, device=dev), "t_E_sample": torch.empty(B, H, 3, 3, device=dev)}
    if B > 0:
        ws = torch.empty(L.dfepe_dsac_bwd_workspace_bytes(B, N, H, S) // 4, device=dev, dtype=torch.float32)
        with _on(dev):
            rc = L.dfepe_dsac_bwd(_stream(), _ptr(X), _ptr(Y), _ptr(K), _ptr(idx), B, N, H, S, float(inlier_thresh), float(inlier_beta),
                                  float(inlier_alpha), kind, _ptr(fwd["E_sample"]), _ptr(fwd["soft"]), _ptr(fwd["score"]),
                                  _ptr(fwd["E_refit"]), _ptr(fwd["loss"]), _ptr(fwd["counts"]), _ptr(g["E_sample"]), _ptr(g["score"]),
                                  _ptr(g["E_refit"]), _ptr(g["loss"]), _ptr(g["quality"]), _ptr(g["exp_loss"]), _ptr(gX), _ptr(gY),
                                  _ptr(t.get("t_score")), _ptr(t.get("t_loss")), _ptr(t.get("t_E_refit")), _ptr(t.get("t_w")),
                                  _ptr(t.get("t_E_sample")), _ptr(ws))
        _lib.check(rc, "dfepe_dsac_bwd")
    return (gX, gY, t) if totals else (gX, gY)


class _DsacFunction(torch.autograd.Function):
    """The loop with its adjoint (dfepe_dsac_bwd).  The forward keeps its inputs and the outputs the adjoint reads; `soft` and
    `exp_loss` are always computed, whatever the caller wants returned."""

    @staticmethod
    def forward(ctx, X, Y, K, idx, thresh, beta, alpha, kind, want):
        out = _dsac_launch(X, Y, K, idx, thresh, beta, alpha, kind, tuple(want) + ("soft", "exp_loss"))
        ctx.save_for_backward(X, Y, K, idx, out["E_sample"], out["soft"], out["score"], out["E_refit"], out["loss"], out["counts"])
        ctx.cfg = (thresh, beta, alpha, kind)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(*(out[k] for k in _DSAC_OUT if k not in _DSAC_DIFF and out[k] is not None))
        return tuple(out[k] for k in _DSAC_OUT)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *g_out):
        X, Y, K, idx, E_sample, soft, score, E_refit, loss, counts = ctx.saved_tensors
        grads = {k: g for k, g in zip(_DSAC_OUT, g_out) if k in _DSAC_DIFF and g is not None}
        need_x, need_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gX = gY = None
        if grads and (need_x or need_y) and X.shape[0] > 0:
            fwd = {"E_sample": E_sample, "soft": soft, "score": score, "E_refit": E_refit, "loss": loss, "counts": counts}
            gX, gY = dsac_bwd(X, Y, K, idx, *ctx.cfg, fwd, grads, want_x=need_x, want_y=need_y)
        return (gX, gY) + (None,) * 7


def dsac(X: Tensor, Y: Tensor, K: Tensor, idx: Tensor, inlier_thresh: float, inlier_beta: float, inlier_alpha: float = 0.0,
         loss_kind=0, want=("soft", "sampson", "exp_loss", "top_loss")) -> dict:
    """The DSAC loop of deepFEPE/dsac_tools/dsac.py (:138-176, :194) for B pairs and H hypotheses each in six launches:
    X, Y [B,N,2] pixel points, K [B,3,3], idx [B,H,S] int32 on the device (8 <= S <= 16, N >= S; distinct within a hypothesis and
    0 <= idx < N: a contract) -> dict with E_sample [B,H,3,3], score [B,H], E_refit [B,H,3,3], loss [B,H], quality [B,N], counts
    [B,N], best [B] int32 and, as named in ``want``, soft [B,H,N], sampson [B,H,N], exp_loss [B], top_loss [B].
    ``loss_kind``: 0 / "none", 1 / "hloss" (HLoss(E_refit, X, Y) as the reference calls it), 2 / "hloss_F" (under K^-T E_refit K^-1).
    include/dfepe.h (dfepe_dsac) has the contract.  No host synchronisation and no allocation inside the call; capturable.
    Differentiable w.r.t. X and Y (dfepe_dsac_bwd, once): E_sample, score, E_refit, loss, quality and exp_loss carry the graph, the
    other outputs do not.  K is a constant of the adjoint: a K that requires grad raises NotImplementedError.  With nothing
    requiring grad it is the forward launch alone."""
    if torch.is_grad_enabled() and torch.is_tensor(K) and K.requires_grad:
        raise NotImplementedError("dsac: the gradient to K is not built (dfepe_dsac_bwd differentiates w.r.t. X and Y only); detach K")
    X, Y, K = _prep(X, "X"), _prep(Y, "Y"), _prep(K, "K")
    if not torch.is_tensor(idx) or not idx.is_cuda:
        raise _lib.DfepeError("idx must live on the GPU (this package has no CPU path)")
    _shape(X, "X", None, None, 2)
    B, N = X.shape[0], X.shape[1]
    _shape(Y, "Y", B, N, 2)
    _shape(K, "K", B, 3, 3)
    _shape(idx, "idx", B, None, None)
    H, S = idx.shape[1], idx.shape[2]
    if not _lib.DSAC_MIN_SAMPLE <= S <= _lib.DSAC_MAX_SAMPLE or N < S or H < 1:
        raise ValueError(f"dsac: idx [B,H,S] needs H >= 1 and {_lib.DSAC_MIN_SAMPLE} <= S <= {_lib.DSAC_MAX_SAMPLE} <= N, got H={H}, S={S}, N={N}")
    kind = DSAC_LOSS_KINDS.get(loss_kind, loss_kind) if isinstance(loss_kind, (str, type(None))) else int(loss_kind)
    if kind not in (0, 1, 2):
        raise ValueError(f"dsac: loss_kind must be 0, 1, 2 or one of {[k for k in DSAC_LOSS_KINDS if k]}, got {loss_kind!r}")
    want = tuple(want)
    if any(w not in ("soft", "sampson", "exp_loss", "top_loss") for w in want):
        raise ValueError(f"dsac: want names soft, sampson, exp_loss, top_loss; got {want}")
    idx = idx.to(torch.int32).contiguous()
    if torch.is_grad_enabled() and (X.requires_grad or Y.requires_grad):
        # the adjoint reads the points as 8-byte pairs: a contiguous view that starts at an odd element of its buffer is copied
        X, Y = (t.clone() if t.data_ptr() % 8 else t for t in (X, Y))
        vals = _DsacFunction.apply(X, Y, K, idx, float(inlier_thresh), float(inlier_beta), float(inlier_alpha), kind, want)
        out = dict(zip(_DSAC_OUT, vals))
        return {k: v for k, v in out.items() if v is not None and (k not in ("soft", "exp_loss") or k in want)}
    out = _dsac_launch(X, Y, K, idx, inlier_thresh, inlier_beta, inlier_alpha, kind, want)
    return {k: v for k, v in out.items() if v is not None}
