"""The DSAC hypothesis loop and its adjoint (csrc/dsac.hip, dsac_adjoint.hip).  Not named dsac.py: the package exports the function
dsac, and a submodule of that name would be hidden behind it."""
from __future__ import annotations

import torch

from .. import _lib
from ._base import Tensor, _on, _on_gpu, _prep, _ptr, _shape, _stream


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
    _on_gpu(idx, "idx")
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
