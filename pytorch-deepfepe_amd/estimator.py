"""The per-correspondence weight estimator on the matrix cores: host side.

``estimator_forward(x, layers, head)`` evaluates the Conv1d(k=1) -> InstanceNorm1d(affine) -> LeakyReLU stack of
ErrorEstimator (deepFEPE/models/ErrorEstimators.py:47-64) with the kernels of csrc/est_*.hip (est_gemm: the products, est_norm: normalisation, adjoints and head, est_planes: plane making
and reductions, est_pass: one pass per call; est_common.h: what they share): every fp32 operand travels as
16-bit planes.  Forward (round 5): two fp16 planes per operand (a = a0 + a1 to 22 bits), three MFMAs per product with fp32
accumulation -- fp32-class accuracy at half the matrix work of the six bf16 products of rounds 3-4; each layer's weights are split
scaled by a power of two found on the device (dfepe_est_absmax) so that their low plane stays out of fp16's subnormal range.
Backward: two bf16 planes, three MFMAs (gradients keep bf16's range, no loss scaling) -- a forward that will be differentiated
also leaves each activation as two bf16 planes, one that will not (torch.no_grad(), nothing requires grad) skips them.
InstanceNorm + LeakyReLU + the split into planes are the forward GEMM's epilogue for N = 100 points per pair, and a kernel of
their own behind the plain product for any other N (the SIFT configurations' 1000-2000).  One autograd node for the whole stack;
parameters and inputs are the module's own fp32 tensors.  PyTorch is plumbing here (allocation, the tiny weight transposes, the
sums over split-K / per-pair partials)."""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from .ops import _on, _ptr, _stream

Tensor = torch.Tensor
BF16 = torch.bfloat16
F16 = torch.float16

import os as _os

_DEBUG_ZERO = set(filter(None, _os.environ.get("DFEPE_EST_DEBUG_ZERO", "").split(",")))


def _buf(name, *shape, **kw):
    """torch.empty, or torch.zeros for the buffers named in DFEPE_EST_DEBUG_ZERO (diagnostics: hunting reads of unwritten memory)."""
    return (torch.zeros if (name in _DEBUG_ZERO or "all" in _DEBUG_ZERO) else torch.empty)(*shape, **kw)


def supported(x: Tensor) -> bool:
    """Any [B, C, N] on the GPU with B >= 1, N >= 2 (N = dfepe_est_points() takes the fused epilogue, see _fused; a single point
    per pair is left to the stock stack, whose InstanceNorm1d raises on it like the reference's)."""
    return x.is_cuda and x.dim() == 3 and x.shape[0] > 0 and x.shape[2] > 1 and x.shape[0] * x.shape[2] < 2 ** 31


def _fused(N: int) -> bool:
    return N == _lib.lib().dfepe_est_points()


def _pad32(c: int) -> int:
    return (c + 31) // 32 * 32


def _split(src: Tensor, rows: int, c_src: int, c: int, n_planes: int) -> Tensor:
    """fp32 [rows, c_src] (contiguous) -> bf16 planes [n_planes, rows, c], channels past c_src zero."""
    out = _buf("split", n_planes, rows, c, device=src.device, dtype=BF16)
    rc = _lib.lib().dfepe_est_split(_ptr(src), rows, c_src, c_src, c, n_planes, _ptr(out), rows * c, _stream())
    _lib.check(rc, "dfepe_est_split")
    return out


def _split_f16(src: Tensor, rows: int, c_src: int, c: int, absmax: Optional[Tensor] = None) -> Tensor:
    """fp32 [rows, c_src] (contiguous) -> two fp16 planes [2, rows, c], scaled by the power of two of `absmax` (weights) if given."""
    out = _buf("split", 2, rows, c, device=src.device, dtype=F16)
    rc = _lib.lib().dfepe_est_split_f16(_ptr(src), rows, c_src, c_src, c, _ptr(absmax), _ptr(out), rows * c, _stream())
    _lib.check(rc, "dfepe_est_split_f16")
    return out


def _ptr_array(ts):
    return (ctypes.c_void_p * len(ts))(*[_ptr(t) for t in ts])


def _int_array(vs):
    return (ctypes.c_int * len(vs))(*vs)


_TAB = 8    # layers per dfepe_est_wprep launch pair
_SEG = 40   # segments per dfepe_est_colsum launch (kSegMax)


def _wprep(Ws: Sequence[Tensor], want_wt: Sequence[bool], dev) -> Tuple[List[Tensor], List[Optional[Tensor]], Tensor]:
    """Every hidden layer's weights [Co, Ci] (fp32, contiguous) in two launches (per eight layers): the device-side power-of-two
    scales, the scaled fp16 planes [2, Co, K] the forward multiplies by, and -- where wanted -- the bf16 planes of W^T [2, K, Co]
    the data gradient multiplies by (the weights a backward sees are the ones its forward saw: autograd's version check)."""
    n = len(Ws)
    words = torch.empty(max(n, 1), device=dev, dtype=torch.int32)
    Co, Ci = [int(W.shape[0]) for W in Ws], [int(W.shape[1]) for W in Ws]
    pf = [_buf("split", 2, Co[l], _pad32(Ci[l]), device=dev, dtype=F16) for l in range(n)]
    pt = [(_buf("split", 2, _pad32(Ci[l]), Co[l], device=dev, dtype=BF16) if want_wt[l] else None) for l in range(n)]
    ws = torch.empty(max(1, _lib.lib().dfepe_est_wprep_workspace_bytes(min(n, _TAB)) // 4), device=dev, dtype=torch.int32)
    for a in range(0, n, _TAB):
        b = min(n, a + _TAB)
        rc = _lib.lib().dfepe_est_wprep(b - a, _ptr_array(Ws[a:b]), _int_array(Co[a:b]), _int_array(Ci[a:b]), _ptr_array(pf[a:b]),
                                        _ptr_array(pt[a:b]), _ptr(words[a:b]), _ptr(ws), _stream())
        _lib.check(rc, "dfepe_est_wprep")
    return pf, pt, words


def _dgamma_zero(fixes, slope: float, N: int, B: int) -> None:
    """fixes: per layer (dA, dlogit, w_head, dY_next, dyn_plane, W_next, C_next, out_planes, out_plane, in_planes, in_plane, W32, Ci,
    rstd, gamma, C, dgamma_part).  One layer: dfepe_est_dgamma_zero; several: dfepe_est_dgamma_zero_multi, one launch."""
    lib = _lib.lib()
    if len(fixes) == 1:
        dA, dlg, wh, dYn, dynp, Wn, Cn, outp, outs, inp, ins, W32, Ci, rstd, g32, C, dg = fixes[0]
        rc = lib.dfepe_est_dgamma_zero(_ptr(dA), _ptr(dlg), _ptr(wh), _ptr(outp), outs, _ptr(inp), ins, _ptr(W32), Ci, Ci, _ptr(rstd), _ptr(g32),
                                       float(slope), C, N, B, _ptr(dg), _ptr(dYn), dynp, _ptr(Wn), C, Cn, _stream())
        _lib.check(rc, "dfepe_est_dgamma_zero")
        return
    col = lambda i: [f[i] for f in fixes]
    sizes = lambda i: (ctypes.c_size_t * len(fixes))(*col(i))
    rc = lib.dfepe_est_dgamma_zero_multi(len(fixes), _ptr_array(col(0)), _ptr_array(col(1)), _ptr_array(col(2)), _ptr_array(col(7)), sizes(8),
                                         _ptr_array(col(9)), sizes(10), _ptr_array(col(11)), _int_array(col(12)), _ptr_array(col(13)),
                                         _ptr_array(col(14)), _int_array(col(15)), _ptr_array(col(16)), _ptr_array(col(3)), sizes(4),
                                         _ptr_array(col(5)), _int_array(col(6)), float(slope), N, B, _stream())
    _lib.check(rc, "dfepe_est_dgamma_zero_multi")


def _colsum(segs: List[Tuple[Optional[Tensor], int, int]], dev) -> List[Tensor]:
    """[(src [rows, cols] or None, rows, cols)] -> the column sums, one launch per 32 segments (rows = 0: zeros), fixed order."""
    outs = [torch.empty(c, device=dev, dtype=torch.float32) for _, _, c in segs]
    for a in range(0, len(segs), _SEG):
        b = min(len(segs), a + _SEG)
        rc = _lib.lib().dfepe_est_colsum(b - a, _ptr_array([t for t, _, _ in segs[a:b]]), _int_array([r for _, r, _ in segs[a:b]]),
                                         _int_array([c for _, _, c in segs[a:b]]), _ptr_array(outs[a:b]), _stream())
        _lib.check(rc, "dfepe_est_colsum")
    return outs


def _row_splits(pairs: int, c: int, n: int) -> int:
    """Workgroups a pair's rows are spread over in the N-generic normalisation kernels: 1 when (pair, 64-channel) workgroups
    alone fill the chip, otherwise enough to reach ~1024 workgroups with at least 128 rows (one unrolled trip) each."""
    blocks = pairs * ((c + 63) // 64)
    if blocks >= 512 or n < 256:
        return 1
    return max(1, min(64, n // 128, (1024 + blocks - 1) // blocks))


FUSE_DGRAD = _os.environ.get("DFEPE_EST_FUSE_DGRAD", "1") != "0"  # A/B switch: the data gradient fused with the adjoint below it

USE_PASS = _os.environ.get("DFEPE_EST_PASS", "1") != "0"  # one library call per estimator pass (0: the per-launch host code)

FIX_AT_END_BYTES = int(_os.environ.get("DFEPE_EST_FIX_AT_END_BYTES", 64 << 20))  # a backward whose dY planes together stay below this keeps them for one gamma == 0 launch at its end

TN_BLOCKS = 768  # workgroups of a weight-gradient launch: three per CU in one residency round (130 registers, 32 KB of LDS each);
# measured: 1024 (the kernel compiled for four per CU, 128 registers) 10.67 against 10.55 ms per estimator call


def _slices_for(cout: int, cin: int, cols: int = 1 << 30) -> int:
    tiles = ((cout + 127) // 128) * ((cin + 127) // 128)
    s = max(1, min(512, TN_BLOCKS // tiles, cols // 256))  # at the reference's batch sizes a slice keeps >= 256 columns (8 K steps)
    return s - s % 8 if s >= 8 else s  # a multiple of eight: one slice group per XCD (est_gemm_tn's block order needs it)


class _EstimatorFunction(torch.autograd.Function):
    """args: x [B, C0, N], then per hidden layer (conv weight [Co,Ci,1], conv bias [Co], gamma [Co], beta [Co]), then the head's
    (weight [O,C,1], bias [O] or None; O = 1 for the weight heads, 4 for update_offsets); cfg = (n_hidden, eps, slope, keep)."""

    @staticmethod
    def forward(ctx, cfg, x, *params):
        n_hidden, eps, slope, keep = cfg
        lib = _lib.lib()
        B, C0, N = x.shape
        cols = B * N
        dev = x.device
        with _on(dev):
            st = _stream()  # the current stream of x's device, read under its guard
            xin = x.detach().float().permute(0, 2, 1).reshape(cols, C0).contiguous()
            # keep: a backward may come (estimator_forward: grad mode on and something requires grad); without one the bf16 planes
            # the backward reads are neither computed nor stored
            act = _split_f16(xin, cols, C0, _pad32(C0))  # the layer's input as the forward reads it: two fp16 planes [2, cols, C]
            acts = [_split(xin, cols, C0, _pad32(C0), 2)] if keep else []  # ... and as the backward reads it: two bf16 planes
            rstds = []
            W32s = [params[4 * l].detach().float().reshape(params[4 * l].shape[0], params[4 * l].shape[1]).contiguous() for l in range(n_hidden)]
            # all layers' weights in two launches: scales, fp16 planes, and the transposed bf16 planes of every layer whose data
            # gradient the backward will form (all but the first, unless the input wants a gradient)
            Wps, WTps, wmax = _wprep(W32s, [keep and (l > 0 or ctx.needs_input_grad[1]) for l in range(n_hidden)], dev)
            for l in range(n_hidden):
                W, _b, gamma, beta = params[4 * l:4 * l + 4]
                Co, Ci = W.shape[0], W.shape[1]
                K = act.shape[2]
                Wp = Wps[l]
                out = _buf("out", 2, cols, Co, device=dev, dtype=F16)
                out_b = _buf("out_b", 2, cols, Co, device=dev, dtype=BF16) if keep else None
                rstd = _buf("rstd", B, Co, device=dev, dtype=torch.float32)
                g32, b32 = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
                if _fused(N):
                    rc = lib.dfepe_est_layer_fwd(_ptr(Wp), Co * K, _ptr(act), cols * K, Co, cols, K, _ptr(wmax[l:l + 1]), _ptr(g32), _ptr(b32),
                                                 float(eps), float(slope), _ptr(out), cols * Co, _ptr(out_b), cols * Co, _ptr(rstd), st)
                    _lib.check(rc, "dfepe_est_layer_fwd")
                else:  # the plain product (three fp16 products, fp32 out), then the statistics over each pair's N columns
                    Y = _buf("Y", cols, Co, device=dev, dtype=torch.float32)
                    rc = lib.dfepe_est_gemm_nt_f16(_ptr(Wp), Co * K, _ptr(act), cols * K, Co, cols, K, _ptr(wmax[l:l + 1]), _ptr(Y), Co, st)
                    _lib.check(rc, "dfepe_est_gemm_nt_f16")
                    sp = _row_splits(B, Co, N)
                    part = _buf("npart", B * sp * 2 * Co, device=dev, dtype=torch.float32) if sp > 1 else None
                    rc = lib.dfepe_est_norm_fwd(_ptr(Y), Co, Co, B, N, _ptr(g32), _ptr(b32), float(eps), float(slope), _ptr(out), cols * Co,
                                                _ptr(out_b), cols * Co, _ptr(rstd), sp, _ptr(part), st)
                    _lib.check(rc, "dfepe_est_norm_fwd")
                    del Y
                act = out  # the previous layer's fp16 planes are dropped here: only the bf16 pair lives on to the backward
                if keep:
                    acts.append(out_b)
                    rstds.append(rstd)
            Wh, bh = params[4 * n_hidden], params[4 * n_hidden + 1]
            C = act.shape[2]
            n_out = Wh.shape[0]  # 1: the weight heads; 4: update_offsets (if_learn_offsets, models/DeepFNet.py:330,342)
            wh = Wh.detach().float().reshape(n_out, C).contiguous()
            bh32 = None if bh is None else bh.detach().float().contiguous()
            logits = _buf("logits", n_out, cols, device=dev, dtype=torch.float32)
            for o in range(n_out):  # a GEMV per output channel over the same planes
                rc = lib.dfepe_est_head_fwd(_ptr(act), cols * C, C, cols, _ptr(wh[o]), _ptr(None if bh32 is None else bh32[o:o + 1]),
                                            _ptr(logits[o]), st)
                _lib.check(rc, "dfepe_est_head_fwd")
        ctx.cfg = cfg
        ctx.shape = (B, C0, N)
        # the bf16 planes and the reciprocal deviations travel through save_for_backward like the parameters: autograd owns their
        # lifetime (freed after the backward of a graph that is not retained, kept under retain_graph=True, and a second backward
        # through a freed graph raises autograd's own error instead of a TypeError on a cleared attribute)
        kept = [p for p in params if p is not None]
        ctx.n_params = len(kept)
        wts = [t for t in WTps if t is not None] if keep else []
        ctx.wt_layers = [l for l in range(n_hidden) if keep and WTps[l] is not None]
        ctx.save_for_backward(*kept, *acts, *rstds, *wts)
        ctx.has_head_bias = bh is not None
        return logits.view(B, 1, N) if n_out == 1 else logits.view(n_out, B, N).permute(1, 0, 2).contiguous()

    @staticmethod
    def backward(ctx, g_logits):
        n_hidden, eps, slope, _keep = ctx.cfg
        lib = _lib.lib()
        B, C0, N = ctx.shape
        cols = B * N
        everything = list(ctx.saved_tensors)
        saved = everything[:ctx.n_params]
        acts = everything[ctx.n_params:ctx.n_params + n_hidden + 1]
        rstds = everything[ctx.n_params + n_hidden + 1:ctx.n_params + 2 * n_hidden + 1]
        WTps = dict(zip(ctx.wt_layers, everything[ctx.n_params + 2 * n_hidden + 1:]))
        params = saved if ctx.has_head_bias else saved + [None]
        dev = g_logits.device
        grads: List[Optional[Tensor]] = [None] * len(params)
        with _on(dev):
            st = _stream()
            Wh = params[4 * n_hidden]
            C = acts[-1].shape[2]
            n_out = Wh.shape[0]
            dl = g_logits.detach().float().permute(1, 0, 2).reshape(n_out, cols).contiguous()  # [n_out, cols]
            wh = Wh.detach().float().reshape(n_out, C).contiguous()
            nblk = 512
            part = _buf("hpart", n_out, nblk, C, device=dev, dtype=torch.float32)
            for o in range(n_out):
                rc = lib.dfepe_est_head_dw(_ptr(acts[-1]), cols * C, C, cols, nblk, _ptr(dl[o]), _ptr(part[o]), None, st)
                _lib.check(rc, "dfepe_est_head_dw")
            # every reduction of this backward is a segment of ONE dfepe_est_colsum launch at the end: (source [rows, cols], rows, cols)
            # and what to do with the sum
            segs: List[Tuple[Optional[Tensor], int, int]] = [(part[o], nblk, C) for o in range(n_out)]
            sinks = [None] * n_out  # the head's: gathered below
            if ctx.has_head_bias:
                grads[4 * n_hidden + 1] = dl.sum(1).to(params[4 * n_hidden + 1].dtype)
            # fp32 [cols, C_l]: gradient w.r.t. the output of hidden layer l.  None under a one-channel head: est_in_bwd forms the
            # rank-one dlogit[col] * w_head[c] itself; several output channels sum their rank-one terms here
            dA = None if n_out == 1 else torch.mm(dl.t(), wh)
            if n_out == 1:
                dl, wh = dl[0], wh[0]
            # (dY, d gamma / d beta partials) of layer l when the fused data gradient of layer l + 1 already went through this layer's
            # InstanceNorm + LeakyReLU adjoint (dfepe_est_dgrad_in_bwd), plus what the gamma == 0 fix needs in place of dA
            pending = None
            fixes: list = []
            fix_at_end = n_hidden <= _TAB and cols * sum(int(a.shape[2]) for a in acts[1:]) * 4 <= FIX_AT_END_BYTES
            for l in range(n_hidden - 1, -1, -1):
                W, bconv, gamma, beta = params[4 * l:4 * l + 4]
                Co, Ci = W.shape[0], W.shape[1]
                a_out, a_in = acts[l + 1], acts[l]
                K = a_in.shape[2]
                g32, b32 = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
                W32 = W.detach().float().reshape(Co, Ci).contiguous()
                if pending is None:
                    dY = _buf("dY", 2, cols, Co, device=dev, dtype=BF16)
                    dg = _buf("dg", B, Co, device=dev, dtype=torch.float32)
                    db = _buf("db", B, Co, device=dev, dtype=torch.float32)
                    if _fused(N):
                        rc = lib.dfepe_est_in_bwd(_ptr(dA), _ptr(dl if dA is None else None), _ptr(wh if dA is None else None), _ptr(a_out),
                                                  cols * Co, _ptr(rstds[l]), _ptr(g32), _ptr(b32), float(slope), Co, cols, _ptr(dY), cols * Co,
                                                  _ptr(dg), _ptr(db), st)
                        _lib.check(rc, "dfepe_est_in_bwd")
                    else:
                        sp = _row_splits(B, Co, N)
                        part = _buf("npart", B * sp * 2 * Co, device=dev, dtype=torch.float32) if sp > 1 else None
                        rc = lib.dfepe_est_in_bwd_n(_ptr(dA), _ptr(dl if dA is None else None), _ptr(wh if dA is None else None), _ptr(a_out),
                                                    cols * Co, _ptr(rstds[l]), _ptr(g32), _ptr(b32), float(slope), Co, B, N, _ptr(dY), cols * Co,
                                                    _ptr(dg), _ptr(db), sp, _ptr(part), st)
                        _lib.check(rc, "dfepe_est_in_bwd_n")
                    zero_src = (dA, dl if dA is None else None, wh if dA is None else None, None, 0, None, 0)
                else:
                    dY, dg, db, dY_up, W_up = pending  # dA was never written: the fix recomputes its channel from dY_up W_up
                    zero_src = (None, None, None, dY_up, cols * W_up.shape[0], W_up, W_up.shape[0])
                # channels whose gamma is exactly 0: x^ cannot be recovered from the stored activation; their d gamma is recomputed from
                # the layer's input (idle workgroups otherwise; N beyond the fix kernel's 4096 keeps the documented zero).  Over few
                # columns (the reference's batch sizes) every layer's fix waits for ONE launch at the end -- its inputs, dY among
                # them, stay alive until then; over many they are released layer by layer
                if N <= 4096:
                    fix = zero_src + (a_out, cols * Co, a_in, cols * K, W32, Ci, rstds[l], g32, Co, dg)
                    if fix_at_end:
                        fixes.append(fix)
                    else:
                        _dgamma_zero([fix], slope, N, B)
                pending = None
                # dW = dY^T X (split-K over the columns; the partials are a segment of the final reduction: deterministic)
                slices = _slices_for(Co, K, cols)
                partw = _buf("partw", slices, Co, K, device=dev, dtype=torch.float32)
                rc = lib.dfepe_est_gemm_tn(_ptr(dY), cols * Co, Co, _ptr(a_in), cols * K, K, cols, slices, _ptr(partw), st)
                _lib.check(rc, "dfepe_est_gemm_tn")
                # d gamma, d beta (per-pair partials), dW (split-K partials), and the convolution bias: it cancels in the instance
                # normalisation -- an exact zero (rows = 0), like the reference's autograd up to its 1e-16 noise
                segs += [(dg, B, Co), (db, B, Co), (partw, slices, Co * K), (None, 0, Co)]
                sinks += [(4 * l + 2, gamma), (4 * l + 3, beta), (4 * l, W), (4 * l + 1, bconv)]
                need_dx = l > 0 or ctx.needs_input_grad[1]
                if need_dx:
                    Mp = K  # a multiple of 32
                    WTp = WTps[l]  # two bf16 planes of W^T [K, Co], made with the forward's weight planes (dfepe_est_wprep)
                    if l > 0 and _fused(N) and Ci == K and FUSE_DGRAD:
                        # the data gradient dA = dY W stays in the GEMM's accumulators and goes straight through the adjoint of the layer
                        # below: dY, d gamma / d beta partials of layer l - 1 out, dA never written (8 of 20 bytes per element)
                        gl, bl = params[4 * (l - 1) + 2].detach().float().contiguous(), params[4 * (l - 1) + 3].detach().float().contiguous()
                        dYd = _buf("dY", 2, cols, K, device=dev, dtype=BF16)
                        dgd = _buf("dg", B, K, device=dev, dtype=torch.float32)
                        dbd = _buf("db", B, K, device=dev, dtype=torch.float32)
                        rc = lib.dfepe_est_dgrad_in_bwd(_ptr(WTp), Mp * Co, _ptr(dY), cols * Co, K, cols, Co, _ptr(a_in), cols * K, _ptr(rstds[l - 1]),
                                                        _ptr(gl), _ptr(bl), float(slope), _ptr(dYd), cols * K, _ptr(dgd), _ptr(dbd), st)
                        _lib.check(rc, "dfepe_est_dgrad_in_bwd")
                        pending = (dYd, dgd, dbd, dY, W32)
                        dA = None
                    else:
                        dA = _buf("dA", cols, Mp, device=dev, dtype=torch.float32)
                        rc = lib.dfepe_est_gemm_nt(_ptr(WTp), Mp * Co, _ptr(dY), cols * Co, Mp, cols, Co, 2, _ptr(dA), Mp, st)
                        _lib.check(rc, "dfepe_est_gemm_nt")
                del dY
            if fixes:
                _dgamma_zero(fixes, slope, N, B)
            del fixes
            sums = _colsum(segs, dev)
            grads[4 * n_hidden] = torch.stack(sums[:n_out]).reshape(Wh.shape).to(Wh.dtype) if n_out > 1 else sums[0].reshape(Wh.shape).to(Wh.dtype)
            for (slot, like), v in zip(sinks[n_out:], sums[n_out:]):
                if slot % 4 == 0:  # a weight gradient [Co, K]: the K - Ci zero-padded input channels dropped
                    Co_, Ci_ = like.shape[0], like.shape[1]
                    v = v.view(Co_, -1)
                    v = v if v.shape[1] == Ci_ else v[:, :Ci_]
                grads[slot] = v.reshape(like.shape).to(like.dtype)
            gx = None
            if ctx.needs_input_grad[1]:
                gx = dA[:, :C0].reshape(B, N, C0).permute(0, 2, 1).contiguous()
        if "clone" in _DEBUG_ZERO:
            grads = [None if g is None else g.clone() for g in grads]
        return (None, gx, *grads)


class Prepared:
    """One estimator's parameters as the library wants them, made ONCE per model forward (round 6):
      packed   every parameter in one fp32 vector (torch.cat: differentiable, its backward hands each parameter a VIEW of the packed
               gradient) -- an estimator called k times in a forward (DeepFNet.update_weights: depth - 1 calls,
               deepFEPE/models/DeepFNet.py:510) then costs autograd k - 1 additions of one vector instead of k - 1 per parameter
               (66 `add` launches per step at depth 5), and every call writes ALL its parameter gradients into one buffer;
      prep     the weights' planes (dfepe_est_prepare: power-of-two scales, scaled fp16 planes, transposed bf16 planes): two
               launches per forward instead of two per call.
    Holds the parameter objects it was made of: estimator_forward uses it only for exactly those."""

    __slots__ = ("params", "packed", "prep", "n_hidden", "Co", "Ci", "W", "gamma", "beta", "w_head", "b_head", "off", "numel", "device")

    def matches(self, flat: Sequence[Optional[Tensor]]) -> bool:
        return len(flat) == len(self.params) and all(a is b for a, b in zip(self.params, flat))

    def pointers(self, base: int):
        """(W[], bias[], gamma[], beta[], w_head, b_head) as ctypes pointer arrays / ints into a packed vector that starts at `base`."""
        n = self.n_hidden
        arr = lambda k: (ctypes.c_void_p * n)(*[base + 4 * self.off[4 * l + k] for l in range(n)])
        bh = self.off[4 * n + 1]
        return arr(0), arr(1), arr(2), arr(3), base + 4 * self.off[4 * n], (None if bh is None else base + 4 * bh)


def _prepare_ok(flat: Sequence[Optional[Tensor]], n_hidden: int) -> bool:
    """One library call per pass serves: a one-channel head, <= 8 hidden layers whose widths are multiples of 32, fp32 parameters on
    one GPU; everything else keeps the per-launch host code of _EstimatorFunction.  Every tensor is looked at on every call (ADVICE r5:
    a cached answer keyed on object identity went stale when one parameter's .data was swapped)."""
    if not USE_PASS or n_hidden < 1 or n_hidden > _TAB or len(flat) != 4 * n_hidden + 2:
        return False
    dev = None
    for i, p in enumerate(flat):
        if p is None:
            if i != 4 * n_hidden + 1:
                return False
            continue
        if p.dtype != torch.float32 or (dev is not None and p.device != dev):
            return False
        dev = p.device
    prev = None
    for l in range(n_hidden):
        W = flat[4 * l]
        if W.dim() != 3 or W.shape[2] != 1 or (prev is not None and W.shape[1] != prev) or W.shape[0] % 32:
            return False
        prev = W.shape[0]
        if any(flat[4 * l + k].numel() != prev for k in (1, 2, 3)):
            return False
    Wh, bh = flat[4 * n_hidden], flat[4 * n_hidden + 1]
    return Wh.dim() == 3 and Wh.shape[0] == 1 and Wh.shape[1] == prev and Wh.shape[2] == 1 and (bh is None or bh.numel() == 1)


def prepare(hidden: Sequence[Tuple[Tensor, Tensor, Tensor, Tensor]], head: Tuple[Tensor, Optional[Tensor]]) -> Optional[Prepared]:
    """The Prepared form of an estimator's parameters (None when the one-call-per-pass path does not serve them: estimator_forward then
    takes its per-launch host code).  Three launches: the cat, and the two of dfepe_est_prepare."""
    flat: List[Optional[Tensor]] = []
    for layer in hidden:
        flat.extend(layer)
    flat.extend(head)
    n = len(hidden)
    if not _prepare_ok(flat, n) or not flat[0].is_cuda:
        return None
    lib = _lib.lib()
    P = Prepared()
    P.params = tuple(flat)
    P.n_hidden = n
    P.device = flat[0].device
    off, at = [], 0
    for p in flat:
        off.append(None if p is None else at)
        at += 0 if p is None else p.numel()
    P.off, P.numel = off, at
    with _on(P.device):
        P.packed = torch.cat([p.reshape(-1) for p in flat if p is not None])
        P.Co = _int_array([int(flat[4 * l].shape[0]) for l in range(n)])
        P.Ci = _int_array([int(flat[4 * l].shape[1]) for l in range(n)])
        P.W, _, P.gamma, P.beta, P.w_head, P.b_head = P.pointers(P.packed.data_ptr())
        P.prep = torch.empty(lib.dfepe_est_prep_bytes(n, P.Co, P.Ci), device=P.device, dtype=torch.uint8)
        rc = lib.dfepe_est_prepare(n, P.W, P.Co, P.Ci, _ptr(P.prep), _stream())
        _lib.check(rc, "dfepe_est_prepare")
    return P


class _EstimatorPackedFunction(torch.autograd.Function):
    """The whole stack through ONE library call per pass (dfepe_est_forward / dfepe_est_backward) on the PACKED parameters of a Prepared:
    args (cfg, prepared, x, packed); the backward returns ONE gradient vector for `packed`.  At the reference's batch sizes the host was
    the limiter of the eager step (round 5: one call instead of ~30 launches and ~40 allocations from Python); round 6 moved the weights'
    preparation out of the call and the parameter gradients into one buffer."""

    @staticmethod
    def forward(ctx, cfg, P, x, packed):
        eps, slope, keep = cfg
        lib = _lib.lib()
        B, C0, N = x.shape
        dev = x.device
        n = P.n_hidden
        with _on(dev):
            st = _stream()
            xin = x.detach()
            # any fp32 layout whose points are contiguous is read in place: the model hands over [B, C, N] VIEWS of its channel-major
            # [C, B, N] input buffers (ops.estimator_input), and the input gradient goes back in the same layout (its rows are then
            # the dense [B, N] blocks the fit's adjoint wants) -- round 5 copied both ways
            if not (xin.dtype == torch.float32 and (xin.stride(2) == 1 or N == 1) and xin.stride(0) > 0 and xin.stride(1) > 0):
                xin = xin.float().contiguous()
            need_gx = bool(keep and ctx.needs_input_grad[2])
            saved = None
            if keep:
                saved = torch.empty(lib.dfepe_est_saved_bytes(n, P.Co, P.Ci, B, C0, N, int(need_gx)), device=dev, dtype=torch.uint8)
            ws = torch.empty(lib.dfepe_est_forward_workspace_bytes(n, P.Co, P.Ci, B, C0, N, int(keep)), device=dev, dtype=torch.uint8)
            logits = torch.empty(B, 1, N, device=dev, dtype=torch.float32)
            rc = lib.dfepe_est_forward(_ptr(xin), xin.stride(0), xin.stride(1), B, C0, N, n, P.W, P.gamma, P.beta, P.Co, P.Ci, P.w_head, P.b_head, float(eps), float(slope),
                                       _ptr(saved), int(need_gx), _ptr(ws), _ptr(P.prep), _ptr(logits), st)
            _lib.check(rc, "dfepe_est_forward")
        ctx.cfg = cfg
        ctx.P = P  # keeps `prep` alive until the backward has read it
        ctx.shape = (B, C0, N)
        ctx.need_gx = need_gx
        ctx.x_strides = (xin.stride(0), xin.stride(1))
        ctx.save_for_backward(*([packed, saved] if keep else []))
        return logits

    @staticmethod
    def backward(ctx, g_logits):
        eps, slope, _keep = ctx.cfg
        lib = _lib.lib()
        B, C0, N = ctx.shape
        P = ctx.P
        n = P.n_hidden
        packed, saved = ctx.saved_tensors
        dev = g_logits.device
        with _on(dev):
            st = _stream()
            gl = g_logits.detach()
            gl = gl if (gl.dtype == torch.float32 and gl.is_contiguous()) else gl.float().contiguous()
            ws = torch.empty(lib.dfepe_est_backward_workspace_bytes(n, P.Co, P.Ci, B, C0, N, int(ctx.need_gx)), device=dev, dtype=torch.uint8)
            flat = torch.empty_like(packed)  # every parameter gradient, laid out like `packed`: each element is written by the call
            gW, gb, gg, gbt, gwh, gbh = P.pointers(flat.data_ptr())
            gx = None
            if ctx.need_gx:
                if ctx.x_strides == (N, B * N):  # x was a view of a channel-major buffer: so is its gradient
                    gx = torch.empty(C0, B, N, device=dev, dtype=torch.float32).permute(1, 0, 2)
                else:
                    gx = torch.empty(B, C0, N, device=dev, dtype=torch.float32)
            rc = lib.dfepe_est_backward(_ptr(gl), B, C0, N, n, P.W, P.gamma, P.beta, P.Co, P.Ci, P.w_head, float(slope), _ptr(saved), _ptr(ws),
                                        _ptr(P.prep), gW, gb, gg, gbt, gwh, gbh, _ptr(gx), 0 if gx is None else gx.stride(0),
                                        0 if gx is None else gx.stride(1), st)
            _lib.check(rc, "dfepe_est_backward")
        return (None, None, gx, flat if ctx.needs_input_grad[3] else None)


def _pass_ok(x: Tensor, flat: Sequence[Optional[Tensor]], n_hidden: int) -> bool:
    """Does the one-call-per-pass path serve these parameters for this input?  (_prepare_ok plus: same device, matching width.)"""
    return _prepare_ok(flat, n_hidden) and x.dim() == 3 and flat[0].device == x.device and flat[0].shape[1] == x.shape[1]


def estimator_forward(x: Tensor, hidden: Sequence[Tuple[Tensor, Tensor, Tensor, Tensor]], head: Tuple[Tensor, Optional[Tensor]],
                      eps: float = 1e-5, slope: float = 0.01, prepared: Optional[Prepared] = None) -> Tensor:
    """x [B, C0, N] fp32 on the GPU -> logits [B, O, N].  hidden: per layer (conv weight, conv bias, InstanceNorm weight,
    InstanceNorm bias); head: (conv weight [O,C,1], bias [O] or None).  prepared: prepare(hidden, head) of THESE parameter objects, made
    once by a caller that evaluates the estimator several times per forward; without it (or with one made of other objects) the call
    prepares its own."""
    if not supported(x):
        raise _lib.DfepeError(f"estimator_forward: needs a GPU tensor [B >= 1, C, N >= 2], got {tuple(x.shape)} on {x.device}")
    flat: List[Optional[Tensor]] = []
    for layer in hidden:
        flat.extend(layer)
    flat.extend(head)
    if prepared is not None and not (prepared.matches(flat) and prepared.device == x.device and _prepare_ok(flat, len(hidden))):
        prepared = None
    if prepared is None and _pass_ok(x, flat, len(hidden)):
        prepared = prepare(hidden, head)
    if prepared is not None and prepared.params[0].shape[1] == x.shape[1]:
        keep = torch.is_grad_enabled() and (x.requires_grad or prepared.packed.requires_grad)
        return _EstimatorPackedFunction.apply((float(eps), float(slope), bool(keep)), prepared, x, prepared.packed)
    keep = torch.is_grad_enabled() and (x.requires_grad or any(p is not None and p.requires_grad for p in flat))
    return _EstimatorFunction.apply((len(hidden), float(eps), float(slope), bool(keep)), x, *flat)
