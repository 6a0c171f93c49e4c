"""The device-side sampler of the DSAC loop (csrc/sampler.hip): minimal sets drawn on the stream, uniform or weighted."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from ._base import Tensor, _n_valid_arg, _on, _on_gpu, _prep, _ptr, _shape, _stream, _workspace

_MASK64 = (1 << 64) - 1


def _counter_arg(counter, name: str) -> Tensor:
    _on_gpu(counter, f"{name}: counter")
    if counter.dtype != torch.uint32 or counter.numel() != 1 or not counter.is_contiguous():
        raise ValueError(f"{name}: counter must be one uint32 on the GPU, got {counter.dtype} {tuple(counter.shape)}")
    return counter


def sample_sets(B: int, N: int, H: int, S: int = 10, *, seed: int, offset: int = 0, counter: Optional[Tensor] = None,
                weights: Optional[Tensor] = None, n_valid: Optional[Tensor] = None, device=None, want_fallback: bool = False):
    """idx [B,H,S] int32 for ops.dsac, drawn on the current stream (dfepe_sample_sets, include/dfepe.h): H sets of S distinct
    correspondences for each of B pairs of N.  Philox4x32-10 under the 64-bit ``seed``; the stream offset is ``offset`` plus the
    one-element uint32 device tensor ``counter`` (read by the kernel: advance it with sampler_advance and a captured draw samples
    afresh on every replay).  ``weights`` None: every S-subset of the first n correspondences is equally likely (random.sample's law for
    the set).  ``weights`` [B,N] on the GPU: successive sampling without replacement in proportion to the weights (quantised to 30
    bits under the pair's largest; NaN, +-inf and <= 0 are never drawn); a pair with fewer than S drawable weights is drawn uniformly
    and flagged.  ``n_valid`` [B] int32 on the GPU: only the first clamp(n_valid[b], S, N) correspondences of pair b can be drawn.
    Returns idx, or (idx, fallback [B] int32) with ``want_fallback``.  A set depends on (seed, offset, b, h, n, S) and its pair's
    weights alone.  No host synchronisation and no allocation inside the call; capturable.  The device is that of weights, n_valid or
    counter, else ``device``, else the current one."""
    B, N, H, S = int(B), int(N), int(H), int(S)
    if B < 0 or H < 1 or not _lib.DSAC_MIN_SAMPLE <= S <= _lib.DSAC_MAX_SAMPLE or N < S:
        raise ValueError(f"sample_sets: needs B >= 0, H >= 1 and {_lib.DSAC_MIN_SAMPLE} <= S <= {_lib.DSAC_MAX_SAMPLE} <= N, got B={B}, H={H}, S={S}, N={N}")
    given = [t for t in (weights, n_valid, counter) if torch.is_tensor(t) and t.is_cuda]
    dev = given[0].device if given else torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise _lib.DfepeError("sample_sets: the device must be a GPU (this package has no CPU path)")
    if weights is not None:
        weights = _prep(weights, "sample_sets: weights")
        _shape(weights, "weights", B, N)
        if N > _lib.SAMPLER_MAX_WEIGHTED_N:
            raise ValueError(f"sample_sets: weighted mode takes N <= {_lib.SAMPLER_MAX_WEIGHTED_N}, got {N}")
    if counter is not None:
        counter = _counter_arg(counter, "sample_sets")
    if n_valid is not None:
        _on_gpu(n_valid, "sample_sets: n_valid")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    n_valid = _n_valid_arg(n_valid, B, dev, "sample_sets")
    L = _lib.lib()
    idx = torch.empty(B, H, S, device=dev, dtype=torch.int32)
    fallback = torch.zeros(B, device=dev, dtype=torch.int32) if want_fallback else None
    if B > 0:
        ws = _workspace(L.dfepe_sample_sets_workspace_bytes(B, N, 1), dev) if weights is not None else None
        with _on(dev):
            rc = L.dfepe_sample_sets(_stream(), B, N, H, S, int(seed) & _MASK64, int(offset) & 0xFFFFFFFF, _ptr(counter), _ptr(weights),
                                     _ptr(n_valid), _ptr(idx), _ptr(fallback), _ptr(ws))
        _lib.check(rc, "dfepe_sample_sets")
    return (idx, fallback) if want_fallback else idx


def sampler_advance(counter: Tensor, by: int = 1) -> Tensor:
    """counter += by (mod 2^32) on the current stream, by a one-thread launch (dfepe_sampler_advance): the next sample_sets that reads
    this counter draws the next offset, inside a captured graph too.  Returns ``counter``."""
    counter = _counter_arg(counter, "sampler_advance")
    with _on(counter.device):
        rc = _lib.lib().dfepe_sampler_advance(_stream(), _ptr(counter), int(by) & 0xFFFFFFFF)
    _lib.check(rc, "dfepe_sampler_advance")
    return counter
