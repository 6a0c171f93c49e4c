"""What every module of the binding shares: pointers, the current stream, the device guard and the argument checks."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib

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


def _on_gpu(t, name: str) -> None:
    """The one refusal of an argument that is not a tensor on the GPU: a missing kernel path is an error, never a detour."""
    if not (torch.is_tensor(t) and t.is_cuda):
        raise _lib.DfepeError(f"{name} must live on the GPU (this package has no CPU path)")


def _prep(t: Tensor, name: str) -> Tensor:
    if not t.is_cuda:  # read here, so that an accepted tensor (every launch has several) pays no call for the refusal
        _on_gpu(t, name)
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _workspace(nbytes, dev) -> Tensor:
    """nbytes of 16-byte aligned scratch from the caching allocator, so that a captured step owns it (at least one cell)."""
    return torch.empty(max(1, (int(nbytes) + 15) // 16), 2, dtype=torch.float64, device=dev)


def _shape(t: Tensor, name: str, *dims) -> None:
    """Raise ValueError unless t has the given shape (None = any size): the kernels index raw pointers, so a wrong
    layout would be a silent out-of-bounds read, not an exception."""
    if t.dim() != len(dims) or any(d is not None and t.shape[i] != d for i, d in enumerate(dims)):
        want = "[" + ",".join("?" if d is None else str(d) for d in dims) + "]"
        raise ValueError(f"{name} must have shape {want}, got {tuple(t.shape)}")


def _n_valid_arg(n_valid, B: int, dev, name: str) -> Optional[Tensor]:
    if n_valid is None:
        return None
    if not torch.is_tensor(n_valid) or not n_valid.is_cuda:
        raise _lib.DfepeError(f"{name}: n_valid must be an int32 [B] tensor on the GPU (the counts stay on the device)")
    if n_valid.shape != (B,):
        raise ValueError(f"{name}: n_valid must have shape [{B}], got {tuple(n_valid.shape)}")
    return n_valid.to(device=dev, dtype=torch.int32).contiguous()


def _h9(H: Tensor, name: str, B: int) -> Tensor:
    _on_gpu(H, name)
    if H.shape not in ((B, 3, 3), (B, 9)):
        raise ValueError(f"{name} must have shape [{B},3,3], got {tuple(H.shape)}")
    return H.to(torch.float64).contiguous()
