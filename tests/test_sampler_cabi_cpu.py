"""The C ABI of the device-side DSAC sampler without a GPU: every refusal of dfepe_sample_sets and dfepe_sampler_advance is made on
the host before any HIP call, in the order include/dfepe.h documents; the workspace byte counts; the getter; the Python layer's own
refusals."""
import ctypes

import pytest

INVALID, UNSUPPORTED = -1, -3


def _addr(align=0):
    buf = ctypes.create_string_buffer(64)  # host memory: only looked at, never dereferenced before the refusals
    _addr.keep.append(buf)
    return (ctypes.addressof(buf) + 15) // 16 * 16 + align


_addr.keep = []


def test_symbols_version_and_chunk(dfepe):
    L = dfepe._lib.lib()
    raw = ctypes.CDLL(dfepe.LIB_PATH)
    for name in ("dfepe_sampler_scan_chunk", "dfepe_sample_sets_workspace_bytes", "dfepe_sample_sets", "dfepe_sampler_advance"):
        assert hasattr(raw, name) and name in dfepe.EXPORTED_SYMBOLS
    assert L.dfepe_version() == 154
    chunk = L.dfepe_sampler_scan_chunk()
    assert chunk >= 64 and chunk % 64 == 0


def test_workspace_bytes(dfepe):
    L = dfepe._lib.lib()
    for B, N in ((1, 10), (3, 129), (2, 1000), (7, 33), (1, 1 << 20), (64, 1 << 20)):
        want = (B * (N + 2) * 8 + 15) // 16 * 16  # P[0 .. N] and the number of q > 0, uint64, per pair
        assert L.dfepe_sample_sets_workspace_bytes(B, N, 1) == want, (B, N)
        assert L.dfepe_sample_sets_workspace_bytes(B, N, 0) == 0
    for bad in ((0, 10), (-1, 10), (1, 0), (1, -5)):
        assert L.dfepe_sample_sets_workspace_bytes(*bad, 1) == 0


def test_refusals_without_a_launch(dfepe):
    L = dfepe._lib.lib()
    a = _addr()

    def call(B=2, N=20, H=3, S=10, weights=None, n_valid=None, idx=a, fallback=None, ws=None, counter=None):
        return L.dfepe_sample_sets(None, B, N, H, S, 12345, 0, counter, weights, n_valid, idx, fallback, ws)

    # in the documented order: the sizes ...
    assert call(B=-1) == INVALID and call(N=-1) == INVALID and call(H=0) == INVALID and call(H=-2) == INVALID
    assert call(S=7) == INVALID and call(S=17, N=40) == INVALID and call(N=9) == INVALID and call(N=15, S=16) == INVALID
    # ... then the empty batch, before any pointer is looked at: nothing is launched (there is no GPU here to launch on)
    assert call(B=0) == 0 and call(B=0, idx=None) == 0 and call(B=0, weights=a, ws=None) == 0 and call(B=0, N=1 << 30, weights=a) == 0
    assert call(B=0, S=7) == INVALID and call(B=0, N=5) == INVALID and call(B=0, H=0) == INVALID
    # ... then idx, then the weighted workspace
    assert call(idx=None) == INVALID and call(idx=None, weights=a, ws=None) == INVALID
    assert call(weights=a, ws=None) == INVALID and call(weights=a, ws=_addr(8)) == INVALID and call(weights=a, ws=_addr(4)) == INVALID
    # ... then the sizes that are not built: a misaligned workspace is refused before them
    assert call(B=1 << 14, H=1 << 14, S=8) == UNSUPPORTED and call(B=1, N=1 << 21, H=1 << 28, S=8) == UNSUPPORTED
    assert call(B=1 << 14, H=1 << 14, S=8, idx=None) == INVALID
    assert call(B=1 << 14, H=1 << 14, S=8, weights=a, ws=_addr(8)) == INVALID
    assert call(N=(1 << 20) + 1, weights=a, ws=a) == UNSUPPORTED and call(N=(1 << 20) + 1, weights=a, ws=_addr(8)) == INVALID
    assert call(B=1 << 14, N=(1 << 20) + 1, H=1 << 14, S=8, weights=a, ws=a) == UNSUPPORTED
    assert L.dfepe_sampler_advance(None, None, 1) == INVALID


def test_python_layer_refusals(dfepe):
    import torch

    ops, C = dfepe.ops, dfepe.compat
    for bad in (dict(B=-1, N=20, H=3), dict(B=2, N=20, H=0), dict(B=2, N=9, H=3), dict(B=2, N=20, H=3, S=7), dict(B=2, N=40, H=3, S=17)):
        with pytest.raises(ValueError):
            ops.sample_sets(**bad, seed=1)
    with pytest.raises(dfepe.DfepeError):
        ops.sample_sets(2, 20, 3, seed=1, device="cpu")
    with pytest.raises(dfepe.DfepeError):
        ops.sample_sets(2, 20, 3, seed=1, weights=torch.ones(2, 20), device="cuda")      # weights on the host
    with pytest.raises(dfepe.DfepeError):
        ops.sampler_advance(torch.zeros(1, dtype=torch.uint32))
    assert C.DeviceSampler is C.dsac.DeviceSampler
    d = C.DSAC(4, 100.0, 0.02, 0.1, torch.eye(3), C.H_loss.HLoss())
    assert d.sampler is None                                                             # the default stays the host draw
