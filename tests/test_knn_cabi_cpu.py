"""Host side of the ratio-test 2-NN matcher (dfepe_knn_match, include/dfepe.h): the symbols are exported, every refusal is made on the
host before anything is launched (so it is safe without a GPU), the workspace size, and the no-CPU-path stance of ops / compat."""
import ctypes

import numpy as np
import pytest
import torch

OK, INVALID, UNSUPPORTED = 0, -1, -3
A = 4096      # a pointer value that is 16-byte aligned and never dereferenced: every call below is refused before any launch


def _call(L, B=2, N1=10, N2=10, D=128, ratio=0.8, ratio_test=1, desc1=A, desc2=A, ws=A, outs=A, count=A):
    return L.dfepe_knn_match(desc1, desc2, B, N1, N2, D, ratio, ratio_test, ws, outs, outs, outs, outs, outs, outs, outs, count, None)


def test_symbols_are_exported(dfepe):
    lib = ctypes.CDLL(dfepe.LIB_PATH)
    for name in ("dfepe_knn_match", "dfepe_knn_match_workspace_bytes"):
        assert hasattr(lib, name) and name in dfepe.EXPORTED_SYMBOLS
    assert dfepe._lib.lib().dfepe_strerror(UNSUPPORTED) != dfepe._lib.lib().dfepe_strerror(INVALID)


def test_refusals_are_made_on_the_host(dfepe):
    L = dfepe._lib.lib()
    assert b"invalid" in L.dfepe_strerror(INVALID) and b"not supported" in L.dfepe_strerror(UNSUPPORTED)
    # negative sizes, D <= 0
    assert _call(L, B=-1) == INVALID and _call(L, N1=-1) == INVALID and _call(L, N2=-1) == INVALID
    assert _call(L, D=0) == INVALID and _call(L, D=-32) == INVALID
    # an empty batch is fine whatever else is passed
    assert _call(L, B=0, desc1=None, desc2=None, ws=None, outs=None, count=None) == OK
    # NaN ratio with the ratio test on; without the test the ratio is not looked at (and the call goes on to the next refusal)
    assert _call(L, ratio=float("nan")) == INVALID
    assert _call(L, ratio=float("nan"), ratio_test=0, D=48) == UNSUPPORTED
    # no second neighbour
    assert _call(L, N2=1) == INVALID and _call(L, N2=0) == INVALID
    # null pointers, one at a time
    assert _call(L, count=None) == INVALID and _call(L, desc1=None) == INVALID and _call(L, desc2=None) == INVALID
    assert _call(L, ws=None) == INVALID and _call(L, outs=None) == INVALID
    # D not a multiple of 32
    for D in (1, 16, 48, 100, 130):
        assert _call(L, D=D) == UNSUPPORTED, D
    # misaligned descriptors (16 bytes) and workspace (8 bytes)
    assert _call(L, desc1=A + 4) == INVALID and _call(L, desc2=A + 8) == INVALID and _call(L, ws=A + 4) == INVALID
    # more than 2^31 - 1 tiles over the batch: 32768 pairs of 256 x 256 tiles
    assert _call(L, B=32768, N1=32768, N2=32768) == UNSUPPORTED
    assert _call(L, B=32768, N1=32768, N2=32768, D=100) == UNSUPPORTED


def test_workspace_size(dfepe):
    L = dfepe._lib.lib()
    ws = L.dfepe_knn_match_workspace_bytes
    assert ws(0, 10, 20) == 0 and ws(2, -1, 20) == 0 and ws(2, 10, -1) == 0 and ws(2, 0, 20) == 0
    # one slot of two 64-bit keys per row and 64-column strip of the 128-wide tiles
    assert ws(2, 10, 20) == 2 * 10 * 2 * 2 * 8 and ws(1, 1, 128) == 32 and ws(1, 1, 129) == 64 and ws(3, 1000, 1000) == 3 * 1000 * 16 * 16
    prev = 0
    for N2 in range(2, 1030):
        cur = ws(4, 77, N2)
        assert cur >= prev and cur % 8 == 0 and cur > 0
        prev = cur
    assert ws(65536, 4096, 4096) == 65536 * 4096 * 64 * 16  # no 32-bit overflow


def test_no_cpu_path(dfepe):
    with pytest.raises(dfepe.DfepeError):
        dfepe.ops.knn_match(torch.zeros(1, 8, 32), torch.zeros(1, 8, 32))
    with pytest.raises(dfepe.DfepeError):
        dfepe.compat.utils_opencv.KNN_match_batch(torch.zeros(1, 8, 32), torch.zeros(1, 8, 32), torch.zeros(1, 8, 2), torch.zeros(1, 8, 2))


def test_compat_surface_without_a_gpu(dfepe):
    uo = dfepe.compat.utils_opencv
    des = np.zeros((8, 128), dtype=np.float32)
    x = np.zeros((8, 2), dtype=np.float32)
    with pytest.raises(NotImplementedError):
        uo.KNN_match(des, des, x, x, None, None, None, None, visualize=True)
    # no query: empty outputs in the reference's shapes, no launch
    x1, x2, all_ij, good_ij = uo.KNN_match(des[:0], des, x[:0], x, None, None, None, None)
    assert x1.shape == (0, 2) and x2.shape == (0, 2) and all_ij.shape == (0, 2) and good_ij.shape == (0, 2)
    import inspect

    assert list(inspect.signature(uo.KNN_match).parameters) == ["des1", "des2", "x1_all", "x2_all", "kp1", "kp2", "img1_rgb", "img2_rgb",
                                                               "visualize", "if_BF", "if_ratio_test"]
    sig = inspect.signature(uo.KNN_match).parameters
    assert (sig["visualize"].default, sig["if_BF"].default, sig["if_ratio_test"].default) == (False, False, True)
    assert "exact search" in uo.__doc__ and "if_BF" in uo.__doc__
