"""The C ABI of the homography estimator without a GPU: the symbols are exported, the version did not move, and every refusal
include/dfepe.h lists is made on the host before anything is launched."""
import ctypes

INVALID, UNSUPPORTED = -1, -3


def _est(L, B=2, N=100, t=3.0, p=0.995, iters=64, flags=0, ptrs=True, align=0):
    buf = ctypes.create_string_buffer(64)
    a = (ctypes.addressof(buf) + 15) // 16 * 16 + align  # host memory: only looked at, never dereferenced before the refusals
    m, ws, o = (a, a, a) if ptrs else (None, None, None)
    return L.dfepe_ransac_homography(m, None, B, N, t, p, iters, 0, flags, ws, o, None, o, o, o, None, None, None)


def test_symbols_and_version(dfepe):
    L = dfepe._lib.lib()
    raw = ctypes.CDLL(dfepe.LIB_PATH)
    for name in ("dfepe_homography_workspace_bytes", "dfepe_ransac_homography", "dfepe_homography_transfer", "dfepe_homography_corners"):
        assert hasattr(raw, name) and name in dfepe.EXPORTED_SYMBOLS
    assert L.dfepe_version() == 154
    assert dfepe._lib.HOMOGRAPHY_ALL_POINTS == 1 and dfepe._lib.HOMOGRAPHY_NO_REFINE == 2


def test_workspace_bytes(dfepe):
    L = dfepe._lib.lib()
    assert L.dfepe_homography_workspace_bytes(8, 1000, 2000) == 8 * 9 * 8 + 8 * 2000 * 4
    assert L.dfepe_homography_workspace_bytes(0, 1000, 2000) == 0 and L.dfepe_homography_workspace_bytes(8, 1000, 0) == 0


def test_estimator_refusals_without_a_launch(dfepe):
    L = dfepe._lib.lib()
    assert _est(L, B=0, ptrs=False) == 0                                   # empty batch
    assert _est(L, B=-1) == INVALID
    assert _est(L, N=0) == INVALID and _est(L, N=4097) == UNSUPPORTED     # 1 <= N <= 4096
    assert _est(L, B=65536) == UNSUPPORTED
    assert _est(L, iters=0) == INVALID
    assert _est(L, p=-0.01) == INVALID and _est(L, p=1.01) == INVALID and _est(L, p=float("nan")) == INVALID
    assert _est(L, t=float("nan")) == INVALID
    assert _est(L, flags=4) == INVALID and _est(L, flags=1 << 31) == INVALID  # any bit but ALL_POINTS | NO_REFINE
    assert _est(L, ptrs=False) == INVALID                                  # null pointers
    assert _est(L, align=4) == INVALID                                     # matches / workspace not 16-byte aligned
    # the refusals come in the documented order: a bad flag on an empty batch is still refused
    assert _est(L, B=0, flags=8, ptrs=False) == INVALID


def test_transfer_and_corners_refusals_without_a_launch(dfepe):
    L = dfepe._lib.lib()
    buf = ctypes.create_string_buffer(64)
    a = (ctypes.addressof(buf) + 15) // 16 * 16
    tr = lambda B, N, H=a, m=a, d=a, k=a, epi=3.0: L.dfepe_homography_transfer(H, m, None, B, N, epi, d, k, None)  # noqa: E731
    assert tr(0, 10, None, None, None, None) == 0 and tr(4, 0, None, None, None, None) == 0
    assert tr(-1, 10) == INVALID and tr(4, -1) == INVALID and tr(4, 10, epi=float("nan")) == INVALID
    assert tr(4, 10, H=None) == INVALID and tr(4, 10, m=None) == INVALID and tr(4, 10, d=None, k=None) == INVALID
    assert tr(4, 10, m=a + 8) == INVALID and tr(65536, 10) == UNSUPPORTED
    co = lambda B, h=240, w=320, T=3, He=a, Hg=a, th=a, md=a, ok=a: L.dfepe_homography_corners(He, Hg, B, h, w, th, T, md, ok, None)  # noqa: E731
    assert co(0, He=None, Hg=None, th=None, md=None, ok=None) == 0
    assert co(-1) == INVALID and co(4, h=0) == INVALID and co(4, w=0) == INVALID and co(4, T=-1) == INVALID
    assert co(4, He=None) == INVALID and co(4, Hg=None) == INVALID and co(4, th=None) == INVALID and co(4, ok=None) == INVALID
    assert co(4, T=0, md=None) == INVALID


def test_python_layer_refuses_cpu_tensors_and_unbuilt_methods(dfepe):
    import numpy as np
    import pytest
    import torch

    with pytest.raises(dfepe.DfepeError):
        dfepe.ops.ransac_homography(torch.zeros(2, 10, 4))
    with pytest.raises(dfepe.DfepeError):
        dfepe.ops.homography_transfer(torch.zeros(2, 3, 3), torch.zeros(2, 10, 4))
    with pytest.raises(dfepe.DfepeError):
        dfepe.ops.homography_corners(torch.zeros(2, 3, 3), torch.zeros(2, 3, 3), 240, 320, torch.zeros(3))
    pts = np.zeros((10, 2), np.float32)
    for method in (4, 16):
        with pytest.raises(NotImplementedError):
            dfepe.compat.utils_opencv.findHomography(pts, pts, method)
    with pytest.raises(NotImplementedError):
        dfepe.compat.descriptor_evaluation.compute_homography({}, orb=True)
    H, mask = dfepe.compat.utils_opencv.findHomography(pts[:3], pts[:3])  # fewer than four points: no model, no device needed
    assert H is None and mask.shape == (3, 1) and mask.dtype == np.uint8
    assert np.allclose(dfepe.compat.descriptor_evaluation.warp_keypoints(np.array([[1.0, 2.0]]), np.array([[1, 0, 3], [0, 1, 4], [0, 0, 2.0]])),
                       [[2.0, 3.0]])
