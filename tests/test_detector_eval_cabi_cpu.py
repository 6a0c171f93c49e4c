"""The C ABI of the detector evaluation without a GPU: the symbols are exported, the version did not move, and every refusal
include/dfepe.h lists is made on the host before anything is launched, in the order in which it lists them."""
import ctypes

import pytest

INVALID, UNSUPPORTED = -1, -3
NAMES = ("dfepe_keypoint_repeatability_workspace_bytes", "dfepe_keypoint_repeatability", "dfepe_average_precision", "dfepe_matching_score")


def _addr(align=0):
    buf = ctypes.create_string_buffer(64)  # host memory: only looked at, never dereferenced before the refusals
    _addr.keep.append(buf)
    return (ctypes.addressof(buf) + 15) // 16 * 16 + align


_addr.keep = []


def _rep(L, B=2, N1=10, N2=12, C=3, h=120, w=160, k=300, T=2, **ptr):
    a = _addr()
    p = {name: a for name in ("kp1", "kp2", "H", "thresh", "ws", "rep", "loc", "c1", "c2", "k1", "k2", "nu")}
    p.update(ptr)
    return L.dfepe_keypoint_repeatability(p["kp1"], p["kp2"], None, None, p["H"], B, N1, N2, C, h, w, k, p["thresh"], T, p["ws"], p["rep"],
                                          p["loc"], p["c1"], p["c2"], p["k1"], p["k2"], p["nu"], None)


def test_symbols_and_version(dfepe):
    L = dfepe._lib.lib()
    raw = ctypes.CDLL(dfepe.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name) and name in dfepe.EXPORTED_SYMBOLS
    assert L.dfepe_version() == 154
    assert dfepe._lib.DETECTOR_EVAL_MAX_N == 4096


def test_workspace_bytes(dfepe):
    L = dfepe._lib.lib()
    # per point a double2, a key, a minimum, and one byte rounded up to 16 over the call
    assert L.dfepe_keypoint_repeatability_workspace_bytes(3, 100, 60) == 3 * 160 * 32 + 480
    assert L.dfepe_keypoint_repeatability_workspace_bytes(1, 1, 0) == 32 + 16
    assert L.dfepe_keypoint_repeatability_workspace_bytes(0, 100, 60) == 0 and L.dfepe_keypoint_repeatability_workspace_bytes(2, 0, 0) == 0
    assert L.dfepe_keypoint_repeatability_workspace_bytes(2, 4097, 0) == 0 and L.dfepe_keypoint_repeatability_workspace_bytes(2, -1, 5) == 0


def test_repeatability_refusals_without_a_launch(dfepe):
    L = dfepe._lib.lib()
    none = {name: None for name in ("kp1", "kp2", "H", "thresh", "ws", "rep", "loc", "c1", "c2", "k1", "k2", "nu")}
    assert _rep(L, B=0, **none) == 0                                            # empty batch
    assert _rep(L, B=-1) == INVALID and _rep(L, N1=-1) == INVALID and _rep(L, N2=-1) == INVALID and _rep(L, T=-1) == INVALID
    assert _rep(L, C=1) == INVALID and _rep(L, C=4) == INVALID
    assert _rep(L, h=0) == INVALID and _rep(L, w=0) == INVALID and _rep(L, k=-1) == INVALID
    assert _rep(L, N1=4097) == UNSUPPORTED and _rep(L, N2=4097) == UNSUPPORTED and _rep(L, B=65536) == UNSUPPORTED
    for name in ("kp1", "kp2", "H", "thresh", "ws", "rep", "loc", "c1", "c2", "k1", "k2", "nu"):
        assert _rep(L, **{name: None}) == INVALID, name                         # null pointers
    assert _rep(L, ws=_addr(8)) == INVALID                                      # workspace not 16-byte aligned
    # the documented order: a bad argument on an empty batch is still refused; the size cap comes before the pointers
    assert _rep(L, B=0, C=5, **none) == INVALID and _rep(L, B=0, k=-1, **none) == INVALID
    assert _rep(L, N1=4097, **none) == UNSUPPORTED
    # what the sizes make unnecessary may be null -- and then the next refusal is reached, so nothing was launched on the way
    assert _rep(L, N1=0, kp1=None, H=None) == INVALID and _rep(L, N2=0, kp2=None, H=None) == INVALID
    assert _rep(L, T=0, thresh=None, rep=None, loc=None, c1=None, c2=None, H=None) == INVALID
    assert _rep(L, N1=0, N2=0, ws=None, H=None) == INVALID


def test_average_precision_and_matching_score_refusals_without_a_launch(dfepe):
    L = dfepe._lib.lib()
    a = _addr()
    ap = lambda B, M, lab=a, sc=a, out=a: L.dfepe_average_precision(lab, sc, None, B, M, out, None, None, None, None)  # noqa: E731
    assert ap(0, 10, None, None, None) == 0
    assert ap(-1, 10) == INVALID and ap(2, -1) == INVALID
    assert ap(2, 4097) == UNSUPPORTED and ap(65536, 10) == UNSUPPORTED and ap(2, 4097, None, None, None) == UNSUPPORTED
    assert ap(2, 10, out=None) == INVALID and ap(2, 10, lab=None) == INVALID and ap(2, 10, sc=None) == INVALID
    assert ap(2, 0, None, None, None) == INVALID                                # M = 0 needs no labels or scores, but an output
    ms = lambda B, i=a, k=a, u=a, out=a: L.dfepe_matching_score(i, k, u, B, out, None)  # noqa: E731
    assert ms(0, None, None, None, None) == 0 and ms(-1) == INVALID
    assert ms(4, i=None) == INVALID and ms(4, k=None) == INVALID and ms(4, u=None) == INVALID and ms(4, out=None) == INVALID


def test_python_layer_refuses_cpu_tensors_and_bad_shapes(dfepe):
    import torch

    kp, H, th = torch.zeros(2, 10, 3, dtype=torch.float64), torch.eye(3).expand(2, 3, 3), torch.zeros(1)
    with pytest.raises(dfepe.DfepeError):
        dfepe.ops.keypoint_repeatability(kp, kp, H, 120, 160, 300, th)
    with pytest.raises(dfepe.DfepeError):
        dfepe.ops.average_precision(torch.zeros(2, 5, dtype=torch.uint8), torch.zeros(2, 5))
    with pytest.raises(dfepe.DfepeError):
        dfepe.ops.matching_score(torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError):
        dfepe.compat.evaluate_frontend.frontend_metrics_batch(kp, kp, kp, kp, H, (120, 160), inliers_method="orb")
    assert dfepe.compat.evaluate_frontend.nn_average_precision([], []) == 0      # no match: no device needed
    assert dfepe.compat.evaluate_frontend.nn_average_precision([0.3, 0.5], [0, 0]) == 0
    assert dfepe.compat.detector_evaluation.warp_keypoints is dfepe.compat.descriptor_evaluation.warp_keypoints
