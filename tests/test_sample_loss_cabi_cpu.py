"""The C ABI and the Python surface of the sample-loss branch without a GPU: every refusal of the six entry points is made on the host
before any HIP call, in the order include/dfepe.h documents; the rows of the ctypes table; the compat layer's host-side contract
(constructor, attributes, state_dict keys, refusals, the host draw against the recorded sets of the reference under the same seed)."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

INVALID, UNSUPPORTED = -1, -3
NAMES = ("dfepe_sample_loss_max_virt", "dfepe_sample_scatter_chunk", "dfepe_sample_multisets", "dfepe_topk_select", "dfepe_sample_gather",
         "dfepe_sample_floss_fwd", "dfepe_sample_floss_bwd", "dfepe_sample_scatter_bwd")


def _addr(align=0):
    buf = ctypes.create_string_buffer(64)  # host memory: only looked at, never dereferenced before the refusals
    _addr.keep.append(buf)
    return (ctypes.addressof(buf) + 15) // 16 * 16 + align


_addr.keep = []


def test_symbols_rows_and_getters(dfepe):
    L = dfepe._lib.lib()
    raw = ctypes.CDLL(dfepe.LIB_PATH)
    i, u, u64, f, P = ctypes.c_int, ctypes.c_uint, ctypes.c_ulonglong, ctypes.c_float, ctypes.c_void_p
    rows = {"dfepe_sample_loss_max_virt": (i, []), "dfepe_sample_scatter_chunk": (i, []),
            "dfepe_sample_multisets": (i, [P, i, i, i, i, u64, u, P, P, P, P, P, P]),
            "dfepe_topk_select": (i, [P, P, P, i, i, i, P, P]),
            "dfepe_sample_gather": (i, [P, P, P, P, P, i, i, i, i, P, P, P, P]),
            "dfepe_sample_floss_fwd": (i, [P, P, i, i, P, P, i, P, P, i, f, P]),
            "dfepe_sample_floss_bwd": (i, [P, P, i, i, P, P, i, P, P, i, f, P, P]),
            "dfepe_sample_scatter_bwd": (i, [P, P, P, P, P, P, i, i, i, i, P])}
    for name in NAMES:
        assert hasattr(raw, name) and name in dfepe.EXPORTED_SYMBOLS
        assert dfepe._lib._SIGNATURES[name] == rows[name], name
    assert L.dfepe_version() == 154
    assert L.dfepe_sample_loss_max_virt() == 2048 and L.dfepe_sample_scatter_chunk() % 64 == 0
    assert (dfepe._lib.SAMPLE_MIN_DRAWS, dfepe._lib.SAMPLE_MAX_DRAWS) == (8, 32)


def test_multisets_refusals_in_order(dfepe):
    L = dfepe._lib.lib()
    a = _addr()

    def call(B=2, N=40, H=3, K=20, weights=None, n_valid=None, idx=a, fallback=None, ws=None, counter=None):
        return L.dfepe_sample_multisets(None, B, N, H, K, 12345, 0, counter, weights, n_valid, idx, fallback, ws)

    assert call(B=-1) == INVALID and call(N=-1) == INVALID and call(H=0) == INVALID and call(H=-2) == INVALID
    assert call(K=7) == INVALID and call(K=33, N=64) == INVALID and call(N=19) == INVALID and call(N=31, K=32) == INVALID
    assert call(B=0) == 0 and call(B=0, idx=None) == 0 and call(B=0, weights=a, ws=None) == 0 and call(B=0, N=1 << 30, weights=a) == 0
    assert call(B=0, K=7) == INVALID and call(B=0, N=5) == INVALID and call(B=0, H=0) == INVALID
    assert call(idx=None) == INVALID and call(idx=None, weights=a, ws=None) == INVALID
    assert call(weights=a, ws=None) == INVALID and call(weights=a, ws=_addr(8)) == INVALID and call(weights=a, ws=_addr(4)) == INVALID
    assert call(B=1 << 14, H=1 << 14, K=8) == UNSUPPORTED and call(B=1 << 14, H=1 << 14, K=8, idx=None) == INVALID
    assert call(B=1 << 14, H=1 << 14, K=8, weights=a, ws=_addr(8)) == INVALID
    assert call(N=(1 << 20) + 1, weights=a, ws=a) == UNSUPPORTED and call(N=(1 << 20) + 1, weights=a, ws=_addr(8)) == INVALID


def test_topk_gather_scatter_refusals_in_order(dfepe):
    L = dfepe._lib.lib()
    a = _addr()
    topk = lambda B=2, N=40, K=20, x=a, idx=a: L.dfepe_topk_select(None, x, None, B, N, K, idx, None)
    assert topk(B=-1) == INVALID and topk(N=0) == INVALID and topk(K=0) == INVALID and topk(K=41) == INVALID
    assert topk(B=0) == 0 and topk(B=0, x=None) == 0 and topk(B=0, K=41) == INVALID
    assert topk(x=None) == INVALID and topk(idx=None) == INVALID
    assert topk(B=1 << 20, N=1 << 12, K=1 << 12) == UNSUPPORTED and topk(B=1 << 20, N=1 << 12, K=1 << 12, idx=None) == INVALID

    def gather(B=2, N=40, H=3, K=20, **nulls):
        p = {k: None if k in nulls else a for k in ("pts1", "pts2", "weights", "idx", "o1", "o2", "ow", "accu")}
        return L.dfepe_sample_gather(None, p["pts1"], p["pts2"], p["weights"], p["idx"], B, N, H, K, p["o1"], p["o2"], p["ow"], p["accu"])

    assert gather(B=-1) == INVALID and gather(N=0) == INVALID and gather(H=0) == INVALID and gather(K=0) == INVALID
    assert gather(B=0) == 0 and gather(B=0, pts1=1) == 0 and gather(B=0, H=0) == INVALID
    for k in ("pts1", "pts2", "weights", "idx", "o1", "o2", "ow"):
        assert gather(**{k: 1}) == INVALID, k
    assert gather(B=1 << 14, H=1 << 14, K=8) == UNSUPPORTED and gather(B=1 << 14, H=1 << 14, K=8, idx=1) == INVALID

    def scatter(B=2, N=40, H=3, K=20, **nulls):
        p = {k: None if k in nulls else a for k in ("gws", "gaccu", "weights", "accu", "idx", "gw")}
        return L.dfepe_sample_scatter_bwd(None, p["gws"], p["gaccu"], p["weights"], p["accu"], p["idx"], B, N, H, K, p["gw"])

    assert scatter(B=-1) == INVALID and scatter(N=0) == INVALID and scatter(H=0) == INVALID and scatter(K=0) == INVALID
    assert scatter(B=0) == 0 and scatter(B=0, idx=1) == 0
    assert scatter(idx=1) == INVALID and scatter(gw=1) == INVALID
    assert scatter(weights=1) == INVALID and scatter(accu=1) == INVALID
    assert scatter(B=1 << 14, H=1 << 14, K=8) == UNSUPPORTED and scatter(B=65536, H=1, K=8) == UNSUPPORTED
    assert scatter(B=1 << 14, H=1 << 14, K=8, weights=1) == INVALID


def test_floss_refusals_in_order(dfepe):
    L = dfepe._lib.lib()
    a = _addr()

    def both(B=2, H=3, M=10, t_stride=9, **nulls):
        p = {k: None if k in nulls else a for k in ("F", "T1", "T2", "v1", "v2", "out", "g")}
        f = L.dfepe_sample_floss_fwd(None, p["F"], B, H, p["T1"], p["T2"], t_stride, p["v1"], p["v2"], M, 0.02, p["out"])
        b = L.dfepe_sample_floss_bwd(None, p["F"], B, H, p["T1"], p["T2"], t_stride, p["v1"], p["v2"], M, 0.02, p["g"], p["out"])
        return f, b

    for bad in (dict(B=-1), dict(H=0), dict(M=0), dict(t_stride=3), dict(t_stride=-9)):
        assert both(**bad) == (INVALID, INVALID), bad
    assert both(B=0) == (0, 0) and both(B=0, F=1, out=1) == (0, 0) and both(B=0, M=0) == (INVALID, INVALID)
    for k in ("F", "T1", "T2", "v1", "v2", "out"):
        assert both(**{k: 1}) == (INVALID, INVALID), k
    assert L.dfepe_sample_floss_bwd(None, a, 2, 3, a, a, 9, a, a, 10, 0.02, None, a) == INVALID  # a NULL g_loss_sum (backward only)
    assert both(M=2049) == (UNSUPPORTED, UNSUPPORTED) and both(M=2049, F=1) == (INVALID, INVALID)
    assert both(B=1 << 16, H=1 << 16) == (UNSUPPORTED, UNSUPPORTED)


def test_python_layer_contract(dfepe):
    import torch

    ops, C = dfepe.ops, dfepe.compat
    for bad in (dict(H=0), dict(K=7), dict(K=33), dict(B=2, N=19)):
        with pytest.raises(ValueError):
            ops.sample_multisets(None, **{"B": 2, "N": 40, "H": 3, "K": 20, **bad}, seed=1, device="cuda")
    with pytest.raises(dfepe.DfepeError):
        ops.sample_multisets(torch.ones(2, 40), seed=1)                       # weights on the host
    with pytest.raises(dfepe.DfepeError):
        ops.sample_multisets(None, B=2, N=40, seed=1, device="cpu")
    with pytest.raises(dfepe.DfepeError):
        ops.topk_select(torch.ones(2, 40), 20)
    with pytest.raises(dfepe.DfepeError):
        ops.sample_fits(torch.ones(2, 40, 3), torch.ones(2, 40, 3), torch.ones(2, 40), torch.zeros(2, 3, 20, dtype=torch.int32))
    with pytest.raises(dfepe.DfepeError):
        ops.sample_floss(torch.ones(2, 3, 3, 3), torch.eye(3), torch.eye(3), torch.ones(2, 5, 3), torch.ones(2, 5, 3))

    M = C.DeepFNetSampleLoss
    fit = M.Fit(True, False, False, True, True)
    assert (fit.topK, fit.selects_each_sample, fit.normalize_SVD, fit.if_sample_loss, fit.sampler) == (20, 100, True, True, None)
    assert list(inspect.signature(M.Fit.forward).parameters) == ["self", "pts1", "pts2", "weights", "if_print", "matches_good_unique_nums"]
    assert list(inspect.signature(M.Norm8PointNet.__init__).parameters)[:14] == [
        "self", "depth", "image_size", "if_quality", "if_goodCorresArch", "if_tri_depth", "if_sample_loss", "if_learn_offsets", "if_des", "des_size",
        "quality_size", "is_cuda", "is_test", "if_cpu_svd"]
    for flag in ("if_goodCorresArch", "if_tri_depth", "if_des"):
        with pytest.raises(NotImplementedError):
            M.Norm8PointNet(2, [376, 1241, 3], False, **{flag: True})
    net = M.Norm8PointNet(3, [376, 1241, 3], False, if_sample_loss=True, img_zoom_xy=(1.0, 1.0))
    ref = C.DeepFNet.DeepFNet(3, [376, 1241, 3], False)
    assert list(net.state_dict().keys()) == list(ref.state_dict().keys())     # the state_dict DeepFNet.py's estimator input fits
    assert isinstance(net.fit, M.Fit) and net.fit.if_sample_loss
    with pytest.raises(dfepe.DfepeError):                                      # CPU tensors: refused, not computed elsewhere
        net({"matches_xy_ori": torch.zeros(2, 32, 4), "matches_good_unique_nums": None, "t_scene_scale": None})
    with pytest.raises(NotImplementedError):
        C.train_good_utils.get_all_loss_DeepF({}, None, None, None, {"if_tri_depth": True, "if_sample_loss": True})


def test_host_draw_is_numpy_random_choice(dfepe):
    """Without a sampler the sets are np.random.choice's, call for call as DeepFNetSampleLoss.py:401-409 makes them: a seeded NumPy
    stream reproduces them (needs no device: the draw happens before anything is launched)."""
    import torch

    fit = dfepe.compat.DeepFNetSampleLoss.Fit()
    w = torch.softmax(torch.randn(2, 1, 50, generator=torch.Generator().manual_seed(0)), 2)
    nums = np.array([50, 33])
    np.random.seed(11)
    got = fit.draw_host(w, nums).numpy()
    np.random.seed(11)
    for b in range(2):
        p = w[b].numpy().flatten()[:nums[b]]
        p = p / np.sum(p)
        for h in range(100):
            assert (got[b, h] == np.random.choice(nums[b], 20, p=p)).all()
    assert got.shape == (2, 100, 20) and got.dtype == np.int32 and got[1].max() < 33
