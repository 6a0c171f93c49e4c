"""The C ABI of the SuperPoint output processing without a GPU: the symbols are exported, the version did not move, the capacity
and workspace sizes, and every refusal include/dfepe.h lists is made on the host before anything is launched, in the order in
which it lists them."""
import ctypes

import pytest

INVALID, UNSUPPORTED = -1, -3
NAMES = ("dfepe_sp_nms_capacity", "dfepe_sp_nms_workspace_bytes", "dfepe_sp_soft_argmax_bwd_workspace_bytes", "dfepe_sp_flatten",
         "dfepe_sp_flatten_bwd", "dfepe_sp_nms", "dfepe_sp_soft_argmax", "dfepe_sp_soft_argmax_bwd", "dfepe_sp_sample_desc",
         "dfepe_gather_offsets_bwd")
BIG = 4104  # 4104 x 4104 > 2^24 pixels, and a multiple of 8


def _addr(align=0):
    buf = ctypes.create_string_buffer(64)  # host memory: only looked at, never dereferenced before the refusals
    _addr.keep.append(buf)
    return (ctypes.addressof(buf) + 15) // 16 * 16 + align


_addr.keep = []


def test_symbols_and_version(dfepe):
    L = dfepe._lib.lib()
    raw = ctypes.CDLL(dfepe.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name) and name in dfepe.EXPORTED_SYMBOLS
    assert L.dfepe_version() == 154
    assert dfepe._lib.SP_MAX_PIXELS == 1 << 24 and dfepe._lib.SP_LDS_PIXELS == 12288 and dfepe._lib.SP_MAX_PATCH == 63


def test_capacity_and_workspace_sizes(dfepe):
    L = dfepe._lib.lib()
    cap = L.dfepe_sp_nms_capacity
    assert cap(16, 24, 0) == 384 and cap(16, 24, 1) == 96 and cap(16, 24, 4) == 4 * 5 and cap(40, 72, 8) == 5 * 8
    assert cap(368, 1240, 4) == 74 * 248 and cap(1, 1, 100) == 1
    assert cap(0, 24, 1) == 0 and cap(16, 24, -1) == 0 and cap(BIG, BIG, 4) == 0
    ws = L.dfepe_sp_nms_workspace_bytes
    # 12288 pixels stay in LDS; above: a state byte per pixel (rounded up to 16 over the call) and an int32 list entry
    assert ws(3, 96, 128) == 0 and ws(1, 104, 120) == 5 * 12480 and ws(3, 104, 120) == 15 * 12480
    assert ws(2, 368, 1240) == 10 * 368 * 1240 and ws(1, 97, 127) == (97 * 127 + 15) // 16 * 16 + 4 * 97 * 127
    assert ws(0, 104, 120) == 0 and ws(1, BIG, BIG) == 0 and ws(1, -1, 5) == 0
    bw = L.dfepe_sp_soft_argmax_bwd_workspace_bytes
    rec = bw(1, 16, 24, 1) - bw(1, 16, 24, 0)
    assert bw(1, 16, 24, 0) == 16 * 24 * 4 and rec >= 9 * 8 and rec % 8 == 0   # the index map, then one record per point
    assert bw(3, 40, 72, 40) == 3 * 40 * 72 * 4 + 3 * 40 * rec
    assert bw(0, 16, 24, 4) == 0 and bw(1, 16, 24, -1) == 0 and bw(1, BIG, BIG, 4) == 0


def test_flatten_refusals_without_a_launch(dfepe):
    L = dfepe._lib.lib()
    a = _addr()
    f = lambda B=2, H=16, W=24, semi=a, heat=a: L.dfepe_sp_flatten(semi, B, H, W, heat, None)  # noqa: E731
    assert f(B=-1) == INVALID and f(H=0) == INVALID and f(W=0) == INVALID
    assert f(H=20) == INVALID and f(W=25) == INVALID                              # not a multiple of 8
    assert f(H=BIG, W=BIG) == UNSUPPORTED and f(B=0, H=BIG, W=BIG, semi=None, heat=None) == UNSUPPORTED
    assert f(B=0, H=20, semi=None, heat=None) == INVALID                          # the order: arguments before the empty batch
    assert f(B=0, semi=None, heat=None) == 0
    assert f(semi=None) == INVALID and f(heat=None) == INVALID and f(heat=_addr(4)) == INVALID
    g = lambda B=2, H=16, W=24, semi=a, gh=a, gs=a: L.dfepe_sp_flatten_bwd(semi, gh, B, H, W, gs, None)  # noqa: E731
    assert g(B=-1) == INVALID and g(H=12) == INVALID and g(W=4) == INVALID and g(H=BIG, W=BIG) == UNSUPPORTED
    assert g(B=0, semi=None, gh=None, gs=None) == 0
    assert g(semi=None) == INVALID and g(gh=None) == INVALID and g(gs=None) == INVALID


def test_nms_refusals_without_a_launch(dfepe):
    L = dfepe._lib.lib()
    a = _addr()
    names = ("heat", "ws", "map", "pts", "conf", "count")

    def nms(B=2, H=16, W=24, d=4, r=4, **ptr):
        p = {n: a for n in names}
        p.update(ptr)
        return L.dfepe_sp_nms(p["heat"], B, H, W, 0.015, d, r, p["ws"], p["map"], p["pts"], p["conf"], p["count"], None)

    none = {n: None for n in names}
    assert nms(B=-1) == INVALID and nms(H=0) == INVALID and nms(W=0) == INVALID and nms(d=-1) == INVALID and nms(r=-1) == INVALID
    assert nms(B=0, **none) == 0 and nms(B=0, d=-1, **none) == INVALID
    assert nms(H=BIG, W=BIG) == UNSUPPORTED and nms(B=65536) == UNSUPPORTED and nms(H=BIG, W=BIG, **none) == UNSUPPORTED
    for n in ("heat", "map", "pts", "conf", "count"):
        assert nms(**{n: None}) == INVALID, n
    assert nms(H=104, W=120, ws=None) == INVALID                                   # above the LDS size a workspace is needed
    assert nms(ws=None, heat=None) == INVALID                                      # below it is not: the next refusal is reached


def test_soft_argmax_refusals_without_a_launch(dfepe):
    L = dfepe._lib.lib()
    a = _addr()

    def fwd(B=2, H=16, W=24, cap=20, p=5, r=4, heat=a, pts=a, count=a, pred=a):
        return L.dfepe_sp_soft_argmax(heat, pts, count, B, H, W, cap, p, r, pred, None, None)

    def bwd(B=2, H=16, W=24, cap=20, p=5, r=4, heat=a, pts=a, count=a, g=a, ws=a, gh=a):
        return L.dfepe_sp_soft_argmax_bwd(heat, pts, count, g, B, H, W, cap, p, r, ws, gh, None)

    for f in (fwd, bwd):
        assert f(B=-1) == INVALID and f(H=0) == INVALID and f(W=0) == INVALID and f(cap=-1) == INVALID and f(r=-1) == INVALID
        assert f(p=4) == INVALID and f(p=0) == INVALID and f(p=-3) == INVALID      # even, or not positive
        assert f(p=11, r=4) == INVALID                                             # p > 2r + 1 and f(p=3, r=0) == INVALID and f(p=1, r=0, heat=None) == INVALID
        assert f(H=BIG, W=BIG) == UNSUPPORTED and f(p=65, r=40) == UNSUPPORTED and f(B=65536, cap=65536) == UNSUPPORTED
        assert f(H=BIG, W=BIG, p=4) == INVALID                                     # the order: arguments before sizes
    assert fwd(B=0, heat=None, pts=None, count=None, pred=None) == 0 and fwd(cap=0, heat=None, pts=None, count=None, pred=None) == 0
    assert fwd(B=0, p=4, heat=None) == INVALID
    assert fwd(heat=None) == INVALID and fwd(pts=None) == INVALID and fwd(count=None) == INVALID and fwd(pred=None) == INVALID
    assert bwd(B=0, heat=None, pts=None, count=None, g=None, ws=None, gh=None) == 0
    assert bwd(heat=None) == INVALID and bwd(gh=None) == INVALID and bwd(ws=None) == INVALID and bwd(ws=_addr(8)) == INVALID
    assert bwd(pts=None) == INVALID and bwd(count=None) == INVALID and bwd(g=None) == INVALID
    assert bwd(cap=0, pts=None, count=None, g=None, heat=None) == INVALID          # cap = 0 still writes g_heatmap: needs the rest


def test_sample_desc_and_gather_adjoint_refusals_without_a_launch(dfepe):
    L = dfepe._lib.lib()
    a = _addr()

    def smp(B=2, D=8, H=16, W=24, cap=20, align=1, desc=a, pts=a, count=a, out=a):
        return L.dfepe_sp_sample_desc(desc, pts, None, count, B, D, H, W, cap, align, out, None)

    assert smp(B=-1) == INVALID and smp(D=0) == INVALID and smp(H=0) == INVALID and smp(H=12) == INVALID and smp(W=20) == INVALID
    assert smp(cap=-1) == INVALID and smp(align=2) == INVALID and smp(align=-1) == INVALID
    assert smp(B=0, desc=None, pts=None, count=None, out=None) == 0 and smp(cap=0, desc=None, pts=None, count=None, out=None) == 0
    assert smp(H=BIG, W=BIG) == UNSUPPORTED and smp(B=65536) == UNSUPPORTED
    assert smp(desc=None) == INVALID and smp(pts=None) == INVALID and smp(count=None) == INVALID and smp(out=None) == INVALID

    def gob(B=2, N1=10, N2=12, n_out=30, g=a, m1=a, m2=a, ch=a, g1=a, g2=a):
        return L.dfepe_gather_offsets_bwd(g, B, N1, N2, m1, m2, ch, n_out, g1, g2, None)

    assert gob(B=-1) == INVALID and gob(N1=0) == INVALID and gob(N2=0) == INVALID and gob(n_out=-1) == INVALID
    assert gob(B=0, g=None, m1=None, m2=None, ch=None, g1=None, g2=None) == 0 and gob(B=65536) == UNSUPPORTED
    assert gob(g1=None) == INVALID and gob(g2=None) == INVALID and gob(m1=None) == INVALID and gob(m2=None) == INVALID
    assert gob(g=None) == INVALID and gob(ch=None) == INVALID
    assert gob(n_out=0, g=None, ch=None, g1=None) == INVALID                       # n_out = 0 needs neither, but the outputs


def test_python_layer_refuses_cpu_tensors_and_bad_shapes(dfepe):
    import torch

    ops = dfepe.ops
    with pytest.raises(dfepe.DfepeError):
        ops.sp_flatten(torch.zeros(1, 65, 2, 3))
    with pytest.raises(dfepe.DfepeError):
        ops.sp_nms(torch.zeros(1, 1, 16, 24), 0.015, 4)
    with pytest.raises(dfepe.DfepeError):
        ops.sp_soft_argmax(torch.zeros(1, 1, 16, 24), torch.zeros(1, 4, 2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 5, 4)
    with pytest.raises(dfepe.DfepeError):
        ops.sp_sample_desc(torch.zeros(1, 8, 2, 3), torch.zeros(1, 4, 2, dtype=torch.int32), None, torch.zeros(1, dtype=torch.int32))
    assert ops.sp_nms_capacity(16, 24, 4) == 20
    P = dfepe.compat.superpoint_process.SuperPointNet_process
    sp = P(out_num_points=1000, patch_size=5, nms_dist=4, conf_thresh=0.015)
    assert (sp.out_num_points, sp.patch_size, sp.nms_dist, sp.conf_thresh, sp.border_remove) == (1000, 5, 4, 0.015, 4)
    with pytest.raises(ValueError):
        P(patch_size=4)
    with pytest.raises(ValueError):
        P(patch_size=11, border_remove=4)
    with pytest.raises(NotImplementedError):
        sp.heatmap_to_nms(torch.zeros(1, 1, 16, 24), boxnms=True)
    assert callable(dfepe.compat.train_good_utils.process_SP_output) and callable(dfepe.compat.superpoint_process.flattenDetection)
