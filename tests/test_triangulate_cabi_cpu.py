"""CPU-side checks of the two-view structure entry points: the symbols are exported under the unchanged version, every refusal
the contract lists is decided on the host (null pointers, no launch: safe without a GPU), and the host-side parts of the compat
surface (utils_misc.within, reproj_and_scatter's refusal to draw)."""
import ctypes

import numpy as np
import pytest

OK, INVALID, UNSUPPORTED = 0, -1, -3
A16 = ctypes.c_void_p(4096)       # a 16-byte aligned address that is never dereferenced: every call below is refused on the host
ODD = ctypes.c_void_p(4096 + 4)   # ... and one that is not aligned


def test_symbols_are_exported_and_the_version_is_unchanged(dfepe):
    L = dfepe._lib.lib()
    assert L.dfepe_version() == 154
    for name in ("dfepe_triangulate", "dfepe_two_view_structure", "dfepe_reproject"):
        assert name in dfepe.EXPORTED_SYMBOLS and hasattr(L, name)
    assert dfepe._lib.POSE_CAMERA_MOTION == 1
    assert L.dfepe_strerror(UNSUPPORTED) != L.dfepe_strerror(INVALID)


def test_triangulate_refusals_without_launching(dfepe):
    tri = dfepe._lib.lib().dfepe_triangulate
    call = lambda P1=A16, s1=12, P2=A16, s2=0, m=A16, B=2, N=5, Xh=A16: tri(P1, s1, P2, s2, m, B, N, Xh, None)
    assert call(B=-1) == INVALID and call(N=-1) == INVALID
    assert call(B=0) == OK and call(N=0) == OK and tri(None, 12, None, 12, None, 0, 7, None, None) == OK
    for k in ("P1", "P2", "m", "Xh"):
        assert call(**{k: None}) == INVALID, k
    assert call(m=ODD) == INVALID and call(Xh=ODD) == INVALID
    for bad in (1, 9, 11, 16, -12):
        assert call(s1=bad) == INVALID and call(s2=bad) == INVALID
    assert call(s1=5, B=0) == INVALID                     # a bad stride is refused before the empty batch returns
    assert call(B=65536) == UNSUPPORTED
    assert call(B=65536, P1=None) == INVALID              # null pointers first, like the siblings


def test_two_view_structure_refusals_without_launching(dfepe):
    tvs = dfepe._lib.lib().dfepe_two_view_structure
    call = lambda Rt=A16, flags=1, K=A16, m=A16, B=2, N=5, win=None, sc=None, X=A16, z1=None, z2=None: \
        tvs(Rt, flags, K, m, B, N, win, sc, 0.0, X, z1, z2, None)
    assert call(B=-1) == INVALID and call(N=-1) == INVALID
    assert call(B=0) == OK and call(N=0) == OK
    for k in ("Rt", "K", "m"):
        assert call(**{k: None}) == INVALID, k
    assert call(X=None) == INVALID                        # all three outputs NULL
    assert call(m=ODD) == INVALID
    assert call(flags=2) == INVALID and call(flags=3) == INVALID and call(flags=1 << 31) == INVALID
    assert call(flags=2, B=0) == INVALID
    assert call(B=65536) == UNSUPPORTED and call(B=65536, X=None, z2=A16) == UNSUPPORTED


def test_reproject_refusals_without_launching(dfepe):
    rp = dfepe._lib.lib().dfepe_reproject
    call = lambda X=A16, Rt=A16, rs=12, flags=0, K=A16, ks=9, B=2, M=5, x=A16: rp(X, Rt, rs, flags, K, ks, B, M, 1241.0, 376.0, x, None, None, None)
    assert call(B=-1) == INVALID and call(M=-1) == INVALID
    assert call(B=0) == OK and call(M=0) == OK
    for k in ("X", "Rt", "K", "x"):
        assert call(**{k: None}) == INVALID, k
    for bad in (1, 3, 9, 16):
        assert call(rs=bad) == INVALID
    for bad in (1, 3, 12):
        assert call(ks=bad) == INVALID
    assert call(rs=0, ks=0, B=0) == OK
    assert call(flags=2) == INVALID
    assert call(B=65536) == UNSUPPORTED


def test_ops_refuse_cpu_tensors_and_wrong_shapes(dfepe):
    import torch

    with pytest.raises(dfepe.DfepeError):
        dfepe.ops.triangulate(torch.zeros(3, 4), torch.zeros(3, 4), torch.zeros(1, 5, 4))
    with pytest.raises(dfepe.DfepeError):
        dfepe.ops.two_view_structure(torch.zeros(1, 3, 4), torch.zeros(1, 3, 3), torch.zeros(1, 5, 4))
    with pytest.raises(dfepe.DfepeError):
        dfepe.ops.reproject(torch.zeros(1, 5, 3), torch.zeros(3, 4), torch.zeros(3, 3), 1241.0, 376.0)


def test_within_against_loops(dfepe):
    within = dfepe.compat.utils_misc.within
    g = np.random.default_rng(0)
    x, y = g.uniform(-50, 1300, 400), g.uniform(-50, 420, 400)
    x[:6], y[:6] = (0.0, 1241.0, 1241.0000001, -1e-300, np.nan, 5.0), (0.0, 376.0, 10.0, 10.0, 10.0, np.nan)
    got = within(x, y, 1241, 376)
    assert got.dtype == bool and got.shape == (400,)
    for i in range(400):
        assert got[i] == (x[i] >= 0 and y[i] >= 0 and x[i] <= 1241 and y[i] <= 376), i
    assert list(got[:6]) == [True, True, False, False, False, False]


def test_reproj_and_scatter_refuses_to_draw(dfepe):
    vis = dfepe.compat.utils_vis
    K, shape = np.eye(3), (376, 1241)
    with pytest.raises(NotImplementedError):
        vis.reproj_and_scatter(np.eye(3, 4), np.zeros((4, 3)), None, visualize=True, param_list=[K, shape])
    with pytest.raises(NotImplementedError):  # the reference's default draws
        vis.reproj_and_scatter(np.eye(3, 4), np.zeros((4, 3)), None, param_list=[K, shape])
    val, x1 = vis.reproj_and_scatter(np.eye(3, 4), np.zeros((0, 3)), None, visualize=False, param_list=[K, shape], debug=False)
    assert val.shape == (0,) and val.dtype == bool and x1.shape == (0, 2)
