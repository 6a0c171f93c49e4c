"""The SuperPoint output processing on the GPU against tests/sp_process_ref.py: the NMS exactly (map, list, confidences, count)
against the sequential nms_fast on every input family, the continuous kernels within the bound the restatement derives (TOL),
the adjoints against float64 autograd and bit-identical on a second run, the gather's gradient, and the whole chain through
compat.get_matches_from_SP against the float64 autograd of the restatement on the same keypoints, matches and choice."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sp_process_cases as sc  # noqa: E402
import sp_process_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV, dtype=dtype)


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_nms(dfepe, heat, d, r, what):
    got = _host(dfepe.ops.sp_nms(_dev(heat), sc.THR, d, r))
    want = sr.nms_batch(heat, sc.THR, d, r)
    assert got["pts"].shape[1] == sr.capacity(heat.shape[2], heat.shape[3], d)
    for key in ("count", "nms_map", "pts", "conf"):
        sc.check(got[key], want[key], f"{what} {key}")
    return got


# ---- NMS ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", sc.BORDERS)
@pytest.mark.parametrize("d", sc.NMS_DISTS)
@pytest.mark.parametrize("shape", sc.SHAPES)
def test_nms_equals_the_sequential_loop_on_every_family(dfepe, shape, d, r):
    names, heat = sc.nms_batch(*shape, r)
    got = _check_nms(dfepe, heat, d, r, f"nms {shape} d={d} r={r}")
    if r == 0:
        assert got["count"][names.index("plateau")] == sr.capacity(*shape, d)     # the list is full, and did not overflow
    assert got["count"][names.index("empty")] == 0


@pytest.mark.parametrize("d", [1, 4])
def test_nms_empty_image_alone_and_among_three(dfepe, d):
    H, W = sc.SHAPES[0]
    fam = sc.nms_families(H, W, 4)
    _check_nms(dfepe, fam["empty"][None, None], d, 4, "nms empty alone")
    _check_nms(dfepe, np.stack((fam["random"], fam["empty"], fam["plateau"]))[:, None], d, 4, "nms empty among three")


@pytest.mark.parametrize("d", [1, 4])
def test_nms_above_the_lds_size_keeps_its_state_in_the_workspace(dfepe, d):
    H, W = sc.BIG_SHAPE
    assert H * W > dfepe._lib.SP_LDS_PIXELS and dfepe._lib.lib().dfepe_sp_nms_workspace_bytes(1, H, W) > 0
    fam = sc.nms_families(H, W, 4)
    heat = np.stack([fam[k] for k in ("random", "plateau", "quantised", "ramp_diag", "nan", "empty")])[:, None]
    _check_nms(dfepe, heat, d, 4, f"nms workspace path d={d}")


# ---- flattenDetection ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", sc.SHAPES)
def test_flatten_forward_and_backward(dfepe, shape, B):
    Hc, Wc = shape[0] // 8, shape[1] // 8
    semi = sc.flatten_semi(B, Hc, Wc)
    g = np.random.default_rng(4).standard_normal((B, 1, *shape)).astype(np.float32)
    t = _dev(semi).requires_grad_(True)
    heat = dfepe.ops.sp_flatten(t)
    heat.backward(_dev(g))
    t64 = torch.from_numpy(semi).double().requires_grad_(True)
    w = sr.flatten_torch(t64)
    (w * torch.from_numpy(g).double()).sum().backward()
    sc.check(heat.detach().cpu().numpy(), sr.flatten(semi), f"flatten {shape} B={B}", sr.TOL(sr.flatten(semi)))
    sc.check(t.grad.cpu().numpy(), t64.grad.numpy(), f"flatten adjoint {shape} B={B}", sr.TOL(t64.grad.numpy()))
    gs = t.grad.cpu().numpy()
    assert (gs[np.isnan(semi)] == 0).all()                                          # NaN -> 0 is a constant
    assert np.abs(gs[:, 64]).max() > 0                                              # the dustbin receives its share
    hh = heat.detach().cpu().numpy()
    assert hh[-1, 0, -8:, -8:].max() < 1e-15 and abs(hh[-1, 0, 0, 7] - 1.0) < 1e-6  # the dominating dustbin; no overflow


# ---- pred_soft_argmax ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("p,d", [(3, 4), (5, 4), (9, 4), (5, 1), (9, 0)])
@pytest.mark.parametrize("shape", sc.SHAPES[1:])
def test_soft_argmax_forward_and_backward(dfepe, shape, p, d, B):
    """d < p: patches overlap, several points send to one pixel."""
    heat = sc.heat_for_patches(B, *shape)
    lst = sr.nms_batch(heat, sc.THR, d, 4)
    assert lst["count"].min() > 0
    pts, cnt = _dev(lst["pts"]), _dev(lst["count"])
    g = np.random.default_rng(p).standard_normal(lst["pts"].shape).astype(np.float32)
    h = _dev(heat).requires_grad_(True)
    pred, patches = dfepe.ops.sp_soft_argmax(h, pts, cnt, p, 4, want_patches=True)
    pred.backward(_dev(g))
    first = h.grad.clone()
    h.grad = None
    dfepe.ops.sp_soft_argmax(h, pts, cnt, p, 4).backward(_dev(g))
    assert torch.equal(first.view(torch.int32), h.grad.view(torch.int32))           # a gather: the same bits on every run
    wpred, wpatch = sr.soft_argmax(heat, lst["pts"], lst["count"], p)
    sc.check(pred.detach().cpu().numpy(), wpred, f"soft-argmax {shape} p={p} d={d}", sr.TOL(wpred))
    sc.check(patches.cpu().numpy(), wpatch, f"patches {shape} p={p} d={d}", sr.TOL(wpatch))
    h64 = torch.from_numpy(heat).double().requires_grad_(True)
    (sr.soft_argmax_torch(h64, lst["pts"], lst["count"], p) * torch.from_numpy(g).double()).sum().backward()
    sc.check(first.cpu().numpy(), h64.grad.numpy(), f"soft-argmax adjoint {shape} p={p} d={d}", sr.TOL(h64.grad.numpy()))
    assert not patches.requires_grad


@pytest.mark.parametrize("p", [3, 5, 9])
def test_soft_argmax_flat_zero_and_dead_patches(dfepe, p):
    H, W = sc.SHAPES[0]
    heat = np.zeros((1, 1, H, W), np.float32)
    heat[0, 0, 3:14, 0:12] = 0.25                                                   # flat around (6, 8)
    heat[0, 0, 8, 18] = 0.5                                                         # one peak among zeros at (18, 8)
    pts = np.array([[[6, 8], [18, 8], [14, 5], [0, 0]]], np.int32)                  # (14, 5): part of the plateau's edge; 4th not listed
    cnt = np.array([3], np.int32)                                                   # p < 9: the third patch is dead (sum 0): offset 0, no gradient
    h = _dev(heat).requires_grad_(True)
    pred = dfepe.ops.sp_soft_argmax(h, _dev(pts), _dev(cnt), p, 4)
    pred.sum().backward()
    got = pred.detach().cpu().numpy()
    want, _ = sr.soft_argmax(heat, pts, cnt, p)
    sc.check(got, want, f"soft-argmax edge patches p={p}", sr.TOL(want))
    np.testing.assert_allclose(got[0, 0], -(p // 2) * 1e-6 / (p * p + 1e-6), rtol=1e-5)   # flat: 0 up to the epsilon terms
    assert abs(got[0, 1]).max() < 1e-5 and (got[0, 3] == 0).all() and (p == 9 or (got[0, 2] == 0).all())
    h64 = torch.from_numpy(heat).double().requires_grad_(True)
    sr.soft_argmax_torch(h64, pts, cnt, p).sum().backward()
    sc.check(h.grad.cpu().numpy(), h64.grad.numpy(), f"soft-argmax edge adjoint p={p}", sr.TOL(h64.grad.numpy()))
    assert torch.isfinite(h.grad).all()


# ---- sample_desc_from_points ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("align", [True, False])
@pytest.mark.parametrize("D", [8, 256])
@pytest.mark.parametrize("B,shape", [(1, sc.SHAPES[0]), (3, sc.SHAPES[2])])
def test_sample_desc(dfepe, B, shape, D, align):
    H, W = shape
    Hc, Wc = H // 8, W // 8
    rng = np.random.default_rng(D + B)
    desc = rng.standard_normal((B, D, Hc, Wc)).astype(np.float32)
    desc[0, :, 0, 0] = 0.0
    desc[-1, 3, 1, 1] = np.nan                                                      # read as 0
    n = 12
    pts = np.stack((rng.integers(0, W, (B, n)), rng.integers(0, H, (B, n))), -1).astype(np.int32)
    pred = (rng.random((B, n, 2)) * 4 - 2).astype(np.float32)
    pts[:, 0], pred[:, 0] = (4, 4), 0.0                                             # a cell centre (align_corners = 0)
    pts[:, 1], pred[:, 1] = (W - 1, H - 1), 0.0                                     # the last row and column
    pts[:, 2], pred[:, 2] = (W - 2, 3), (100.0, 0.0)                                # pushed outside: zero padding, zero norm
    pts[:, 3], pred[:, 3] = (3, H - 2), (0.0, 9.5)                                  # half outside
    pts[:, 4], pred[:, 4] = (0, 0), (-4.0, -4.0) if not align else (0.0, 0.0)       # the zeroed cell alone: zero norm
    cnt = np.full(B, n, np.int32)
    cnt[-1] = n - 3
    got = dfepe.ops.sp_sample_desc(_dev(desc), _dev(pts), _dev(pred), _dev(cnt), align).cpu().numpy()
    want = sr.sample_desc(desc, pts, pred, cnt, align)
    sc.check(got, want, f"sample_desc {shape} D={D} align={align}", sr.TOL(want))
    assert (got[:, 2] == 0).all() and (got[0, 4] == 0).all() and (got[-1, n - 3:] == 0).all()
    np.testing.assert_allclose(np.linalg.norm(got[0, 5:n - 3], axis=1), 1.0, atol=1e-6)
    nopred = dfepe.ops.sp_sample_desc(_dev(desc), _dev(pts), None, _dev(cnt), align).cpu().numpy()
    want = sr.sample_desc(desc, pts, None, cnt, align)
    sc.check(nopred, want, "sample_desc without offsets", sr.TOL(want))


# ---- the gather's gradient -----------------------------------------------------------------------------------------------------
def test_gather_offsets_gradient_and_unchanged_forward(dfepe):
    rng = np.random.default_rng(6)
    B, N1, N2, n_out, cnt = 3, 300, 280, 1100, 40                                   # more rows than one tile of the adjoint holds
    m1 = np.stack([rng.permutation(N1) for _ in range(B)]).astype(np.int32)
    m2 = rng.integers(0, N2, (B, N1)).astype(np.int32)
    choice = rng.integers(0, cnt, (B, n_out)).astype(np.int32)                      # repeats; most keypoints unused
    choice[0, :] = 7                                                                # every row names one keypoint
    p1, p2 = rng.random((B, N1, 2)).astype(np.float32), rng.random((B, N2, 2)).astype(np.float32)
    o1, o2 = rng.standard_normal((B, N1, 2)).astype(np.float32), rng.standard_normal((B, N2, 2)).astype(np.float32)
    score = rng.random((B, N1)).astype(np.float32)
    g = rng.standard_normal((B, n_out, 4)).astype(np.float32)
    args = lambda a, b: (_dev(p1), _dev(p2), a, b, _dev(m1), _dev(m2), _dev(score), _dev(choice))  # noqa: E731
    plain = dfepe.ops.gather_matches(*args(_dev(o1), _dev(o2)))
    a, b = _dev(o1).requires_grad_(True), _dev(o2).requires_grad_(True)
    xs, offs, q = dfepe.ops.gather_matches(*args(a, b))
    for u, v in zip(plain, (xs, offs, q)):
        assert torch.equal(u.view(torch.int32), v.detach().view(torch.int32))       # the forward is the same launch
    assert offs.requires_grad and not xs.requires_grad and not q.requires_grad
    offs.backward(_dev(g))
    w1, w2 = sr.gather_offsets_bwd(g, m1, m2, choice, N1, N2)
    assert ((a.grad.cpu().numpy() != 0) == (w1 != 0)).all() and ((b.grad.cpu().numpy() != 0) == (w2 != 0)).all()
    # the sum of up to n_out fp32 values in fp64 (exact to 2^-53 n_out of the sum of magnitudes), rounded once
    mag1, mag2 = sr.gather_offsets_bwd(np.abs(g), m1, m2, choice, N1, N2)
    sc.check(a.grad.cpu().numpy(), w1, "gather adjoint off1", 2.0 ** -24 * np.abs(w1) + 2.0 ** -53 * n_out * mag1 + 1e-300)
    sc.check(b.grad.cpu().numpy(), w2, "gather adjoint off2", 2.0 ** -24 * np.abs(w2) + 2.0 ** -53 * n_out * mag2 + 1e-300)
    first = a.grad.clone()
    a.grad = None
    dfepe.ops.gather_matches(*args(a, b))[1].backward(_dev(g))
    assert torch.equal(first.view(torch.int32), a.grad.view(torch.int32))


# ---- the compat processor ------------------------------------------------------------------------------------------------------
def test_processor_takes_its_own_map_or_any_other(dfepe):
    """The point list behind a dense map: the one heatmap_to_nms kept, or (a copy, a map from elsewhere) the map's own non-zero
    pixels in row-major order; both give the same offsets, points and descriptors."""
    H, W = sc.SHAPES[1]
    heat = sc.heat_for_patches(2, H, W)
    h = _dev(heat)
    sp = dfepe.compat.superpoint_process.SuperPointNet_process(out_num_points=8, patch_size=5, nms_dist=4, conf_thresh=sc.THR)
    want = sr.nms_batch(heat, sc.THR, 4, 4)
    np.testing.assert_array_equal(sp.heatmap_to_nms(h), want["nms_map"])            # tensor=False: a numpy array
    m = sp.heatmap_to_nms(h, tensor=True)
    a = sp.pred_soft_argmax(m, h)["pred"]
    b = sp.pred_soft_argmax(m.clone(), h)["pred"]
    assert a.shape[1] == sr.capacity(H, W, 4) and b.shape[1] == H * W
    for img in range(2):
        n = int(want["count"][img])
        assert torch.equal(a[img, :n], b[img, :n]) and (b[img, n:] == 0).all() and float(a[img, :n].abs().max()) > 0
    desc = torch.randn(2, 32, H // 8, W // 8, device=DEV)
    np.random.seed(3)
    o1 = sp.batch_extract_features(desc, m, a)
    np.random.seed(3)
    o2 = sp.batch_extract_features(desc, m.clone(), b)
    for key in ("pts_int", "pts_offset", "pts_desc"):
        assert torch.equal(o1[key], o2[key]), key
    assert o1["pts_int"].shape == (2, 8, 2) and o1["pts_offset"].shape == (2, 8, 2) and o1["pts_desc"].shape == (2, 8, 32)
    one = sp.sample_desc_from_points(desc[:1], o1["pts_int"][0] + o1["pts_offset"][0])
    # here pts + offset is a rounded float32 sum (off by <= 2^-24 * 32 px = 2.4e-7 cells), the kernel adds the two in fp64: a
    # bilinear sample of values |v| < 6 moves by < 4 * 6 * 2.4e-7 = 6e-6, and the norms of these samples are above 1
    assert float((one - o1["pts_desc"][0]).abs().max()) < 1e-4


# ---- the chain -------------------------------------------------------------------------------------------------------------
def _twin_grad(semi, lists, picks, weights, dtype):
    """The restatement's autograd on fixed keypoints (lists), fixed rows (picks) and fixed weights: d sum(w offsets) / d semi."""
    grads, offs = [], []
    for s in range(2):
        t = torch.from_numpy(semi[s]).to(dtype).requires_grad_(True)
        res = sr.soft_argmax_torch(sr.flatten_torch(t), lists[s]["pts"], lists[s]["count"], 5)
        B = res.shape[0]
        o = res[torch.arange(B)[:, None], torch.from_numpy(picks[s])]
        (o * torch.from_numpy(weights[:, :, 2 * s:2 * s + 2]).to(dtype)).sum().backward()
        grads.append(t.grad.double().numpy())
        offs.append(o.detach().double().numpy())
    return grads, offs


def test_the_chain_carries_the_offsets_gradient_to_semi(dfepe):
    C = dfepe.compat
    B, (H, W), D, n_sp, n_out = 2, sc.SHAPES[2], 256, 24, 16
    Hc, Wc = H // 8, W // 8
    rng = np.random.default_rng(12)
    semi1 = sc.rand_semi(B, Hc, Wc, 21)
    semi = [semi1, (semi1 + 0.02 * rng.standard_normal(semi1.shape)).astype(np.float32)]
    desc1 = rng.standard_normal((B, D, Hc, Wc)).astype(np.float32)
    desc = [desc1, (desc1 + 0.02 * rng.standard_normal(desc1.shape)).astype(np.float32)]
    leaves = [{"semi": _dev(semi[s]).requires_grad_(True), "desc": _dev(desc[s]).requires_grad_(True)} for s in range(2)]
    feed = iter(leaves)
    sp = C.superpoint_process.SuperPointNet_process(out_num_points=n_sp, patch_size=5, nms_dist=4, conf_thresh=sc.THR)
    tracker = C.model_wrap.PointTracker(max_length=2, nn_thresh=1.0)
    np.random.seed(7)
    imgs = [torch.zeros(B, H, W), torch.zeros(B, H, W)]
    r = C.train_good_utils.get_matches_from_SP(imgs, lambda img: dict(next(feed)), sp, tracker, out_num_points=n_out,
                                               process_SP_output=C.train_good_utils.process_SP_output)
    assert set(r) == {"xs", "offsets", "quality", "num_matches", "xs_SP"}
    assert r["xs"].shape == (B, n_out, 4) and r["offsets"].shape == (B, n_out, 4) and r["quality"].shape == (B, n_out, 1)
    assert r["num_matches"].shape == (B,) and len(r["xs_SP"]) == 2 and r["xs_SP"][0].shape == (B, n_sp, 2)
    assert int(r["num_matches"].min()) > 0
    weights = rng.standard_normal((B, n_out, 4)).astype(np.float32)
    ((r["xs"] + r["offsets"]) * _dev(weights)).sum().backward()
    # the same keypoints (the lists of the same heatmaps), the same matches and choice (the rows that xs names)
    xs = r["xs"].detach().cpu().numpy()
    lists, picks = [], []
    for s in range(2):
        lst = _host(dfepe.ops.sp_nms(dfepe.ops.sp_flatten(leaves[s]["semi"].detach()), sc.THR, 4, 4))
        pick = np.zeros((B, n_out), np.int64)
        for b in range(B):
            listed = lst["pts"][b, :lst["count"][b]]
            for t in range(n_out):
                hit = np.flatnonzero((listed == xs[b, t, 2 * s:2 * s + 2].astype(np.int32)).all(1))
                assert len(hit) == 1
                pick[b, t] = hit[0]
        lists.append(lst)
        picks.append(pick)
    g64, o64 = _twin_grad(semi, lists, picks, weights, torch.float64)
    g32, o32 = _twin_grad(semi, lists, picks, weights, torch.float32)
    offsets = r["offsets"].detach().cpu().numpy()
    for s in range(2):
        got = leaves[s]["semi"].grad
        assert got is not None and float(got.abs().max()) > 0 and leaves[s]["desc"].grad is None
        # no bound can be derived across the fp32 heatmap: allow 4x what torch's own float32 evaluation loses
        tol_g, tol_o = 4 * np.abs(g32[s] - g64[s]).max(), 4 * np.abs(o32[s] - o64[s]).max()
        print(f"chain image {s}: float32 torch is {tol_g / 4:.3e} (gradient, scale {np.abs(g64[s]).max():.3e}) and {tol_o / 4:.3e} (offsets) from float64")
        sc.check(offsets[:, :, 2 * s:2 * s + 2], o64[s], f"chain offsets image {s}", np.full(o64[s].shape, tol_o))
        sc.check(got.cpu().numpy(), g64[s], f"chain semi.grad image {s}", np.full(g64[s].shape, tol_g))
