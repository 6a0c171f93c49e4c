"""dfepe_triangulate, dfepe_two_view_structure and dfepe_reproject on the device: every family of tests/triangulate_cases.py through
the same check() the host build of the header passes (tests/test_triangulate_ref_cpu.py), the exact relations of the contract bit
for bit, consistency with the cheirality and in-front kernels, launch edges, guard elements, graph capture and the compat
wrappers.  The restatements are computed once per process and shared."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cheirality_ref as cref  # noqa: E402
import triangulate_cases as C  # noqa: E402
import triangulate_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POSE = C.POSE_FAMILIES
ALL = C.REGULAR + C.DEGENERATE


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()} if isinstance(d, dict) else d.cpu().numpy()


def _stack(names, key):
    return _dev(np.stack([C.family(n)[key] for n in names]))


def _same(a, b):
    return np.array_equal(_np(a), _np(b), equal_nan=True)


@pytest.fixture(scope="module")
def batch(dfepe):
    """Every pose family as one pair of one batch, and the three entry points run once on it."""
    m, K, Rt, Rt_cam, Xw = (_stack(POSE, k) for k in ("m", "K", "Rt", "Rt_cam", "Xw"))
    ops = dfepe.ops
    out = {"m": m, "K": K, "Rt": Rt, "Rt_cam": Rt_cam, "Xw": Xw,
           "scene": ops.two_view_structure(Rt, K, m, camera_motion=False),
           "cam": ops.two_view_structure(Rt_cam, K, m, camera_motion=True),
           "tri": ops.triangulate(_stack(ALL, "P1"), _stack(ALL, "P2"), _stack(ALL, "m")),
           "rp1": ops.reproject(Xw, _dev(C.IDENTITY_RT), K, C.W, C.H),
           "rp2": ops.reproject(Xw, Rt, K, C.W, C.H),
           "rp2_cam": ops.reproject(Xw, Rt_cam, K, C.W, C.H, camera_motion=True)}
    torch.cuda.synchronize()
    return out


def test_every_family_through_check(batch):
    tri = _np(batch["tri"])
    for i, name in enumerate(ALL):
        fr = {"Xh": C.check("Xh", tri[i], C.ref_triangulate(name), name, "device")}
        if name in POSE:
            b = POSE.index(name)
            pick = lambda d: {k: v[b] for k, v in _np(d).items()}
            fr["structure"] = C.check("structure", pick(batch["scene"]), C.ref_structure(name), name, "device")
            fr["structure_cam"] = C.check("structure", pick(batch["cam"]), C.ref_structure(name, True), name, "device_cam")
            fr["reproject1"] = C.check("reproject", pick(batch["rp1"]), C.ref_reproject(name, 1), name, "device")
            fr["reproject2"] = C.check("reproject", pick(batch["rp2"]), C.ref_reproject(name, 2), name, "device")
            fr["reproject_cam"] = C.check("reproject", pick(batch["rp2_cam"]), C.ref_reproject(name, 2, True), name, "device_cam")
        print(f"device, {name}: " + ", ".join(f"{k} {v:.2g}" for k, v in fr.items()))


def test_structure_and_triangulate_are_the_same_lane_code(dfepe):
    """two_view_structure has no Xh output, so the identity is stated on what both write: on integer_pixels K [R | t] is exact in
    fp32, ops.triangulate gets the very cameras two_view_structure forms, and X = Xh[:3] / w holds up to the three fp32 roundings
    involved (Xh_i, w, X_i: 3 x 2^-24 relative, asserted at 2^-22); the depths follow from X the same way."""
    f = C.family("integer_pixels")
    K64, Rt64 = f["K"].astype(np.float64), f["Rt"].astype(np.float64)
    assert np.array_equal(f["P2"].astype(np.float64), K64 @ Rt64)  # exact: no rounding between the two entry points' cameras
    m = _dev(f["m"][None])
    Xh = dfepe.ops.triangulate(_dev(f["P1"]), _dev(f["P2"]), m)[0].cpu().numpy().astype(np.float64)
    s = _np(dfepe.ops.two_view_structure(_dev(f["Rt"][None]), _dev(f["K"][None]), m, camera_motion=False))
    X = Xh[:, :3] / Xh[:, 3:4]
    h = C.held(C.ref_structure("integer_pixels"))
    assert (np.abs(s["X"][0] - X) <= 2.0 ** -22 * np.abs(X))[h].all()
    assert np.array_equal(s["z1"][0], s["X"][0][:, 2])


def test_exact_relations_bit_for_bit(dfepe, batch):
    ops = dfepe.ops
    P1, P2, m = _stack(ALL, "P1"), _stack(ALL, "P2"), _stack(ALL, "m")
    for k in (20, -20):  # scaling both cameras by a power of two changes no bit
        assert _same(ops.triangulate(P1 * 2.0 ** k, P2 * 2.0 ** k, m), batch["tri"]), k
    one = ALL.index("forward")
    b1 = ops.triangulate(P1[one], P2[one], m)                                   # stride 0 ...
    b2 = ops.triangulate(P1[one].expand(len(ALL), 3, 4), P2[one].expand(len(ALL), 3, 4), m)  # ... against the broadcast batch
    assert _same(b1, b2) and _same(ops.triangulate(P1[one], P2, m), ops.triangulate(P1[one].expand(len(ALL), 3, 4), P2, m))
    Xw, K, Rt = batch["Xw"], batch["K"], batch["Rt"]
    r0 = ops.reproject(Xw, Rt[0], K[0], C.W, C.H)
    assert all(_same(r0[k], v) for k, v in ops.reproject(Xw, Rt[0].expand(len(POSE), 3, 4), K[0].expand(len(POSE), 3, 3), C.W, C.H).items())
    for want in (("X",), ("z1",), ("z2",), ("X", "z2"), ("z1", "z2"), ("X", "z1")):  # any subset of the nullable outputs
        sub = ops.two_view_structure(batch["Rt_cam"], K, batch["m"], want=want)
        assert tuple(sub) == want and all(_same(sub[k], batch["cam"][k]) for k in want), want
    zeros = torch.zeros(len(POSE), dtype=torch.int32, device=DEV)
    assert all(_same(v, batch["cam"][k]) for k, v in ops.two_view_structure(batch["Rt_cam"], K, batch["m"], winner=zeros).items())
    ones = torch.ones(len(POSE), device=DEV)
    assert all(_same(v, batch["cam"][k]) for k, v in ops.two_view_structure(batch["Rt_cam"], K, batch["m"], scale=ones).items())


def test_swapped_views_scale_and_clamp_within_the_bounds(dfepe, batch):
    ops = dfepe.ops
    names = [n for n in POSE if C.family(n)["regular"]]
    idx = [POSE.index(n) for n in names]
    m, K, Rt, Rt_cam = batch["m"][idx], batch["K"][idx], batch["Rt"][idx], batch["Rt_cam"][idx]
    # swapped views: the inverse pose on (x2, x1) sees the same points from camera 2; its depths are (z2, z1) of the original
    sw = _np(ops.two_view_structure(Rt_cam, K, m[:, :, [2, 3, 0, 1]].contiguous(), camera_motion=False, want=("z1", "z2")))
    scale = np.float32(7.25) * np.arange(1, len(names) + 1, dtype=np.float32)
    sc = _np(ops.two_view_structure(Rt, K, m, camera_motion=False, scale=_dev(scale), clamp=150.0))
    neg = _np(ops.two_view_structure(Rt, K, m, camera_motion=False, scale=_dev(-scale)))
    for b, name in enumerate(names):
        r = C.ref_structure(name)
        f = C.family(name)
        rs = ref.two_view_structure(f["Rt_cam"], f["K"], f["m"][:, [2, 3, 0, 1]], False)  # the restatement of the swapped problem
        C.check("structure", {k: v[b] for k, v in sw.items()}, rs, name, "device_swapped")
        C.check("structure", {k: v[b] for k, v in sc.items()}, r, name, "device_scaled", scale=scale[b], clamp=150.0)
        C.check("structure", {"X": sc["X"][b]}, r, name, "device_scaled", scale=scale[b])
        C.check("structure", {k: v[b] for k, v in neg.items()}, r, name, "device_scaled", scale=-scale[b])
        assert (np.abs(sc["z1"][b][C.held(r)]) <= 150.0).all() and (np.abs(sc["z2"][b][C.held(r)]) <= 150.0).all()


def _essential(f):
    """E = [t]x R / |t| of a family's scene motion, fp64."""
    R, t = f["Rt"][:, :3].astype(np.float64), f["Rt"][:, 3].astype(np.float64)
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R / np.linalg.norm(t)


@pytest.mark.parametrize("name", ("forward_noise", "outliers"))
def test_depths_agree_with_the_cheirality_and_in_front_kernels(dfepe, name):
    ops = dfepe.ops
    f = C.family(name)
    B, N = 3, 257
    m = _dev(np.stack([f["m"][k * 100:k * 100 + N] for k in range(B)]))
    K = _dev(f["K"][None]).expand(B, 3, 3).contiguous()
    E = _dev(_essential(f).astype(np.float32)[None]).expand(B, 3, 3).contiguous()
    Rt_cam, winner, counts = ops.cheirality(E, K, m, 50.0)
    mask = ops.ransac_in_front(E, K, m, winner, 50.0).cpu().numpy() > 0
    s = _np(ops.two_view_structure(Rt_cam, K, m, camera_motion=True, winner=winner, want=("z1", "z2")))
    with np.errstate(invalid="ignore"):
        mine = (s["z1"] > 0) & (s["z1"] < 50) & (s["z2"] > 0) & (s["z2"] < 50)
    win, cnt = winner.cpu().numpy(), counts.cpu().numpy()
    assert (win >= 0).all()
    for b in range(B):
        und = cref.reference(E[b].cpu().numpy(), K[b].cpu().numpy(), m[b].cpu().numpy(), 50.0)["undecided"][win[b]]
        assert np.array_equal(mine[b][~und], mask[b][~und]), (name, b)
        assert mask[b].sum() == cnt[b, win[b]]
        print(f"{name} pair {b}: {mask[b].sum()} in front, {und.sum()} undecided, {(mine[b] != mask[b]).sum()} differ")


def _edge_inputs(B, N):
    """B distinct pairs of N correspondences assembled from the regular pose families' cached points."""
    names = ("forward", "outliers", "short_baseline")[:B]
    return names, {k: _dev(np.stack([C.family(n)[k][:N] if k in ("m", "Xw") else C.family(n)[k] for n in names]))
                   for k in ("m", "Xw", "K", "Rt", "P1", "P2")}


def test_launch_edges_guards_and_neighbours(dfepe):
    """N in {1, 63, 64, 65, 255, 256, 257} x B in {1, 2, 3} through the C ABI with 64 guard elements after every output."""
    L = dfepe._lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    G, MARK = 64, 12345.0
    full = {n: (C.ref_triangulate(n), C.ref_structure(n), C.ref_reproject(n, 2)) for n in ("forward", "outliers", "short_baseline")}
    for B in (1, 2, 3):
        for N in (1, 63, 64, 65, 255, 256, 257):
            names, t = _edge_inputs(B, N)
            buf = {k: torch.full((B * N * w + G,), MARK, device=DEV) for k, w in (("Xh", 4), ("X", 3), ("z1", 1), ("z2", 1), ("x", 2), ("z", 1))}
            ins = torch.full((B * N + G,), 77, device=DEV, dtype=torch.uint8)
            p = lambda a: a.data_ptr()
            assert L.dfepe_triangulate(p(t["P1"]), 12, p(t["P2"]), 12, p(t["m"]), B, N, p(buf["Xh"]), stream) == 0
            assert L.dfepe_two_view_structure(p(t["Rt"]), 0, p(t["K"]), p(t["m"]), B, N, None, None, 0.0, p(buf["X"]), p(buf["z1"]), p(buf["z2"]), stream) == 0
            assert L.dfepe_reproject(p(t["Xw"]), p(t["Rt"]), 12, 0, p(t["K"]), 9, B, N, C.W, C.H, p(buf["x"]), p(buf["z"]), p(ins), stream) == 0
            torch.cuda.synchronize()
            for k, v in buf.items():
                assert (v[-G:] == MARK).all(), (k, B, N)
            assert (ins[-G:] == 77).all()
            o = {k: v[:-G].cpu().numpy() for k, v in buf.items()}
            inside = ins[:-G].cpu().numpy().reshape(B, N)
            for b, name in enumerate(names):
                (Xr, eta), rs, rr = full[name]
                cut = lambda d: {k: (v[:N] if isinstance(v, np.ndarray) else v) for k, v in d.items()}
                C.check("Xh", o["Xh"].reshape(B, N, 4)[b], (Xr[:N], eta[:N]), name, "device_edges")
                C.check("structure", {"X": o["X"].reshape(B, N, 3)[b], "z1": o["z1"].reshape(B, N)[b], "z2": o["z2"].reshape(B, N)[b]},
                        cut(rs), name, "device_edges", regular=N >= 100)  # the 1 % cap needs a population; below, rows are only screened for NaN
                if N < 100:  # ... and every held point is still bounded
                    h = C.held(cut(rs))
                    bd = C.structure_bounds(cut(rs))
                    assert (np.abs(o["z1"].reshape(B, N)[b] - rs["z1"][:N]) <= bd["z1"])[h].all()
                C.check("reproject", {"x": o["x"].reshape(B, N, 2)[b], "z": o["z"].reshape(B, N)[b], "inside": inside[b]}, cut(rr), name, "device_edges")


def test_nan_rows_and_a_pair_without_a_pose_touch_only_their_own_rows(dfepe, batch):
    i_nan, i_fwd = POSE.index("nan_rows"), POSE.index("forward")
    bad = sorted({r for r, _, _ in C.NAN_ROWS})
    good = np.setdiff1d(np.arange(C.N), bad)
    for d in (batch["scene"], batch["cam"]):
        for k, v in _np(d).items():
            assert np.isnan(v[i_nan][bad]).all() and np.array_equal(v[i_nan][good], v[i_fwd][good]), k
    tri = _np(batch["tri"])
    assert np.isnan(tri[ALL.index("nan_rows")][bad]).all() and np.array_equal(tri[ALL.index("nan_rows")][good], tri[ALL.index("forward")][good])
    # a pair with winner = -1 between two good pairs
    idx = [POSE.index(n) for n in ("forward", "sideways", "far")]
    win = torch.tensor([0, -1, 2], dtype=torch.int32, device=DEV)
    out = _np(dfepe.ops.two_view_structure(batch["Rt_cam"][idx], batch["K"][idx], batch["m"][idx], winner=win))
    for k, v in out.items():
        assert np.isnan(v[1]).all() and np.array_equal(v[0], _np(batch["cam"])[k][idx[0]]) and np.array_equal(v[2], _np(batch["cam"])[k][idx[2]]), k


def test_round_trip_into_both_images(dfepe, batch):
    for name in ("forward", "sideways"):
        b = POSE.index(name)
        X = batch["scene"]["X"][b:b + 1]
        h = C.held(C.ref_structure(name))
        for view in (1, 2):
            Rt = _dev(C.IDENTITY_RT) if view == 1 else batch["Rt"][b]
            x = dfepe.ops.reproject(X, Rt, batch["K"][b], C.W, C.H)["x"][0].cpu().numpy().astype(np.float64)
            d = np.abs(x - C.family(name)["m"][:, 2 * view - 2:2 * view].astype(np.float64))
            bound = C.round_trip_bound(name, view)
            print(f"round trip, {name} view {view}: max {d[h].max():.3g} px, {(d / bound)[h].max():.3g} of the bound")
            assert (d <= bound)[h].all()


def test_capture_replays_bit_equal_to_eager(dfepe, batch):
    ops = dfepe.ops
    win = torch.zeros(len(POSE), dtype=torch.int32, device=DEV)
    scale = torch.full((len(POSE),), 2.5, device=DEV)
    run = lambda: (ops.two_view_structure(batch["Rt_cam"], batch["K"], batch["m"], winner=win, scale=scale, clamp=150.0),
                   ops.reproject(batch["Xw"], batch["Rt"], batch["K"], C.W, C.H))
    eager = run()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    graph.replay()
    torch.cuda.synchronize()
    for e, c in zip(eager, captured):
        for k, v in e.items():
            assert _same(v, c[k]), k


def test_compat_wrappers(dfepe):
    comp = dfepe.compat
    f = C.family("forward_noise")
    # get_depth: shape, and bit-equal to two_view_structure on its own intermediate pose
    B, N = 2, 250
    K64 = f["K"].astype(np.float64)
    F_gt = np.linalg.inv(K64).T @ _essential(f) @ np.linalg.inv(K64)  # x2^T F x1 = 0
    data = {"Ks": _dev(f["K"][None]).expand(B, 3, 3).contiguous(), "matches_xy_ori": _dev(np.stack((f["m"][:N], f["m"][N:2 * N])))}
    net = comp.DeepFNet.DeepFNet(depth=2, image_size=[376, 1241, 3], if_quality=False).to(DEV)
    T = net._T_hw(B, torch.device(DEV))
    Ti = np.linalg.inv(T[0].cpu().numpy().astype(np.float64))
    F_out = _dev((Ti.T @ F_gt @ Ti / np.abs(Ti.T @ F_gt @ Ti).max()).astype(np.float32)[None]).expand(B, 3, 3).contiguous()  # T^T F_out T ~ F_gt
    depth = net.get_depth(data, F_out, T, T)
    assert depth.shape == (B, 1, N) and depth.dtype == torch.float32 and depth.is_cuda
    Rt_cam, winner, K, m = net._depth_pose(data, F_out, T, T)
    assert torch.equal(depth[:, 0], dfepe.ops.two_view_structure(Rt_cam, K, m, camera_motion=True, winner=winner, want=("z1",))["z1"])
    assert (winner >= 0).all() and (depth[:, 0] > 0).float().mean() > 0.9
    # distinct T1, T2 objects take the general T2^T F T1 product (fp32 matmul): the same pose up to that product's rounding, so
    # the same depths up to the depth's own sensitivity to the pose (unbounded next to the epipole: the median is compared)
    other = net.get_depth(data, F_out, T, T.clone())
    near = (depth > 1) & (depth < 100)
    assert other.shape == depth.shape and near.float().mean() > 0.8
    assert ((other - depth).abs()[near] / depth[near]).median() <= 1e-3
    # triangulatePoints: cv2's layout and dtype, the kernel's values
    Xh = comp.utils_opencv.triangulatePoints(f["P1"].astype(np.float64), f["P2"], f["m"][:, :2].T, f["m"][:, 2:].T.astype(np.float64))
    assert Xh.shape == (4, C.N) and Xh.dtype == np.float32 and (Xh[3] >= 0).all()
    C.check("Xh", Xh.T, C.ref_triangulate("forward_noise"), "forward_noise", "device_compat")
    # reproj_and_scatter: within() of its own x1, and the restatement
    val, x1 = comp.utils_vis.reproj_and_scatter(f["Rt"], f["Xw"], None, visualize=False, param_list=[f["K"], (int(C.H), int(C.W))], debug=False)
    assert val.shape == (C.N,) and val.dtype == bool and x1.shape == (C.N, 2)
    assert np.array_equal(val, comp.utils_misc.within(x1[:, 0], x1[:, 1], C.W, C.H))
    C.check("reproject", {"x": x1.astype(np.float32), "inside": val.astype(np.uint8)}, C.ref_reproject("forward_noise", 2), "forward_noise", "device_compat")

    class Loader:
        K, im_shape = f["K"], (int(C.H), int(C.W))

    val2, x2 = comp.utils_vis.reproj_and_scatter(f["Rt"], f["Xw"], None, Loader(), visualize=False)
    assert np.array_equal(val, val2) and np.array_equal(x1, x2)
