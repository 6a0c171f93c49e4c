"""The batched five-point RANSAC estimator (csrc/ransac5.hip: ops.ransac_essential / ops.ransac_essential_pose) on the device,
and the validation baseline built on it (compat.utils_opencv.recover_camera_five_point, val_rt_batch / validation_summary with
baseline="five_point").

Every device result goes through one comparison (check_pair), with the count table and the hypotheses returned.  The five-point
solve is too ill-conditioned on KITTI-like pairs for an independent restatement to pin the counts root for root, so the counts are
held to an fp64 Sampson evaluation of the device's OWN hypotheses (hyp_E), the hypotheses to the validity bounds of
tests/test_ransac5_cpu.py, the outputs to the sequential rule (tests/ransac5_ref.py) applied to the device's own table, exactly,
and the winner, the mask and the NaN-masked copy to the winning hypothesis.  The solver's completeness is held to the restatement
where the problem is well conditioned.

The cases sit on the edges of the launches: N = 6 (the minimum) and 7, the 64-lane tails of the sweep, the 256-lane tails of the
sweep's stride and of the mask launch, the LDS attribute of the count launch (16 N + 38592 bytes of LDS exceed 64 KiB, and need
hipFuncSetAttribute, from N = 1685 on: csrc/ransac5.hip, dfepe_ransac_essential), N = 4096 (kMaxN5), the 16-iteration chunks of
the count grid (kChunk5), the 64-iteration windows of the select kernel, 4 pairs per select workgroup (kSelectWaves), 65535 pairs
(kMaxPairs5), and the branches of the rule (confidence 0 and 1, threshold 0, an all-inlier pair, a 64-bit seed)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac5_ref as ref  # noqa: E402
from test_ransac5_cpu import KINDS, KITTI_K, check_valid, complete, kind_points, wide_scene  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAND = 1e-4   # relative band around t^2 inside which a decision may differ from the fp64 evaluation (as test_ransac_gpu.py)
OUT_KEYS = ("E", "mask", "n_inliers", "iters_run", "best_hyp", "masked")


def _bits(x):
    x = x.detach().cpu().contiguous()
    return x.view(torch.uint8) if x.is_floating_point() else x


def _np(out):
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}


def _pairs(dfepe, kinds, N, seed):
    return np.stack([kind_points(dfepe, kd, N, seed * 1000 + i) for i, kd in enumerate(kinds)])


def run(dfepe, m, K, threshold, confidence, max_iters, seed):
    """Device result with the table, the hypotheses and the NaN-masked copy; the same call with the table in the workspace (and no
    hypotheses returned) must give bit-identical outputs."""
    md = torch.from_numpy(np.ascontiguousarray(m)).to(DEV)
    Kd = torch.from_numpy(np.broadcast_to(np.asarray(K, np.float32), (m.shape[0], 3, 3)).copy()).to(DEV)
    kw = dict(threshold=threshold, confidence=confidence, max_iters=max_iters, seed=seed)
    out = dfepe.ops.ransac_essential(md, Kd, want_hyp_counts=True, want_hyp_E=True, want_masked=True, **kw)
    ws = dfepe.ops.ransac_essential(md, Kd, want_masked=True, **kw)
    torch.cuda.synchronize()
    assert ws["hyp_counts"] is None and ws["hyp_E"] is None
    for k in OUT_KEYS:
        assert torch.equal(_bits(out[k]), _bits(ws[k])), k
    return _np(out)


def check_pair(m, K, out, b, threshold, confidence, seed, max_iters):
    """The device result of pair b: hypotheses, counts, selection, winner, mask."""
    pts = m[b]
    N = pts.shape[0]
    q = ref.normalize(pts, K)
    t2 = ref.threshold2(threshold, K)
    tab, hE = out["hyp_counts"][b], out["hyp_E"][b]
    assert tab.shape == (max_iters, 10) and hE.shape == (max_iters, 10, 3, 3) and hE.dtype == np.float64
    assert (tab >= -1).all() and (tab <= N).all()

    # 1. every hypothesis is valid for its sample, and its count is the fp64 Sampson count of that hypothesis up to the
    #    correspondences inside the band (threshold 0: the band is empty and a residual of exactly zero is a matter of the last
    #    bit, so there only the rule is held: whatever the table holds, the outputs follow from it)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(max_iters):
            row = tab[k]
            n = int((row >= 0).sum())
            assert (row[n:] == ref.NO_ROOT).all(), (b, k, row)  # roots first, absent ones after
            assert (hE[k, n:] == 0).all(), (b, k)
            q5 = q[ref.draw_sample(seed, k, N)]
            for r in range(n):
                check_valid(hE[k, r], q5)
                if t2 > 0:
                    e = ref.sampson(hE[k, r], q)
                    band = int((np.abs(e - t2) <= BAND * t2).sum())
                    assert abs(int(row[r]) - int((e <= t2).sum())) <= band, (b, k, r, int(row[r]), int((e <= t2).sum()), band)

    # 2. the rule over the device's own table gives the device's outputs exactly
    nb, dk, dr, it = int(out["n_inliers"][b]), int(out["best_hyp"][b, 0]), int(out["best_hyp"][b, 1]), int(out["iters_run"][b])
    assert ref.select(tab, N, confidence, max_iters) == (nb, dk, dr, it), b

    # 3. the winner is the fp32 rounding of its hypothesis; the mask is that hypothesis' decisions outside the band
    E = out["E"][b]
    mask = out["mask"][b]
    if nb == 0:
        assert (dk, dr) == (-1, -1) and (E == 0).all() and (mask == 0).all(), b
    else:
        assert nb > 4 and 0 <= dk < max_iters and 0 <= dr < 10 and tab[dk, dr] == nb, (b, nb, dk, dr)
        assert np.array_equal(E.view(np.uint32), hE[dk, dr].astype(np.float32).view(np.uint32)), b
        if t2 > 0:
            with np.errstate(divide="ignore", invalid="ignore"):
                e = ref.sampson(hE[dk, dr], q)
            sure = np.abs(e - t2) > BAND * t2
            assert ((mask == 1) == (e <= t2))[sure].all(), b
    assert int(mask.sum()) == nb, b
    masked = out["masked"][b]
    nan_rows = np.isnan(masked).all(-1)
    assert (np.isnan(masked).any(-1) == nan_rows).all(), b
    assert (nan_rows == (mask == 0)).all(), b
    assert np.array_equal(masked[mask == 1].view(np.uint32), pts[mask == 1].view(np.uint32)), b
    return nb, dk, dr, it


def run_and_check(dfepe, m, threshold, confidence, max_iters, seed, K=KITTI_K, pairs=None):
    out = run(dfepe, m, K, threshold, confidence, max_iters, seed)
    return out, [check_pair(m, K, out, b, threshold, confidence, seed, max_iters) for b in (pairs if pairs is not None else range(m.shape[0]))]


# ---- the launch edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [6, 7, 63, 64, 65, 255, 256, 257, 1000, 1684, 1685, 4096])
def test_every_correspondence_count_edge(dfepe, N):
    """40 iterations (two full chunks of the count grid and a partial one) of an outlier pair and a noise pair."""
    m = _pairs(dfepe, [(0.3, 0.5), "noise"], N, 10 + N)
    _, res = run_and_check(dfepe, m, 1.0, 0.999, 40, 2)
    if N >= 63:
        assert res[0][0] > 0.25 * N  # the outlier pair (70 % inliers) found a model that the noise pair cannot have


@pytest.mark.parametrize("max_iters", [1, 15, 16, 17, 63, 64, 65, 1000])
def test_every_iteration_count_edge(dfepe, max_iters):
    """One below / at / above the count kernel's chunk (16) and the select kernel's window (64), one iteration, and 1000."""
    kinds = [(0.6, 0.5), "noise"] if max_iters < 1000 else [(0.6, 0.5)]
    m = _pairs(dfepe, kinds, 100, 20 + max_iters)
    _, res = run_and_check(dfepe, m, 0.5, 0.999, max_iters, 4)
    if max_iters == 1000:
        assert res[0][0] >= 15  # 40 inliers among 100: a model well above what five random points collect


@pytest.mark.parametrize("B", [1, 3, 5])
def test_every_batch_edge(dfepe, B):
    """4 pairs per select workgroup: 5 pairs need a second one."""
    m = _pairs(dfepe, (KINDS * 2)[:B], 100, 30 + B)
    run_and_check(dfepe, m, 0.5, 0.999, 20, 6)


def test_the_largest_batch(dfepe):
    """65535 pairs (the grid's y limit) at N = 6, one iteration: 9 distinct pairs repeated."""
    base = _pairs(dfepe, [(0.0, 0.05)] * 8 + ["noise"], 6, 40)
    m = base[np.arange(65535) % 9]
    out, _ = run_and_check(dfepe, m, 1.0, 0.999, 1, 8, pairs=[0, 8, 9, 32768, 65534])
    for k in OUT_KEYS + ("hyp_counts", "hyp_E"):
        v = out[k]
        ok = np.isnan(v) & np.isnan(v[np.arange(65535) % 9]) if k == "masked" else False
        assert ((v == v[np.arange(65535) % 9]) | ok).all(), k  # a pair's result does not depend on where it sits


@pytest.mark.parametrize("confidence", [0.0, 1.0])
def test_confidence_zero_and_one(dfepe, confidence):
    m = _pairs(dfepe, [(0.3, 0.5), "noise"], 100, 50)
    _, res = run_and_check(dfepe, m, 0.5, confidence, 40, 1)
    if confidence == 1.0:
        assert res[0][3] == 40  # log(DBL_MIN) / log(den): never below 40 with 30 % outliers
    else:
        assert res[0][3] == res[0][1] + 1  # log(1 - 0) = 0: the first model ends the loop


def test_a_64_bit_seed(dfepe):
    m = _pairs(dfepe, [(0.3, 0.5)], 100, 60)
    a, _ = run_and_check(dfepe, m, 0.5, 0.999, 20, 0xFEDCBA9876543210)
    b, _ = run_and_check(dfepe, m, 0.5, 0.999, 20, 0x76543210)  # its low 32 bits alone give another stream
    assert not np.array_equal(a["hyp_counts"], b["hyp_counts"])


def test_threshold_zero(dfepe):
    m = _pairs(dfepe, [(0.0, 0.05), "noise"], 100, 70)
    run_and_check(dfepe, m, 0.0, 0.999, 20, 3)


def test_identity_camera_uses_points_and_threshold_as_given(dfepe):
    m = ref.normalize(_pairs(dfepe, [(0.3, 0.5)], 100, 80)[0], KITTI_K).astype(np.float32)[None]
    _, res = run_and_check(dfepe, m, 1e-3, 0.999, 40, 5, K=np.eye(3))
    assert res[0][0] > 25


def test_an_all_inlier_pair_stops_after_the_first_model(dfepe):
    pts, E_gt = wide_scene(3, n=100)
    out, res = run_and_check(dfepe, pts[None], 1.0, 0.999, 1000, 0)
    assert res[0][0] == 100 and res[0][1] == 0 and res[0][3] == 1  # ep = 0: RANSACUpdateNumIters returns 0
    assert (out["mask"] == 1).all()
    assert np.abs(out["E"][0].ravel() - E_gt).max() < 1e-4


def test_reproducible_and_independent_of_the_batch(dfepe):
    big = torch.from_numpy(_pairs(dfepe, (KINDS * 3)[:9], 500, 90)).to(DEV)
    one = big[6:7].clone()
    K = torch.from_numpy(KITTI_K.astype(np.float32)).to(DEV)
    kw = dict(threshold=0.5, max_iters=100, seed=9, want_hyp_counts=True, want_hyp_E=True, want_masked=True)
    a = dfepe.ops.ransac_essential(big, K.expand(9, 3, 3).contiguous(), **kw)
    b = dfepe.ops.ransac_essential(big, K.expand(9, 3, 3).contiguous(), **kw)
    c = dfepe.ops.ransac_essential(one, K.reshape(1, 3, 3), **kw)
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
        assert torch.equal(_bits(a[k][6]), _bits(c[k][0])), k


@pytest.mark.parametrize("kind", ["wide", "noise"])
def test_the_solver_is_complete_where_the_problem_is_well_conditioned(dfepe, kind):
    """The criterion and the 95 % cap of tests/test_ransac5_cpu.py, on the device's hypotheses of the first 128 iterations."""
    pts = wide_scene(1)[0] if kind == "wide" else kind_points(dfepe, "noise", 200, 11)
    out = run(dfepe, pts[None], KITTI_K, 1.0, 0.999, 128, 5)
    q = ref.normalize(pts, KITTI_K)
    same = 0
    for k in range(128):
        n = int((out["hyp_counts"][0, k] >= 0).sum())
        same += complete(list(out["hyp_E"][0, k, :n]), ref.five_point(q[ref.draw_sample(5, k, 200)]))
    print(f"{kind}: device roots equal to the restatement's {same}/128")
    assert same >= 0.95 * 128


def test_fewer_than_6_correspondences_is_refused(dfepe):
    with pytest.raises(dfepe._lib.DfepeError, match="at least 6"):
        dfepe.ops.ransac_essential(torch.rand(2, 5, 4, device=DEV) * 100, torch.eye(3, device=DEV).expand(2, 3, 3).contiguous())


# ---- end to end -------------------------------------------------------------------------------------------------------------
def _val_inputs(dfepe, B=4, N=1000, seed=41):
    """The scene of _val_inputs in tests/test_ransac_gpu.py."""
    sc = dfepe.synth.make_scene(B, N, seed=seed, outlier_ratio=0.2, noise_px=0.05)
    m = sc["matches_xy_ori"].numpy()
    E_est = sc["E_gt"].numpy() + np.random.default_rng(seed).normal(0, 1e-3, (B, 3, 3)).astype(np.float32)
    return sc, m, E_est


def test_the_pose_of_the_validation_scene(dfepe):
    sc, _, _ = _val_inputs(dfepe)
    dev = {k: v.to(DEV) for k, v in sc.items()}
    out = dfepe.ops.ransac_essential_pose(dev["matches_xy_ori"], dev["Ks"], threshold=0.1)
    gt = torch.linalg.inv(dev["delta_Rtijs_4_4"].float())
    err_R = dfepe.ops.rot_angle_deg(out["Rt_cam"][:, :, :3].contiguous(), gt[:, :3, :3].contiguous()).cpu().numpy()
    err_t = dfepe.ops.vector_angle_deg(out["Rt_cam"][:, :, 3].contiguous(), gt[:, :3, 3].contiguous()).cpu().numpy()
    print("five-point pose errors (deg):", err_R, err_t, "iterations:", out["iters_run"].cpu().numpy())
    assert (out["winner"] >= 0).all()
    assert (err_R < 1.0).all() and (err_t < 5.0).all()
    win = out["winner"].long().cpu()
    assert torch.equal(out["in_front"].sum(1).cpu(), out["counts"].cpu().gather(1, win[:, None])[:, 0].to(torch.int64))
    assert (out["in_front"] <= out["mask"]).all()  # recoverPose only sees the inliers


def test_recover_camera_five_point_returns_the_references_tuple(dfepe):
    uo = dfepe.compat.utils_opencv
    sc, m, _ = _val_inputs(dfepe, B=1)
    K = sc["Ks"][0].numpy()
    delta_inv = np.linalg.inv(sc["delta_Rtijs_4_4"][0].numpy().astype(np.float64))[:3]
    M, (eR, et), mask2, E = uo.recover_camera_five_point(K, m[0, :, :2], m[0, :, 2:], delta_inv, show_result=False)
    assert M.shape == (3, 4) and M.dtype == np.float64
    assert isinstance(eR, float) and isinstance(et, float) and eR < 1.0 and et < 5.0
    assert mask2.shape == (1000,) and mask2.dtype == bool and 500 < mask2.sum() <= 1000
    assert E.shape == (3, 3) and E.dtype == np.float64
    assert np.allclose(np.linalg.svd(E, compute_uv=False), [2 ** -0.5, 2 ** -0.5, 0], atol=1e-5)  # unit norm, an essential matrix
    # a pair without a pose: matches at random
    g = np.random.default_rng(0)
    M, err, mask2, E = uo.recover_camera_five_point(np.eye(3), g.uniform(-1, 1, (6, 2)), g.uniform(-1, 1, (6, 2)), np.eye(4)[:3],
                                                    threshold=0.0, show_result=False, if_normalized=True)
    if not mask2.any():
        assert err == (180.0, 90.0) and np.array_equal(M, np.hstack((np.eye(3), np.zeros((3, 1)))))
    with pytest.raises(NotImplementedError):  # deliberately unchanged
        uo.recover_camera_opencv(K, m[0, :, :2], m[0, :, 2:], delta_inv, five_point=True)


def test_val_rt_batch_and_the_summary_carry_the_five_point_baseline(dfepe):
    tgu, utils_F = dfepe.compat.train_good_utils, dfepe.compat.utils_F
    sc, m, E_est = _val_inputs(dfepe)
    B = m.shape[0]
    dev = {k: v.to(DEV) for k, v in sc.items()}
    Ee = torch.from_numpy(E_est).to(DEV)
    pairs = tgu.val_rt_batch(dev["Ks"], dev["matches_xy_ori"], Ee, dev["delta_Rtijs_4_4"], baseline="five_point")
    new = {"err_R_deg_opencv5p", "err_t_deg_opencv5p", "Rt_cam_opencv5p", "winner_opencv5p", "E_opencv5p", "F_opencv5p",
           "inlier_mask_opencv5p"}
    plain = tgu.val_rt_batch(dev["Ks"], dev["matches_xy_ori"], Ee, dev["delta_Rtijs_4_4"])
    assert set(pairs) == set(plain) | new
    assert pairs["err_R_deg_opencv5p"].shape == (B,) and float(pairs["err_R_deg_opencv5p"].max()) < 2.0
    K64 = sc["Ks"].double().numpy()
    for i in range(B):
        Ki = np.linalg.inv(K64[i])
        F = Ki.T @ pairs["E_opencv5p"][i].cpu().double().numpy() @ Ki
        assert np.allclose(pairs["F_opencv5p"][i].cpu().double().numpy(), F, rtol=1e-3, atol=1e-5 * np.abs(F).max())  # fp32 products of K^-1 (entries up to ~1)
    summary, pp = tgu.validation_summary(dev["Ks"], dev["matches_xy_ori"], Ee, dev["F_gt"], dev["F_gt"], dev["delta_Rtijs_4_4"],
                                         baseline="five_point")
    assert "opencv_5p" in summary and "opencv_8p" not in summary and pp["epi_dists_opencv5p"].shape == (B, 1000)
    d_ref = np.stack([utils_F.epi_distance_np(pp["F_opencv5p"][i].cpu().double().numpy(), m[i, :, :2], m[i, :, 2:], if_homo=False)[0]
                      for i in range(B)])
    assert np.allclose(pp["epi_dists_opencv5p"].cpu().numpy(), d_ref, rtol=1e-4, atol=1e-4)
    # baseline=True keeps exactly today's keys
    s8, p8 = tgu.validation_summary(dev["Ks"], dev["matches_xy_ori"], Ee, dev["F_gt"], dev["F_gt"], dev["delta_Rtijs_4_4"], baseline=True)
    assert "opencv_8p" in s8 and "opencv_5p" not in s8
    assert set(p8) == set(plain) | {"epi_dists", "epi_dists_gt", "epi_dists_opencv", "err_R_deg_opencv", "err_t_deg_opencv",
                                    "Rt_cam_opencv", "winner_opencv", "F_opencv", "E_opencv", "inlier_mask_opencv"}
