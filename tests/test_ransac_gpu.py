"""The batched RANSAC fundamental-matrix estimator (csrc/ransac.hip: ops.ransac_fundamental / ops.ransac_pose) on the device,
against the fp64 restatement of OpenCV 3.4's findFundamentalMat(FM_RANSAC) in tests/ransac_ref.py, and the validation baseline
built on it (compat.utils_opencv.recover_camera_opencv, compat.train_good_utils.val_rt / val_rt_batch / validation_summary)."""
import os
import sys
import warnings
from collections import defaultdict

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_ref as ref  # noqa: E402
import test_ransac_edges_gpu as edges  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAND = 1e-4  # relative band around t^2 inside which a decision may differ from the fp64 restatement


def unit(F):
    f = np.asarray(F, np.float64).ravel()
    f = f / np.linalg.norm(f)
    return f * np.sign(f[np.argmax(np.abs(f))])


def _scene(dfepe, B, N, seed, outliers, noise=0.5):
    return dfepe.synth.make_scene(B, N, seed=seed, outlier_ratio=outliers, noise_px=noise)


def test_noise_free_pairs_stop_after_the_first_model(dfepe):
    sc = _scene(dfepe, 8, 100, 11, 0.0, noise=0.0)
    out = dfepe.ops.ransac_fundamental(sc["matches_xy_ori"].to(DEV))
    torch.cuda.synchronize()
    assert (out["mask"] == 1).all()
    assert (out["n_inliers"] == 100).all()
    assert (out["iters_run"] == 1).all()  # ep = 0: RANSACUpdateNumIters returns 0 after the first model
    assert (out["best_hyp"][:, 0] == 0).all()
    for b in range(8):
        F = out["F"][b].cpu().double().numpy()
        assert F[2, 2] == 1.0
        assert np.linalg.norm(unit(F) - unit(sc["F_gt"][b].double().numpy())) < 1e-4


@pytest.fixture(scope="module")
def outlier_run(dfepe):
    sc = _scene(dfepe, 2, 1000, 5, 0.4)
    m = sc["matches_xy_ori"].numpy()
    out = edges.run(dfepe, m, 1.0, 0.99, 1000, 3)  # also: the workspace table gives bit-identical outputs
    return m, out, [ref.hypotheses(m[b], 3, 1000) for b in range(m.shape[0])]


def test_count_table_against_the_fp64_restatement(outlier_run):
    m, out, hyps = outlier_run
    for b in range(m.shape[0]):
        verdict, n_cmp = edges.check_pair(m, out, b, 1.0, 0.99, 3, 1000, hyps[b])
        assert n_cmp > 900
        assert verdict == "exact"  # the rule over the restatement's own table reaches the device's count, iteration and stop


def test_selection_and_mask_follow_the_sequential_rule(outlier_run):
    m, out, hyps = outlier_run
    t2 = 1.0
    for b in range(m.shape[0]):
        best, bk, br, iters = ref.select(out["hyp_counts"][b], m.shape[1], 0.99, 1000)
        assert (best, bk, br, iters) == (out["n_inliers"][b], out["best_hyp"][b, 0], out["best_hyp"][b, 1], out["iters_run"][b])
        assert best > 300  # 60 % true correspondences with 0.5 px noise: ~390 within 1 px
        mask = out["mask"][b]
        assert int(mask.sum()) == best
        err = ref.errors(out["F"][b].astype(np.float64), m[b])
        sure = np.abs(err - t2) > BAND * t2
        assert ((mask == 1) == (err <= t2))[sure].all()
        # the winner is the root of that iteration's sample whose count is n_inliers
        idx, Fr = hyps[b][bk]
        assert idx == ref.draw_sample(3, bk, m[b])
        Fc = [F for F in Fr if int((ref.errors(F, m[b]) <= t2).sum()) == best]
        assert Fc and min(np.linalg.norm(unit(out["F"][b]) - unit(F)) for F in Fc) < 1e-5


def test_pose_on_the_nan_masked_matches(dfepe):
    sc = _scene(dfepe, 6, 1000, 21, 0.3)
    m, K = sc["matches_xy_ori"].to(DEV), sc["Ks"].to(DEV)
    out = dfepe.ops.ransac_pose(m, K, threshold=1.0)
    Rt64, win64, cnt64 = dfepe.ops.cheirality(out["E"], K, out["masked"], 50.0, fp64_only=True)
    torch.cuda.synchronize()
    assert torch.equal(out["counts"], cnt64) and torch.equal(out["winner"], win64)
    mask = out["mask"].bool()
    assert (torch.isnan(out["masked"]).all(-1) == ~mask).all()
    for b in range(6):
        sub = m[b][mask[b]].unsqueeze(0).contiguous()  # recoverPose(mask=...) = the pose of the inlier subset
        _, w1, c1 = dfepe.ops.cheirality(out["E"][b:b + 1], K[b:b + 1], sub, 50.0, fp64_only=True)
        assert torch.equal(c1[0], out["counts"][b]) and int(w1[0]) == int(out["winner"][b])
        assert int(out["winner"][b]) >= 0
        assert int(out["in_front"][b].sum()) == int(out["counts"][b, out["winner"][b]])
        assert not (out["in_front"][b].bool() & ~mask[b]).any()


def test_deterministic_and_batch_invariant(dfepe):
    big = _scene(dfepe, 64, 500, 31, 0.3)["matches_xy_ori"].to(DEV)
    one = _scene(dfepe, 1, 500, 77, 0.3)["matches_xy_ori"].to(DEV)
    big[17] = one[0]
    kw = dict(threshold=0.5, max_iters=700, seed=9, want_hyp_counts=True, want_masked=True)
    a = dfepe.ops.ransac_fundamental(big, **kw)
    b = dfepe.ops.ransac_fundamental(big, **kw)
    c = dfepe.ops.ransac_fundamental(one, **kw)
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k].view(torch.uint8) if a[k].is_floating_point() else a[k],
                           b[k].view(torch.uint8) if b[k].is_floating_point() else b[k]), k
        x, y = a[k][17], c[k][0]
        assert torch.equal(x.view(torch.uint8) if x.is_floating_point() else x, y.view(torch.uint8) if y.is_floating_point() else y), k


def test_fewer_than_15_correspondences_is_refused(dfepe):
    with pytest.raises(dfepe._lib.DfepeError, match="LMedS"):
        dfepe.ops.ransac_fundamental(torch.rand(2, 14, 4, device=DEV) * 100)


def _val_inputs(dfepe, B=4, N=1000, seed=41):
    sc = _scene(dfepe, B, N, seed, 0.2, noise=0.05)  # most true correspondences within the baseline's fixed 0.1 px
    m = sc["matches_xy_ori"].numpy()
    E_est = sc["E_gt"].numpy() + np.random.default_rng(seed).normal(0, 1e-3, (B, 3, 3)).astype(np.float32)
    return sc, m, E_est


def test_recover_camera_opencv_returns_the_references_tuple(dfepe):
    uo = dfepe.compat.utils_opencv
    sc, m, _ = _val_inputs(dfepe, B=1)
    K = sc["Ks"][0].numpy()
    delta_inv = np.linalg.inv(sc["delta_Rtijs_4_4"][0].numpy().astype(np.float64))[:3]
    M, (eR, et), mask2, (E, F) = uo.recover_camera_opencv(K, m[0, :, :2], m[0, :, 2:], delta_inv, show_result=False)
    assert M.shape == (3, 4) and M.dtype == np.float64
    assert isinstance(eR, float) and isinstance(et, float) and eR < 1.0 and et < 5.0
    assert mask2.shape == (1000,) and mask2.dtype == bool and 500 < mask2.sum() <= 1000
    assert E.shape == (3, 3) and F.shape == (3, 3)
    assert np.allclose(np.linalg.svd(E, compute_uv=False), [1, 1, 0], atol=1e-5)
    # E_given: no RANSAC, every correspondence takes part; the pose of the ground-truth E
    M2, err2, mask3, (E2, F2) = uo.recover_camera_opencv(K, m[0, :, :2], m[0, :, 2:], delta_inv, E_given=sc["E_gt"][0].numpy(),
                                                         show_result=False)
    assert F2 is None and err2[0] < 0.5 and mask3.sum() > mask2.sum() * 0.5
    with pytest.raises(NotImplementedError):
        uo.recover_camera_opencv(K, m[0, :, :2], m[0, :, 2:], delta_inv, five_point=True)


def test_a_pair_without_a_model_gets_the_failure_values(dfepe):
    uo = dfepe.compat.utils_opencv
    rng = np.random.default_rng(0)
    x1 = np.c_[np.arange(50.0), 2.0 * np.arange(50.0) + 3.0].astype(np.float32)  # image 1: every point on one line: no sample
    x2 = rng.uniform(0, 500, (50, 2)).astype(np.float32)
    out = dfepe.ops.ransac_pose(torch.from_numpy(np.c_[x1, x2]).unsqueeze(0).to(DEV), torch.eye(3, device=DEV).unsqueeze(0))
    assert int(out["n_inliers"][0]) == 0 and int(out["iters_run"][0]) == 0 and (out["F"] == 0).all() and (out["mask"] == 0).all()
    assert int(out["winner"][0]) == -1 and int(out["in_front"].sum()) == 0
    M, err, mask2, _ = uo.recover_camera_opencv(np.eye(3), x1, x2, np.eye(4)[:3], show_result=False)
    assert err == (180.0, 90.0) and not mask2.any() and np.array_equal(M, np.hstack((np.eye(3), np.zeros((3, 1)))))


def test_val_rt_fills_the_baseline_slots_and_the_agents_block_records_both_tags(dfepe):
    tgu, um = dfepe.compat.train_good_utils, dfepe.compat.utils_misc
    sc, m, E_est = _val_inputs(dfepe)
    B = m.shape[0]
    Ks, F_gt, E_gt, delta = sc["Ks"].numpy(), sc["F_gt"].numpy(), sc["E_gt"].numpy(), sc["delta_Rtijs_4_4"].numpy()
    results = []
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for i in range(B):
            results.append(tgu.val_rt(i, Ks[i], m[i, :, :2], m[i, :, 2:], E_est[i], E_gt[i], F_gt[i], F_gt[i], delta[i], False))
    assert not [w for w in caught if "val_rt" in str(w.message)]  # the default if_opencv=True with five_point=False warns no more
    # Train_model_pipeline.py:1063-1150, restated: what the agent does with each result
    dict_of_lists = defaultdict(lambda: defaultdict(list))
    for i, r in enumerate(results):
        error_Rt_estW, epi_dist_mean_estW, error_Rt_5point, epi_dist_mean_5point, error_Rt_gt, epi_dist_mean_gt = r[:6]
        M_estW, M_opencv = um.Rt_pad(r[7]), um.Rt_pad(r[8])
        assert M_opencv.shape == (4, 4) and M_estW.shape == (4, 4)
        assert error_Rt_estW and error_Rt_5point
        for tag, e, d in (("DeepF", error_Rt_estW, epi_dist_mean_estW), ("opencv_8p", error_Rt_5point, epi_dist_mean_5point),
                          ("gt", error_Rt_gt, epi_dist_mean_gt)):
            dict_of_lists["err_q"][tag].append(e[0])
            dict_of_lists["err_t"][tag].append(e[1])
            dict_of_lists["epi_dists"][tag].append(np.expand_dims(d, -1))
        assert isinstance(epi_dist_mean_5point, np.ndarray) and epi_dist_mean_5point.shape == (1000,)
        assert len(error_Rt_5point) == 2 and all(isinstance(v, float) for v in error_Rt_5point)
    assert len(dict_of_lists["err_q"]["DeepF"]) == B and len(dict_of_lists["err_q"]["opencv_8p"]) == B
    assert max(dict_of_lists["err_q"]["opencv_8p"]) < 2.0

    # the batched form gives the per-pair numbers
    dev = {k: v.to(DEV) for k, v in sc.items()}
    pairs = tgu.val_rt_batch(dev["Ks"], dev["matches_xy_ori"], torch.from_numpy(E_est).to(DEV), dev["delta_Rtijs_4_4"], baseline=True)
    for i, r in enumerate(results):
        assert abs(float(pairs["err_R_deg_opencv"][i]) - r[2][0]) < 1e-3
        assert abs(float(pairs["err_t_deg_opencv"][i]) - r[2][1]) < 1e-3
        Rc = pairs["Rt_cam_opencv"][i].cpu().double().numpy()
        assert np.allclose(r[8][:, :3], Rc[:, :3].T, atol=1e-6)
    summary, pp = tgu.validation_summary(dev["Ks"], dev["matches_xy_ori"], torch.from_numpy(E_est).to(DEV), dev["F_gt"], dev["F_gt"],
                                         dev["delta_Rtijs_4_4"], baseline=True)
    assert "opencv_8p" in summary and pp["epi_dists_opencv"].shape == (B, 1000)
    d_ref = np.stack([r[3] for r in results])
    assert np.allclose(pp["epi_dists_opencv"].cpu().numpy(), d_ref, rtol=1e-4, atol=1e-4)
    # the default keeps today's outputs
    plain, pp0 = tgu.validation_summary(dev["Ks"], dev["matches_xy_ori"], torch.from_numpy(E_est).to(DEV), dev["F_gt"], dev["F_gt"],
                                        dev["delta_Rtijs_4_4"])
    assert "opencv_8p" not in plain and "epi_dists_opencv" not in pp0 and "err_R_deg_opencv" not in pp0


def test_five_point_keeps_the_warning_and_the_none_slots(dfepe, monkeypatch):
    tgu = dfepe.compat.train_good_utils
    monkeypatch.setattr(tgu, "_warned_opencv", False)
    sc, m, E_est = _val_inputs(dfepe, B=1)
    with pytest.warns(RuntimeWarning, match="five-point"):
        r = tgu.val_rt(0, sc["Ks"][0].numpy(), m[0, :, :2], m[0, :, 2:], E_est[0], sc["E_gt"][0].numpy(), sc["F_gt"][0].numpy(),
                       sc["F_gt"][0].numpy(), sc["delta_Rtijs_4_4"][0].numpy(), True)
    assert r[2] is None and r[3] is None and r[8] is None and r[0] is not None
