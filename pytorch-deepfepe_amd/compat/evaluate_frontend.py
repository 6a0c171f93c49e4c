"""Mirror of the reference's front-end evaluation loop, deepFEPE/evaluate_frontend.py: the five numbers it reports per image pair
(line 45: correctness, repeatability, mscore, mAP, localization_err) and the means it writes to result.txt (lines 143-157).
Everything runs in libdfepe_hip.so: compute_repeatability_batch (ops.keypoint_repeatability), compute_homography_batch
(ops.knn_match, ops.ransac_homography, ops.homography_corners), the matching score (ops.matching_score, lines 176-183), the
two-way matches of PointTracker at nn_thresh = 1.2 (ops.nn_match_two_way, lines 186-208), their labels by getInliers
(ops.homography_transfer) or getInliers_cv (ops.ransac_homography), and the average precision (ops.average_precision in place of
sklearn.metrics.average_precision_score, lines 244-275).

What differs from the reference: keypoints are (x, y) rows throughout (the reference's loop body is an outline that mixes both
orders); warpLabels belongs to the superpoint package, which is not part of the reference's tree, so its count is the one stated
in include/dfepe.h -- the image-2 keypoints whose warp by inv(H) lies in 0 <= x <= w - 1, 0 <= y <= h - 1, both ends inclusive,
nothing truncated; the random stream of the homography estimator is this package's; files, prints and images are not mirrored.
Not built: the dense-map precision / recall curves and drawing."""
import numpy as np
import torch

from .. import ops
from .descriptor_evaluation import compute_homography_batch
from .detector_evaluation import compute_repeatability_batch

NN_THRESH = 1.2  # evaluate_frontend.py:192
HOMOGRAPHY_THRESH = (1.0, 3.0, 5.0)  # evaluate_frontend.py:162


def matching_score(inliers, keypoints, warped_keypoints, real_H, shape):
    """evaluate_frontend.py:176-183: inliers (the mask of compute_homography's result), keypoints [N1,>=2] and warped_keypoints
    [N2,>=2] as (x, y) rows, real_H [3,3], shape = (h, w) -> 2 * inliers.sum() / (N1 + the number of warped_keypoints that
    warpLabels(..., inv(real_H), h, w) keeps)."""
    dev = torch.device("cuda")
    t = lambda a: torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(len(a), -1)[:, :2]), device=dev).unsqueeze(0)  # noqa: E731
    H = torch.as_tensor(np.asarray(real_H, dtype=np.float64), device=dev).unsqueeze(0)
    rep = compute_repeatability_batch(t(keypoints), t(warped_keypoints), H, shape, 0, ())
    n_in = torch.as_tensor([int(np.asarray(inliers).sum())], dtype=torch.int32, device=dev)
    n_kp = torch.as_tensor([len(keypoints)], dtype=torch.int32, device=dev)
    return float(ops.matching_score(n_in, n_kp, rep["n_unwarped"])[0])


def nn_average_precision(matches_dist, inliers):
    """evaluate_frontend.py:252-273: matches_dist [n] the distances of the two-way matches (mscores[:, 2]), inliers [n] their
    labels -> the average precision of the scores max(dist) - dist (flipArr, taken in the input's dtype as the reference does),
    0 when there is no match or no positive."""
    dist, lab = np.asarray(matches_dist), np.asarray(inliers)
    if not (lab.shape[0] > 0 and lab.sum() > 0):
        return 0
    dev = torch.device("cuda")
    flip = dist.max() - dist
    out = ops.average_precision(torch.as_tensor(np.ascontiguousarray(lab != 0), device=dev).unsqueeze(0),
                                torch.as_tensor(np.ascontiguousarray(flip), device=dev).unsqueeze(0))
    return float(out["ap"][0])


def frontend_metrics_batch(kp1, kp2, desc1, desc2, H_gt, shape, rep_thd=3.0, keep_k_points=300, homography_thresh=HOMOGRAPHY_THRESH,
                           inliers_method="gt", nn_thresh=NN_THRESH, epi=3.0, seed=0):
    """B image pairs on the device: kp1 [B,N1,C], kp2 [B,N2,C] rows (x, y[, prob]); desc1 [B,N1,D], desc2 [B,N2,D] unit-norm
    descriptors; H_gt [B,3,3]; shape = (h, w).  inliers_method: 'gt' labels the two-way matches by |H_gt x1 - x2| < epi
    (getInliers), 'cv' by the mask of the RANSAC homography of the matches (getInliers_cv).  Returns dict(correctness [B,T]
    uint8, repeatability, localization_err, mscore, mAP [B] float64, and for inspection n_unwarped, n_matches, nn_count [B] int32).
    localization_err is -1 and repeatability 0 where nothing is counted; mAP is 0 without a match or a positive.  No host
    synchronisation."""
    if inliers_method not in ("gt", "cv"):
        raise ValueError(f"inliers_method must be 'gt' or 'cv', got {inliers_method!r}")
    B, N1 = kp1.shape[0], kp1.shape[1]
    dev = kp1.device
    rep = compute_repeatability_batch(kp1, kp2, H_gt, shape, keep_k_points, [float(rep_thd)])
    xy1, xy2 = kp1[:, :, :2].float(), kp2[:, :, :2].float()
    hom = compute_homography_batch(xy1, xy2, desc1, desc2, H_gt, homography_thresh, shape, seed)
    n_in = hom["inliers"].sum(1, dtype=torch.int32)
    mscore = ops.matching_score(n_in, torch.full((B,), N1, dtype=torch.int32, device=dev), rep["n_unwarped"])
    m1, m2, dist, cnt = ops.nn_match_two_way(desc1, desc2, float(nn_thresh))
    if N1 > 0:
        p1 = torch.gather(xy1, 1, m1.long().clamp(0, N1 - 1).unsqueeze(-1).expand(-1, -1, 2))
        p2 = torch.gather(xy2, 1, m2.long().clamp(0, max(kp2.shape[1] - 1, 0)).unsqueeze(-1).expand(-1, -1, 2))
        m = torch.cat((p1, p2), 2).contiguous()
        if inliers_method == "gt":
            labels = ops.homography_transfer(H_gt, m, cnt, float(epi))[1]
        else:
            labels = ops.ransac_homography(m, cnt, seed=seed)["mask"]
        valid = torch.arange(dist.shape[1], device=dev)[None, :] < cnt[:, None]
        top = torch.where(valid, dist, torch.full_like(dist, float("-inf"))).max(1, keepdim=True).values
        ap = ops.average_precision(labels, top - dist, cnt)["ap"]  # flipArr in the distances' own dtype
    else:
        ap = torch.zeros(B, dtype=torch.float64, device=dev)
    return {"correctness": hom["correctness"] * hom["found"][:, None].to(torch.uint8), "repeatability": rep["repeatability"][:, 0],
            "localization_err": rep["loc_err"][:, 0], "mscore": mscore, "mAP": ap, "n_unwarped": rep["n_unwarped"],
            "n_matches": hom["n_matches"], "nn_count": cnt}


def evaluate(list_of_data, rep_thd=3, inliers_method="gt", seed=0):
    """The means evaluate_frontend.py writes to result.txt, over the loaded dicts (keys 'prob', 'warped_prob' [N,3] rows (x, y,
    prob), 'desc', 'warped_desc' [N,D], 'homography' [3,3], 'image' [h,w]): dict(repeatability, localization_err, correctness
    (one mean per threshold of 1, 3, 5), mscore, mAP).  The localization error is averaged only over the pairs where it is > 0
    (lines 172-173; NaN when there is none, as numpy's mean of an empty list)."""
    dev = torch.device("cuda")
    rows = {k: [] for k in ("repeatability", "localization_err", "correctness", "mscore", "mAP")}
    for d in list_of_data:
        t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=dev).unsqueeze(0)  # noqa: E731
        out = frontend_metrics_batch(t(d["prob"], np.float64), t(d["warped_prob"], np.float64), t(d["desc"], np.float32),
                                     t(d["warped_desc"], np.float32), t(d["homography"], np.float64), np.asarray(d["image"]).shape,
                                     rep_thd=rep_thd, inliers_method=inliers_method, seed=seed)
        rows["repeatability"].append(float(out["repeatability"][0]))
        le = float(out["localization_err"][0])
        if le > 0:
            rows["localization_err"].append(le)
        rows["correctness"].append(out["correctness"][0].cpu().numpy().astype(np.float64))
        rows["mscore"].append(float(out["mscore"][0]))
        rows["mAP"].append(float(out["mAP"][0]))
    with np.errstate(all="ignore"):
        return {"repeatability": np.array(rows["repeatability"]).mean(), "localization_err": np.array(rows["localization_err"]).mean(),
                "correctness": np.array(rows["correctness"]).mean(axis=0), "mscore": np.array(rows["mscore"]).mean(axis=0),
                "mAP": np.array(rows["mAP"]).mean()}
