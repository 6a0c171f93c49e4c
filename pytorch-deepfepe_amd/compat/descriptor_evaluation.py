"""Mirror of the reference's homography evaluation of a detector / descriptor front end: evaluations/descriptor_evaluation.py
(compute_homography, homography_estimation) and the inlier labels of deepFEPE/evaluate_frontend.py:210-241 (getInliers,
getInliers_cv), backed by libdfepe_hip.so instead of cv2: the cross-checked matcher is two ops.knn_match launches, the
estimator ops.ransac_homography, the corner test ops.homography_corners, the inlier labels ops.homography_transfer.

What differs from the reference: 'matches' is an int [M,2] array of (index into keypoints1, index into keypoints2), not a list of
cv2.DMatch; the random stream of the estimator is this package's (include/dfepe.h), so results agree with cv2's in distribution;
the reference's print calls are not mirrored; ORB / Hamming matching is not built; homography_estimation takes the loaded
dicts, not an experiment name (there is no settings.EXPER_PATH here).  compute_repeatability is in compat/detector_evaluation.py,
the matching score and the nn mean AP in compat/evaluate_frontend.py.  Not built: the dense-map precision / recall curves
(compute_tp_fp, compute_pr, compute_loc_error) and drawing."""
import numpy as np
import torch

from .. import ops
from .._lib import HOMOGRAPHY_MAX_N, DfepeError


def warp_keypoints(keypoints, H):
    """keypoints [N,2] (x, y), H [3,3] -> the points warped by H (evaluations/detector_evaluation.warp_keypoints); numpy."""
    keypoints = np.asarray(keypoints)
    hom = np.concatenate([keypoints, np.ones((keypoints.shape[0], 1))], axis=1)
    w = np.dot(hom, np.transpose(H))
    return w[:, :2] / w[:, 2:]


def cross_check_batch(desc1, desc2):
    """desc1 [B,N1,D], desc2 [B,N2,D] on the device -> (idx1, idx2 [B,N1] int64, count [B] int32): the mutual nearest neighbours
    (cv2.BFMatcher(NORM_L2, crossCheck=True).match) of every pair in increasing index into desc1, compacted to the front of
    each row; the rest of a row is padding.  Two ops.knn_match launches (ratio_test=False); no host synchronisation."""
    nn12 = ops.knn_match(desc1, desc2, ratio_test=False)[0].long()
    nn21 = ops.knn_match(desc2, desc1, ratio_test=False)[0].long()
    B, N1 = nn12.shape
    i = torch.arange(N1, device=nn12.device).expand(B, N1)
    keep = torch.gather(nn21, 1, nn12) == i
    order = torch.argsort((~keep).to(torch.uint8), dim=1, stable=True)
    return order, torch.gather(nn12, 1, order), keep.sum(1).to(torch.int32)


def compute_homography_batch(kp1, kp2, desc1, desc2, H_gt, correctness_thresh=(3.0,), shape=(240, 320), seed=0):
    """B image pairs on the device: kp1 [B,N1,2], kp2 [B,N2,2] keypoints as (x, y); desc1 [B,N1,D], desc2 [B,N2,D]; H_gt [B,3,3];
    correctness_thresh: a sequence of T thresholds.  Returns dict(correctness [B,T] uint8, mean_dist [B] float64 (NaN without a
    model), homography [B,3,3] float64 (the identity where cv2 would return None), found [B] bool, matches [B,N1,2] int64 with
    n_matches [B] int32 valid rows, inliers [B,N1] uint8, matched_points [B,N1,4]).  No host synchronisation."""
    N1, N2 = desc1.shape[1], desc2.shape[1]
    if N1 > HOMOGRAPHY_MAX_N:
        raise DfepeError(f"compute_homography_batch: {N1} keypoints per image; the estimator takes at most {HOMOGRAPHY_MAX_N} matches")
    i1, i2, cnt = cross_check_batch(desc1, desc2)
    p1 = torch.gather(kp1.float(), 1, i1.unsqueeze(-1).expand(-1, -1, 2))
    p2 = torch.gather(kp2.float(), 1, i2.unsqueeze(-1).expand(-1, -1, 2))
    m = torch.cat((p1, p2), 2).contiguous()
    est = ops.ransac_homography(m, cnt, seed=seed)
    found = est["n_inliers"] > 0
    th = torch.as_tensor(list(correctness_thresh), dtype=torch.float64, device=m.device)
    mean_dist, correct = ops.homography_corners(est["H"], H_gt, int(shape[0]), int(shape[1]), th)
    eye = torch.eye(3, dtype=torch.float64, device=m.device).expand_as(est["H"])
    return {"correctness": correct, "mean_dist": mean_dist, "homography": torch.where(found[:, None, None], est["H"], eye), "found": found,
            "matches": torch.stack((i1, i2), 2), "n_matches": cnt, "inliers": est["mask"], "matched_points": m}


def compute_homography(data, keep_k_points=1000, correctness_thresh=3, orb=False, shape=(240, 320)):
    """evaluations/descriptor_evaluation.compute_homography (lines 54-130) with the reference's signature and dict keys: data
    holds 'prob' and 'warped_prob' [N,>=2] keypoints as (x, y, ...), 'desc' and 'warped_desc' [N,D], 'homography' [3,3].
    Returns {'correctness', 'keypoints1', 'keypoints2', 'matches', 'inliers', 'homography'}: keypoints as (y, x) like the
    reference; 'matches' an int [M,2] index array (queryIdx, trainIdx), not cv2.DMatch objects; 'inliers' uint8 [M];
    'correctness' a bool, or a bool array when correctness_thresh is a list (evaluate_frontend.py:162 passes [1, 3, 5]);
    without a model correctness is 0 and 'homography' the identity.  keep_k_points is unused, as in the reference."""
    if orb:
        raise NotImplementedError("compute_homography(orb=True): Hamming matching of binary descriptors is not built")
    dev = torch.device("cuda")
    keypoints = np.asarray(data["prob"])[:, [1, 0]]
    warped_keypoints = np.asarray(data["warped_prob"])[:, [1, 0]]
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev).unsqueeze(0)  # noqa: E731
    scalar = np.ndim(correctness_thresh) == 0
    th = [float(correctness_thresh)] if scalar else [float(v) for v in correctness_thresh]
    H_gt = torch.as_tensor(np.asarray(data["homography"], dtype=np.float64), device=dev).unsqueeze(0)
    out = compute_homography_batch(t(keypoints[:, [1, 0]]), t(warped_keypoints[:, [1, 0]]), t(data["desc"]), t(data["warped_desc"]), H_gt,
                                   th, shape)
    M = int(out["n_matches"][0])
    found = bool(out["found"][0])
    correct = out["correctness"][0].cpu().numpy().astype(bool)
    if not found:
        correctness = 0
    else:
        correctness = bool(correct[0]) if scalar else correct
    return {"correctness": correctness, "keypoints1": keypoints, "keypoints2": warped_keypoints,
            "matches": out["matches"][0, :M].cpu().numpy(), "inliers": out["inliers"][0, :M].cpu().numpy(),
            "homography": out["homography"][0].cpu().numpy()}


def homography_estimation(list_of_data, keep_k_points=1000, correctness_thresh=3, orb=False, shape=(240, 320)):
    """evaluations/descriptor_evaluation.homography_estimation over the loaded dicts (not an experiment name): the mean
    correctness."""
    return np.mean([compute_homography(d, keep_k_points, correctness_thresh, orb, shape)["correctness"] for d in list_of_data], axis=0)


def get_inliers(matches, H, epi=3):
    """evaluate_frontend.getInliers: matches numpy [n,4] (x1, y1, x2, y2), H [3,3] -> bool [n], |H x1 - x2| < epi."""
    m = np.array(np.asarray(matches)[:, :4], dtype=np.float32)  # a writable, contiguous copy
    if m.shape[0] == 0:
        return np.zeros(0, dtype=bool)
    dev = torch.device("cuda")
    Ht = torch.as_tensor(np.asarray(H, dtype=np.float64), device=dev).unsqueeze(0)
    return ops.homography_transfer(Ht, torch.as_tensor(m, device=dev).unsqueeze(0), None, epi)[1][0].cpu().numpy().astype(bool)


def get_inliers_cv(matches, seed=0):
    """evaluate_frontend.getInliers_cv: the inlier mask of findHomography(RANSAC) on the matches [n,4], flattened (uint8 [n])."""
    from .utils_opencv import findHomography

    m = np.asarray(matches)
    return findHomography(m[:, [0, 1]], m[:, [2, 3]], 8, seed=seed)[1].flatten()
