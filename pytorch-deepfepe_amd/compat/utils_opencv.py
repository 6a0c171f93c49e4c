"""Mirror of deepFEPE.dsac_tools.utils_opencv: the OpenCV 8-point RANSAC baseline of the validation (recover_camera_opencv,
utils_opencv.py:129-208), backed by the batched RANSAC estimator of libdfepe_hip.so (ops.ransac_pose) instead of cv2.

What differs from OpenCV: the random stream (include/dfepe.h, dfepe_ransac_fundamental), so results agree with cv2's in
distribution, not bit for bit.  The five-point baseline (cv2.findEssentialMat, Nister's solver) is recover_camera_five_point,
backed by ops.ransac_essential_pose; recover_camera_opencv(five_point=True) itself still raises.  LMedS, OpenCV's choice for
fewer than 15 correspondences of the 8-point branch, is ops.lmeds_pose: recover_camera_opencv takes it for 8 <= N < 15 as OpenCV
does, and recover_camera_lmeds runs it (or its five-point form, cv2.findEssentialMat(method=LMEDS)) on any pair.  Not built: the
direct 7-point solve OpenCV runs on exactly 7 correspondences.

KNN_match (utils_opencv.py:39-90) is backed by ops.knn_match: the exact k = 2 search of cv2.BFMatcher(NORM_L2).knnMatch with
Lowe's ratio test.  What differs from OpenCV: ``if_BF=False`` selects FLANN's randomised kd-trees (5 trees, 50 checks) in the
reference, an approximate search whose answer is not reproducible; here both values of ``if_BF`` run the exact search, so the
FLANN branch's occasional misses do not occur.  Near-ties inside the float32 error of the distance (include/dfepe.h,
dfepe_knn_match) may be ordered differently from OpenCV's own float32 summation.

triangulatePoints stands in for cv2.triangulatePoints (utils_opencv.py:199 and the other call sites listed in its docstring),
backed by ops.triangulate."""
import numpy as np
import torch

from .. import ops
from .._lib import LMEDS_MIN_N, RANSAC_MIN_N

BASELINE_THRESHOLD = 0.1  # the reference's 8-point branch passes 0.1 to findFundamentalMat whatever `threshold` says (:157)
FIVE_POINT_THRESHOLD = 0.01  # what val_rt passes to the five-point branch, which uses it (train_good_utils.py:622)
FAILED = (180.0, 90.0)    # the pose-error values of a pair without a pose (utils_F.goodCorr_eval_nondecompose, utils_F.py:942-952)


def recover_pose_camera(K):
    """K [B,3,3] (device) -> the camera the reference hands cv2.recoverPose: focal K[0,0], principal point (K[0,2], K[1,2])
    (utils_opencv.py:177)."""
    return ops._recover_pose_camera(K)


def triangulatePoints(projMatr1, projMatr2, projPoints1, projPoints2):
    """cv2.triangulatePoints with cv2's layout, numpy in and out: projMatr1, projMatr2 [3,4], projPoints1, projPoints2 [2,N]
    -> [4,N] homogeneous points, from one launch (ops.triangulate).  The values are the float32 output of the kernel (fp64
    arithmetic, one rounding; include/dfepe.h, dfepe_triangulate): every column has unit 2-norm and w = out[3] >= 0, where OpenCV
    leaves the sign to its SVD -- every call site of the reference divides by w (utils_F.py:554, :712, DeepFNet.py:421-422,
    utils_opencv.py:199)."""
    x1, x2 = np.asarray(projPoints1, dtype=np.float32), np.asarray(projPoints2, dtype=np.float32)
    if x1.ndim != 2 or x1.shape[0] != 2 or x2.shape != x1.shape:
        raise ValueError(f"projPoints1 and projPoints2 must both be [2,N], got {x1.shape} and {x2.shape}")
    if x1.shape[1] == 0:
        return np.zeros((4, 0), dtype=np.float32)
    dev = torch.device("cuda")
    m = torch.as_tensor(np.ascontiguousarray(np.vstack((x1, x2)).T), device=dev).unsqueeze(0)
    P1 = torch.as_tensor(np.ascontiguousarray(projMatr1, dtype=np.float32), device=dev)
    P2 = torch.as_tensor(np.ascontiguousarray(projMatr2, dtype=np.float32), device=dev)
    return np.ascontiguousarray(ops.triangulate(P1, P2, m)[0].cpu().numpy().T)


def _pose_errors(Rt_cam, delta_Rtij_inv):
    """Rotation / translation angle (degrees) of camera motion [3,4] against the ground truth, as goodCorr_eval_nondecompose
    measures them (utils_geo.rot12_to_angle_error / vector_angle)."""
    gt = torch.as_tensor(np.asarray(delta_Rtij_inv), dtype=torch.float32, device=Rt_cam.device)
    err_R = ops.rot_angle_deg(Rt_cam[:, :3].reshape(1, 3, 3), gt[:3, :3].reshape(1, 3, 3))[0].item()
    err_t = ops.vector_angle_deg(Rt_cam[:, 3].reshape(1, 3), gt[:3, 3].reshape(1, 3))[0].item()
    return err_R, err_t


def recover_camera_opencv(K, x1, x2, delta_Rtij_inv, five_point=False, threshold=0.1, show_result=True, c=False,
                          if_normalized=False, method_app="", E_given=None, RANSAC=True):
    """Same call, defaults and return as the reference: (np.hstack((R, t)) [3,4] (scene motion, x2 ~ R x1 + t),
    (error_R, error_t) degrees, mask2 [N] bool (the correspondences recoverPose kept), (E, F)).
    The 8-point branch ignores ``threshold`` and uses 0.1 px like the reference.  ``E_given`` skips RANSAC (every correspondence
    takes part in the pose; F is then None: the reference has none to return).  ``if_normalized``: the pose step uses focal 1 and
    principal point (0, 0).  ``RANSAC`` only concerned the five-point branch in the reference.  A pair whose pose has no point in
    front of both cameras gets the identity, (180, 90) and an all-False mask."""
    if five_point:
        raise NotImplementedError("recover_camera_opencv(five_point=True): Nister's five-point solver (cv2.findEssentialMat) is not built")
    dev = torch.device("cuda")
    K = np.asarray(K, dtype=np.float64)
    x1, x2 = np.asarray(x1), np.asarray(x2)
    m = torch.as_tensor(np.hstack((x1, x2)), dtype=torch.float32, device=dev).unsqueeze(0).contiguous()
    Kt = torch.as_tensor(K, dtype=torch.float32, device=dev).reshape(1, 3, 3)
    K_pose = torch.eye(3, device=dev).reshape(1, 3, 3) if if_normalized else recover_pose_camera(Kt)
    if E_given is None:
        if LMEDS_MIN_N <= m.shape[1] < RANSAC_MIN_N:  # cv2.findFundamentalMat(.., cv2.RANSAC, ..) runs LMedS there; no threshold
            out = ops.lmeds_pose(m, Kt, K_pose=K_pose)
        else:
            out = ops.ransac_pose(m, Kt, threshold=BASELINE_THRESHOLD, K_pose=K_pose)
        E, F = out["E"], out["F"]
        Rt_cam, win, in_front = out["Rt_cam"], out["winner"], out["in_front"]
        F_np = F[0].cpu().double().numpy()
    else:
        E = torch.as_tensor(np.asarray(E_given, dtype=np.float64), dtype=torch.float32, device=dev).reshape(1, 3, 3)
        Rt_cam, win, _ = ops.cheirality(E, K_pose, m, 50.0)
        in_front = ops.ransac_in_front(E, K_pose, m, win)
        F_np = None
    mask2 = in_front[0].cpu().numpy() > 0
    if int(win[0].item()) < 0:
        M = np.hstack((np.eye(3), np.zeros((3, 1))))
        err = FAILED
    else:
        err = _pose_errors(Rt_cam[0], delta_Rtij_inv)
        R = Rt_cam[0, :, :3].t()
        t = -(R @ Rt_cam[0, :, 3].reshape(3, 1))
        M = torch.cat((R, t), 1).cpu().double().numpy()
    if show_result:
        print("Recovered by OpenCV %s (camera): The rotation error (degree) %.4f, and translation error (degree) %.4f"
              % ("8 point" + method_app, err[0], err[1]))
    return M, err, mask2, (E[0].cpu().double().numpy(), F_np)


def recover_camera_five_point(K, x1, x2, delta_Rtij_inv, threshold=0.1, show_result=True, if_normalized=False, method_app=""):
    """The five_point=True branch of the reference's recover_camera_opencv (utils_opencv.py:147-151,177,207):
    cv2.findEssentialMat(x1, x2, focal K[0,0], pp, RANSAC, 0.999, threshold) and cv2.recoverPose with the same camera, by
    ops.ransac_essential_pose.  ``if_normalized``: focal 1 and principal point (0, 0), points and threshold used as given.
    Returns the reference's five-point tuple: (np.hstack((R, t)) [3,4], (error_R, error_t) degrees, mask2 [N] bool, E [3,3]);
    a pair without a pose gets the identity, (180, 90) and an all-False mask."""
    dev = torch.device("cuda")
    m = torch.as_tensor(np.hstack((np.asarray(x1), np.asarray(x2))), dtype=torch.float32, device=dev).unsqueeze(0).contiguous()
    Kt = torch.eye(3, device=dev).reshape(1, 3, 3) if if_normalized else \
        torch.as_tensor(np.asarray(K, dtype=np.float64), dtype=torch.float32, device=dev).reshape(1, 3, 3)
    out = ops.ransac_essential_pose(m, Kt, threshold=threshold)
    Rt_cam = out["Rt_cam"]
    mask2 = out["in_front"][0].cpu().numpy() > 0
    if int(out["winner"][0].item()) < 0:
        M = np.hstack((np.eye(3), np.zeros((3, 1))))
        err = FAILED
    else:
        err = _pose_errors(Rt_cam[0], delta_Rtij_inv)
        R = Rt_cam[0, :, :3].t()
        t = -(R @ Rt_cam[0, :, 3].reshape(3, 1))
        M = torch.cat((R, t), 1).cpu().double().numpy()
    if show_result:
        print("Recovered by OpenCV %s (camera): The rotation error (degree) %.4f, and translation error (degree) %.4f"
              % ("5 point" + method_app, err[0], err[1]))
    return M, err, mask2, out["E"][0].cpu().double().numpy()


def recover_camera_lmeds(K, x1, x2, delta_Rtij_inv, five_point=False, show_result=True, if_normalized=False, method_app=""):
    """The pose of one pair by least median of squares, with the reference's return for either branch.
    five_point=False: what cv2.findFundamentalMat(x1, x2, cv2.RANSAC, 0.1) computes below 15 correspondences (utils_opencv.py:157),
    here for any 8 <= N <= 4096, by ops.lmeds_pose; returns (np.hstack((R, t)) [3,4], (error_R, error_t) degrees, mask2 [N] bool,
    (E, F)) like recover_camera_opencv.  five_point=True: cv2.findEssentialMat(.., method=cv2.LMEDS) -- what RANSAC=False means in
    OpenCV's five-point branch (:137-151) -- by ops.lmeds_essential_pose; returns (M, errors, mask2, E) like
    recover_camera_five_point.  LMedS takes no threshold.  ``if_normalized``: focal 1 and principal point (0, 0) for the pose step
    (and, with five_point, for the estimate).  A pair without a pose gets the identity, (180, 90) and an all-False mask."""
    dev = torch.device("cuda")
    m = torch.as_tensor(np.hstack((np.asarray(x1), np.asarray(x2))), dtype=torch.float32, device=dev).unsqueeze(0).contiguous()
    Kt = torch.as_tensor(np.asarray(K, dtype=np.float64), dtype=torch.float32, device=dev).reshape(1, 3, 3)
    eye = torch.eye(3, device=dev).reshape(1, 3, 3)
    if five_point:
        out = ops.lmeds_essential_pose(m, eye if if_normalized else Kt)
    else:
        out = ops.lmeds_pose(m, Kt, K_pose=eye if if_normalized else recover_pose_camera(Kt))
    Rt_cam = out["Rt_cam"]
    mask2 = out["in_front"][0].cpu().numpy() > 0
    if int(out["winner"][0].item()) < 0:
        M = np.hstack((np.eye(3), np.zeros((3, 1))))
        err = FAILED
    else:
        err = _pose_errors(Rt_cam[0], delta_Rtij_inv)
        R = Rt_cam[0, :, :3].t()
        t = -(R @ Rt_cam[0, :, 3].reshape(3, 1))
        M = torch.cat((R, t), 1).cpu().double().numpy()
    if show_result:
        print("Recovered by OpenCV %s (camera): The rotation error (degree) %.4f, and translation error (degree) %.4f"
              % (("5 point" if five_point else "8 point") + " LMedS" + method_app, err[0], err[1]))
    E = out["E"][0].cpu().double().numpy()
    return M, err, mask2, (E if five_point else (E, out["F"][0].cpu().double().numpy()))


def KNN_match(des1, des2, x1_all, x2_all, kp1, kp2, img1_rgb, img2_rgb, visualize=False, if_BF=False, if_ratio_test=True):
    """Same call and return as the reference (utils_opencv.py:39-90), numpy in and out: (x1 [n,2], x2 [n,2], all_ij [N1,2],
    good_ij [n,2]) from one launch.  des1 [N1,D], des2 [N2,D] (D a multiple of 32; SIFT: 128); the ratio is the reference's 0.8,
    evaluated as its Python line does (float64).  ``if_BF`` is accepted and ignored: the search is always the exact one (module
    docstring).  ``kp1``, ``kp2``, ``img1_rgb``, ``img2_rgb`` are accepted and unused; ``visualize=True`` needs cv2 and
    matplotlib and raises NotImplementedError.  N2 < 2 raises ValueError like the reference's ``for m, n in matches``."""
    if visualize:
        raise NotImplementedError("KNN_match(visualize=True): drawing the matches needs cv2 and matplotlib, which are not used here")
    des1, des2 = np.asarray(des1, dtype=np.float32), np.asarray(des2, dtype=np.float32)
    x1_all, x2_all = np.asarray(x1_all), np.asarray(x2_all)
    N1 = des1.shape[0]
    if N1 == 0:
        empty = np.zeros((0, 2), dtype=np.int64)
        return x1_all[:0], x2_all[:0], empty, empty.copy()
    dev = torch.device("cuda")
    out = ops.knn_match(torch.tensor(des1, device=dev).unsqueeze(0), torch.tensor(des2, device=dev).unsqueeze(0), ratio=0.8,
                        ratio_test=bool(if_ratio_test))
    nn1, m1, m2 = (out[k][0].cpu().numpy().astype(np.int64) for k in (0, 4, 5))
    cnt = int(out[7][0].item())
    good_ij = np.stack((m1[:cnt], m2[:cnt]), axis=1)
    all_ij = np.stack((np.arange(N1, dtype=np.int64), nn1), axis=1)
    x1, x2 = x1_all[good_ij[:, 0], :], x2_all[good_ij[:, 1], :]
    print("# good points: %d/(%d, %d)" % (cnt, des1.shape[0], des2.shape[0]))
    return x1, x2, all_ij, good_ij


def KNN_match_batch(des1, des2, x1_all, x2_all, ratio=0.8, out_num_points=None):
    """KNN_match for a whole batch on the device: des1 [B,N1,D], des2 [B,N2,D], x1_all [B,N1,2], x2_all [B,N2,2] tensors.
    Returns the dict of ops.knn_match's outputs (nn1, nn2, dist1, dist2, m_idx1, m_idx2, score, count).  With ``out_num_points``
    it also holds xs [B,n,4] and quality [B,n,2] = (distance, dist1 / dist2) of the good matches cropped or padded to n per pair:
    the permutation is drawn on the host by utils_misc.crop_or_pad_choice (numpy's RNG, as matches_from_SP_outputs does) and
    gathered by ops.gather_matches.  A pair without a good match cannot be padded: crop_or_pad_choice's error propagates."""
    from .utils_misc import crop_or_pad_choice

    nn1, nn2, dist1, dist2, m1, m2, sc, cnt = ops.knn_match(des1, des2, ratio=ratio, ratio_test=True)
    out = {"nn1": nn1, "nn2": nn2, "dist1": dist1, "dist2": dist2, "m_idx1": m1, "m_idx2": m2, "score": sc, "count": cnt}
    if out_num_points is None:
        return out
    counts = cnt.cpu().numpy()
    choice = np.stack([crop_or_pad_choice(int(n), out_num_points, shuffle=True) for n in counts]).astype(np.int32)
    choice_dev = torch.from_numpy(choice).to(m1.device)
    xs, _, q = ops.gather_matches(x1_all, x2_all, None, None, m1, m2, sc, choice_dev)
    rows = torch.gather(m1, 1, choice_dev.long()).long()  # every position of choice is below the pair's count
    out["xs"] = xs
    out["quality"] = torch.cat((q, torch.gather(dist1 / dist2, 1, rows).unsqueeze(-1)), dim=2)
    return out


# ---- cv2.findHomography ------------------------------------------------------------------------------------------------------
RANSAC, LMEDS, RHO = 8, 4, 16  # cv2's method constants


def findHomography_batch(matches, n_valid=None, method=RANSAC, ransacReprojThreshold=3.0, maxIters=2000, confidence=0.995, seed=0):
    """cv2.findHomography for B pairs on the device: matches [B,N,4] (x1, y1, x2, y2), n_valid [B] int32 or None ->
    (H [B,3,3] float64, zeros where cv2 returns None; mask [B,N] uint8; found [B] bool).  No host synchronisation."""
    if method not in (0, RANSAC):
        raise NotImplementedError(f"findHomography: method {method} (LMEDS = 4 and RHO = 16 are not built; 0 and RANSAC = 8 are)")
    out = ops.ransac_homography(matches, n_valid, ransacReprojThreshold, confidence, maxIters, seed, all_points=(method == 0))
    return out["H"], out["mask"], out["n_inliers"] > 0


def findHomography(srcPoints, dstPoints, method=RANSAC, ransacReprojThreshold=3.0, maxIters=2000, confidence=0.995, seed=0):
    """cv2.findHomography(srcPoints, dstPoints, method, ransacReprojThreshold, maxIters=, confidence=) with cv2's layout, numpy in
    and out: points [N,2] (or [N,1,2]) -> (H float64 [3,3] or None when there is no model, mask uint8 [N,1]).  method 0 (least
    squares over all points) and 8 (RANSAC) are built; LMEDS (4) and RHO (16) raise NotImplementedError.  What differs from
    OpenCV: the random stream (`seed`; include/dfepe.h, dfepe_ransac_homography), so results agree with cv2's in distribution,
    not bit for bit.  evaluations/descriptor_evaluation.py:93, deepFEPE/evaluate_frontend.py:234."""
    if method not in (0, RANSAC):
        raise NotImplementedError(f"findHomography: method {method} (LMEDS = 4 and RHO = 16 are not built; 0 and RANSAC = 8 are)")
    src = np.asarray(srcPoints, dtype=np.float32).reshape(-1, 2)
    dst = np.asarray(dstPoints, dtype=np.float32).reshape(-1, 2)
    if src.shape != dst.shape:
        raise ValueError(f"srcPoints and dstPoints must hold the same number of points, got {src.shape} and {dst.shape}")
    N = src.shape[0]
    if N < 4:
        return None, np.zeros((N, 1), dtype=np.uint8)
    m = torch.as_tensor(np.ascontiguousarray(np.hstack((src, dst))), device=torch.device("cuda")).unsqueeze(0)
    H, mask, found = findHomography_batch(m, None, method, ransacReprojThreshold, maxIters, confidence, seed)
    mask = mask[0].cpu().numpy().reshape(N, 1)
    return (H[0].cpu().numpy() if bool(found[0]) else None), mask
