"""Mirror of deepFEPE.dsac_tools.utils_opencv: the OpenCV 8-point RANSAC baseline of the validation (recover_camera_opencv,
utils_opencv.py:129-208), backed by the batched RANSAC estimator of libdfepe_hip.so (ops.ransac_pose) instead of cv2.

What differs from OpenCV: the random stream (include/dfepe.h, dfepe_ransac_fundamental), so results agree with cv2's in
distribution, not bit for bit.  The five-point baseline (cv2.findEssentialMat, Nister's solver) is recover_camera_five_point,
backed by ops.ransac_essential_pose; recover_camera_opencv(five_point=True) itself still raises.  Not built: LMedS (OpenCV's
choice for fewer than 15 correspondences of the 8-point branch)."""
import numpy as np
import torch

from .. import ops

BASELINE_THRESHOLD = 0.1  # the reference's 8-point branch passes 0.1 to findFundamentalMat whatever `threshold` says (:157)
FIVE_POINT_THRESHOLD = 0.01  # what val_rt passes to the five-point branch, which uses it (train_good_utils.py:622)
FAILED = (180.0, 90.0)    # the pose-error values of a pair without a pose (utils_F.goodCorr_eval_nondecompose, utils_F.py:942-952)


def recover_pose_camera(K):
    """K [B,3,3] (device) -> the camera the reference hands cv2.recoverPose: focal K[0,0], principal point (K[0,2], K[1,2])
    (utils_opencv.py:177)."""
    Kp = torch.zeros_like(K)
    Kp[:, 0, 0] = Kp[:, 1, 1] = K[:, 0, 0]
    Kp[:, 0, 2], Kp[:, 1, 2], Kp[:, 2, 2] = K[:, 0, 2], K[:, 1, 2], 1.0
    return Kp


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
