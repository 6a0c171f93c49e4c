"""Mirror of the reference's Python call surface for the hot path: same class / function names,
argument order, defaults, return arity, tensor layouts and dict keys, backed by libdfepe_hip.so.

    reference module                         this package
    deepFEPE.models.DeepFNet            ->   compat.DeepFNet        (NormalizeAndExpand_HW, Fit, DeepFNet)
    deepFEPE.models.DeepFNetSampleLoss  ->   compat.DeepFNetSampleLoss (Fit with the top-K and sampled-set fits, Norm8PointNet: the
                                                                    if_sample_loss model; sets drawn on the stream or by NumPy)
    deepFEPE.models.ErrorEstimators     ->   compat.ErrorEstimators (stock PyTorch; not part of the hot path)
    deepFEPE.dsac_tools.utils_F         ->   compat.utils_F
    deepFEPE.dsac_tools.utils_geo       ->   compat.utils_geo
    deepFEPE.train_good_utils           ->   compat.train_good_utils (get_all_loss_DeepF, get_Rt_loss, get_matches_from_SP,
                                                                    get_loss_softmax: differentiable through the kernel's adjoint)
    deepFEPE.dsac_tools.H_loss          ->   compat.H_loss          (HLoss: the mean Sampson distance, differentiable likewise)
    deepFEPE.dsac_tools.utils_misc      ->   compat.utils_misc      (homogeneous / rigid-transform helpers, crop_or_pad_choice,
                                                                    get_virt_x1x2*: the F-loss's virtual points, no cv2)
    deepFEPE.dsac_tools.utils_opencv    ->   compat.utils_opencv    (recover_camera_opencv: the 8-point RANSAC baseline, no cv2;
                                                                    triangulatePoints in place of cv2.triangulatePoints)
                                                                    findHomography in place of cv2.findHomography)
    evaluations.descriptor_evaluation   ->   compat.descriptor_evaluation (compute_homography, homography_estimation; getInliers
                                                                    and getInliers_cv of deepFEPE/evaluate_frontend.py)
    evaluations.detector_evaluation     ->   compat.detector_evaluation (compute_repeatability, warp_keypoints)
    deepFEPE.evaluate_frontend          ->   compat.evaluate_frontend (matching score, nn mean AP, the five numbers per pair)
    deepFEPE.dsac_tools.utils_vis       ->   compat.utils_vis       (reproj_and_scatter without the drawing)
    deepFEPE.dsac_tools.dsac            ->   compat.dsac            (DSAC: the hypothesis loop in six launches; dsac_batch: a whole batch
                                                                    of pairs on the device; DeviceSampler: the minimal sets drawn on
                                                                    the stream, uniform or by weight)
    superpoint.models.model_wrap        ->   compat.model_wrap      (PointTracker: nn_match_two_way and the two-frame state)
    superpoint.models.model_utils,      ->   compat.superpoint_process (flattenDetection, SuperPointNet_process: what
    superpoint.utils.utils                                          process_SP_output calls; the network stays the caller's)
    deepFEPE.utils.eval_tools           ->   compat.eval_tools      (Exp_table_processor's odometry methods: get_abs_poses,
                                                                    compensate_poses, compute_pose_error, pose_seq_ate; plus
                                                                    relative_pose_cam_to_body and the on-device odometry_summary;
                                                                    Result_processor, the correspondence table)
    deepFEPE.evaluation_epiDist         ->   compat.evaluation_epiDist (epi_dist_from_matches, process_grey2tensor; the on-device
                                                                    correspondence_eval_batch)

    (no counterpart: the reference's agent is eager)  compat.CapturedStep  (its training step as one replayed hipGraph)

See INTEGRATION.md for how train_good.py is pointed at these.
"""
from . import DeepFNet, DeepFNetSampleLoss, ErrorEstimators, H_loss, captured, descriptor_evaluation, detector_evaluation, dsac, eval_tools, evaluate_frontend, evaluation_epiDist, model_wrap, superpoint_process, train_good_utils, utils_F, utils_geo, utils_misc, utils_opencv, utils_vis  # noqa: F401
from .captured import CapturedStep  # noqa: F401
from .descriptor_evaluation import compute_homography, compute_homography_batch, get_inliers, get_inliers_cv, homography_estimation, warp_keypoints  # noqa: F401
from .detector_evaluation import compute_repeatability, compute_repeatability_batch  # noqa: F401
from .dsac import DSAC, DeviceSampler, dsac_batch  # noqa: F401
from .evaluate_frontend import frontend_metrics_batch  # noqa: F401
from .evaluation_epiDist import correspondence_eval_batch  # noqa: F401
from .utils_opencv import findHomography, findHomography_batch  # noqa: F401
