"""ctypes binding of libdfepe_hip.so (the C ABI declared in include/dfepe.h).

The library is the product: there is no CPU fallback.  `lib()` raises if the shared object is
missing, so a GPU box without the HIP extension fails loudly instead of silently running something else.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_double, c_float, c_int, c_long, c_size_t, c_uint, c_ulonglong, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# DFEPE_LIB_PATH: another build of the same library (scripts/ab_step.sh times two builds alternately on one box)
LIB_PATH = os.environ.get("DFEPE_LIB_PATH") or os.path.join(_HERE, "libdfepe_hip.so")

OK = 0
W8PT_RAW_MATCHES = 1
W8PT_LOGITS = 2
W8PT_SQRT2 = 4
W8PT_NO_ROWNORM = 8
W8PT_FORCE_110 = 16
W8PT_NO_HARTLEY = 32
W8PT_ROW_PER_PAIR = 64
W8PT16_MAX_N = 128
HARTLEY_DOUBLES = 8  # dfepe_w8pt_fwd_shared: doubles per pair in the Hartley record (64-byte aligned)
HARTLEY_NONE, HARTLEY_WRITE, HARTLEY_READ = 0, 1, 2  # ... and its modes
TAIL_MAX_LAYERS = 16  # dfepe_loss_tail: layers per launch (kTailMaxLayers, csrc/loss_tail_body.h)
EPI_HOMOGENEOUS = 8
CHEIR_FP64_ONLY = 1
RANSAC_MIN_N = 15  # dfepe_ransac_fundamental: below, OpenCV switches to LMedS (dfepe_lmeds_fundamental)
POSE_CHAIN_THREADS = 256  # dfepe_pose_chain: lanes per sequence (kChainThreads, csrc/odometry.hip)
POSE_CHAIN_CHUNK = 8  # ... and consecutive poses per lane and tile (kChainChunk): a tile is 2048 poses
SNIPPET_MAX_L = 64  # dfepe_snippet_errors: longest snippet (kSnipMaxL)
TRAJ_MODES = ("none", "scale", "scale_7dof", "7dof", "6dof")  # dfepe_trajectory_align: mode = index (DFEPE_TRAJ_*, traj::Mode)
KITTI_DIST_LDS = 4096  # dfepe_kitti_odometry_errors: frames whose path length stays in LDS (kDistLds, csrc/trajectory.hip)
LMEDS_MIN_N = 8  # dfepe_lmeds_fundamental: N = 7 is OpenCV's direct 7-point path (not built)
LMEDS5_MIN_N = 6  # dfepe_lmeds_essential
POSE_CAMERA_MOTION = 1  # dfepe_two_view_structure / dfepe_reproject: Rt is camera motion (DFEPE_POSE_CAMERA_MOTION)
RANSAC5_MIN_N = 6  # dfepe_ransac_essential: with 5 OpenCV returns the stacked models of the one sample (not built)
HOMOGRAPHY_ALL_POINTS = 1  # dfepe_ransac_homography: cv2's method = 0 (DFEPE_HOMOGRAPHY_ALL_POINTS)
HOMOGRAPHY_NO_REFINE = 2  # ... no Levenberg-Marquardt step (DFEPE_HOMOGRAPHY_NO_REFINE)
HOMOGRAPHY_MAX_N = 4096
DETECTOR_EVAL_MAX_N = 4096  # dfepe_keypoint_repeatability (points per image), dfepe_average_precision (entries per pair): de::kMaxN
SP_MAX_PIXELS = 1 << 24  # dfepe_sp_*: pixels per image (sp::kMaxPixels, csrc/sp_process_math.h)
SP_LDS_PIXELS = 12288  # dfepe_sp_nms: pixels per image up to which no workspace is needed (sp::kLdsPixels)
SP_MAX_PATCH = 63  # dfepe_sp_soft_argmax: largest patch_size (sp::kMaxPatch)
DSAC_MIN_SAMPLE, DSAC_MAX_SAMPLE = 8, 16  # dfepe_dsac: correspondences per hypothesis (ds::kMinSample, ds::kMaxSample)
SAMPLER_MAX_WEIGHTED_N = 1 << 20  # dfepe_sample_sets: correspondences per pair in weighted mode (sm::kMaxWeightedN)
SAMPLE_MIN_DRAWS, SAMPLE_MAX_DRAWS = 8, 32  # dfepe_sample_multisets: draws per set (sl::kMinDraws, sl::kMaxDraws)
INLIER_TABLE_MAX_THDS = 16  # dfepe_inlier_table: inlier thresholds per call, and mask thresholds per call (ce::kMaxThds)

_P = c_void_p
_SIGNATURES = {
    "dfepe_version": (c_int, []),
    "dfepe_strerror": (c_char_p, [c_int]),
    "dfepe_save_floats": (c_int, []),
    "dfepe_selftest_rowgroup": (c_int, [_P, _P, _P, _P]),
    "dfepe_w8pt_fwd": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_uint, c_float, c_float, c_float, _P, _P, _P, _P, _P, _P]),
    "dfepe_w8pt_fwd_shared": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_uint, c_float, c_float, c_float, _P, _P, _P, _P, _P, _P, c_int, _P]),
    "dfepe_w8pt_shares_hartley": (c_int, [c_int, c_uint]),
    "dfepe_w8pt_bwd": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_uint, c_float, c_float, c_float, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "dfepe_w8pt_rows_fwd": (c_int, [_P, c_int, c_int, c_uint, _P, _P, _P, _P]),
    "dfepe_floss_fwd": (c_int, [_P, c_int, c_int, _P, _P, c_int, _P, _P, _P, c_int, c_float, _P, _P, _P]),
    "dfepe_floss_bwd": (c_int, [_P, c_int, c_int, _P, _P, c_int, _P, _P, _P, c_int, c_float, _P, c_float, _P, _P, _P, _P]),
    "dfepe_pose_fwd": (c_int, [_P, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "dfepe_pose_bwd": (c_int, [_P, c_int, c_int, _P, _P, _P, _P, c_float, c_float, c_float, c_float, _P, _P, _P]),
    "dfepe_loss_head": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_float, c_float, c_float, c_float, _P, _P, _P]),
    "dfepe_loss_tail_workspace_bytes": (c_size_t, [c_int]),
    "dfepe_loss_tail": (c_int, [_P, c_int, c_int, _P, _P, c_int, _P, _P, _P, c_int, c_float, _P, _P, _P, c_float, c_float, c_float, c_float,
                                c_float, c_double, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, _P]),
    "dfepe_loss_head_pending": (c_int, [_P, _P]),
    "dfepe_loss_tail_jac": (c_int, [_P, c_int, c_int, _P, _P, c_int, _P, _P, _P, c_int, c_float, _P, _P, _P, c_int, _P, _P, _P, _P, _P, _P, _P,
                                    _P, _P]),
    "dfepe_loss_tail_bwd": (c_int, [_P, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_float, _P, _P]),
    "dfepe_loss_stats": (c_int, [_P, c_int, c_float, _P, c_int, c_float, _P, c_int, c_float, _P, c_int, c_float, c_int, _P, _P, _P, _P]),
    "dfepe_deepf_input": (c_int, [_P, _P, c_int, c_int, c_int, c_float, c_float, _P, c_size_t, c_size_t, c_int, c_size_t, _P, _P, _P]),
    "dfepe_row_dot": (c_int, [_P, c_size_t, _P, c_size_t, c_int, c_int, c_int, _P, _P]),
    "dfepe_cheirality": (c_int, [_P, _P, _P, _P, c_int, c_int, c_float, _P, _P, _P, _P]),
    "dfepe_cheirality_workspace_bytes": (c_size_t, [c_int]),
    "dfepe_cheirality_ex": (c_int, [_P, _P, _P, _P, c_int, c_int, c_float, c_uint, _P, _P, _P, _P, _P]),
    "dfepe_w8pt_pose_fwd": (c_int, [_P, _P, c_int, c_int, c_uint, c_float, c_float, c_float, _P, _P, c_float, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "dfepe_metrics_summary_bytes": (c_size_t, []),
    "dfepe_metrics_summary": (c_int, [_P, _P, c_size_t, _P, _P, c_int, _P, _P]),
    "dfepe_epi_metrics": (c_int, [c_int, _P, _P, _P, c_int, c_int, c_float, c_float, _P, _P]),
    "dfepe_epi_residual_fwd": (c_int, [_P, _P, _P, c_int, c_int, c_float, _P, _P]),
    "dfepe_epi_residual_bwd": (c_int, [_P, _P, _P, c_int, c_int, c_float, _P, _P, _P]),
    "dfepe_geo_misc": (c_int, [c_int, _P, _P, c_int, _P, _P]),
    "dfepe_inorm_lrelu_fwd": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_float, c_float, _P, _P, _P]),
    "dfepe_inorm_lrelu_bwd": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_float, _P, _P, _P, _P]),
    "dfepe_est_points": (c_int, []),
    "dfepe_est_split": (c_int, [_P, c_long, c_int, c_int, c_int, c_int, _P, c_size_t, _P]),
    "dfepe_est_absmax": (c_int, [_P, c_long, _P, _P]),
    "dfepe_est_wprep_workspace_bytes": (c_size_t, [c_int]),
    "dfepe_est_wprep": (c_int, [c_int, _P, _P, _P, _P, _P, _P, _P, _P]),
    "dfepe_est_colsum": (c_int, [c_int, _P, _P, _P, _P, _P]),
    "dfepe_est_split_f16": (c_int, [_P, c_long, c_int, c_int, c_int, _P, _P, c_size_t, _P]),
    "dfepe_est_layer_fwd": (c_int, [_P, c_size_t, _P, c_size_t, c_int, c_int, c_int, _P, _P, _P, c_float, c_float, _P, c_size_t, _P, c_size_t, _P, _P]),
    "dfepe_est_gemm_nt_f16": (c_int, [_P, c_size_t, _P, c_size_t, c_int, c_int, c_int, _P, _P, c_int, _P]),
    "dfepe_est_gemm_nt": (c_int, [_P, c_size_t, _P, c_size_t, c_int, c_int, c_int, c_int, _P, c_int, _P]),
    "dfepe_est_gemm_tn": (c_int, [_P, c_size_t, c_int, _P, c_size_t, c_int, c_int, c_int, _P, _P]),
    "dfepe_est_in_bwd": (c_int, [_P, _P, _P, _P, c_size_t, _P, _P, _P, c_float, c_int, c_int, _P, c_size_t, _P, _P, _P]),
    "dfepe_est_dgamma_zero": (c_int, [_P, _P, _P, _P, c_size_t, _P, c_size_t, _P, c_int, c_int, _P, _P, c_float, c_int, c_int, c_long, _P, _P,
                                      c_size_t, _P, c_int, c_int, _P]),
    "dfepe_est_dgamma_zero_multi": (c_int, [c_int] + [_P] * 17 + [c_float, c_int, c_long, _P]),
    "dfepe_est_dgrad_in_bwd": (c_int, [_P, c_size_t, _P, c_size_t, c_int, c_int, c_int, _P, c_size_t, _P, _P, _P, c_float, _P, c_size_t, _P, _P, _P]),
    "dfepe_est_norm_fwd": (c_int, [_P, c_int, c_int, c_long, c_int, _P, _P, c_float, c_float, _P, c_size_t, _P, c_size_t, _P, c_int, _P, _P]),
    "dfepe_est_in_bwd_n": (c_int, [_P, _P, _P, _P, c_size_t, _P, _P, _P, c_float, c_int, c_long, c_int, _P, c_size_t, _P, _P, c_int, _P, _P]),
    "dfepe_est_saved_bytes": (c_size_t, [c_int, _P, _P, c_long, c_int, c_int, c_int]),
    "dfepe_est_forward_workspace_bytes": (c_size_t, [c_int, _P, _P, c_long, c_int, c_int, c_int]),
    "dfepe_est_backward_workspace_bytes": (c_size_t, [c_int, _P, _P, c_long, c_int, c_int, c_int]),
    "dfepe_est_forward": (c_int, [_P, c_long, c_long, c_long, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, c_float, c_float, _P, c_int, _P, _P, _P, _P]),
    "dfepe_est_backward": (c_int, [_P, c_long, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, c_float, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_long, c_long, _P]),
    "dfepe_est_head_fwd": (c_int, [_P, c_size_t, c_int, c_int, _P, _P, _P, _P]),
    "dfepe_est_head_dw": (c_int, [_P, c_size_t, c_int, c_int, c_int, _P, _P, _P, _P]),
    "dfepe_est_gemm_nt_f16_splitk": (c_int, [_P, c_size_t, _P, c_size_t, c_int, c_int, c_int, _P, _P, c_int, c_int, c_size_t, _P]),
    "dfepe_est_gemm_nt_splitk": (c_int, [_P, c_size_t, _P, c_size_t, c_int, c_int, c_int, _P, c_int, c_int, c_size_t, _P]),
    "dfepe_est_gemm_nt_gx": (c_int, [_P, c_size_t, _P, c_size_t, c_int, c_int, c_int, _P, c_int, c_int, c_long, c_long, _P]),
    "dfepe_est_gemm_tn_multi": (c_int, [c_int, _P, _P, _P, _P, _P, _P, c_int, _P, _P, _P]),
    "dfepe_est_norm_fwd_r": (c_int, [_P, c_int, c_int, c_size_t, c_int, c_long, c_int, _P, _P, c_float, c_float, _P, c_size_t, _P, c_size_t, _P, _P]),
    "dfepe_est_in_bwd_r": (c_int, [_P, c_int, c_int, c_size_t, _P, _P, _P, c_size_t, _P, _P, _P, c_float, c_int, c_long, c_int, _P, c_size_t, _P, _P, _P]),
    "dfepe_est_prep_bytes": (c_size_t, [c_int, _P, _P]),
    "dfepe_est_prepare": (c_int, [c_int, _P, _P, _P, _P, _P]),
    "dfepe_nn_match_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dfepe_nn_match_two_way": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_float, _P, _P, _P, _P, _P, _P]),
    "dfepe_gather_matches": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, _P, _P, _P, _P, c_int, _P, _P, _P, _P]),
    "dfepe_knn_match_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dfepe_knn_match": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_double, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "dfepe_ransac_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dfepe_ransac_fundamental": (c_int, [_P, c_int, c_int, c_double, c_double, c_int, c_ulonglong, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "dfepe_ransac_in_front": (c_int, [_P, _P, _P, c_int, c_int, c_float, _P, _P, _P]),
    "dfepe_ransac5_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dfepe_ransac_essential": (c_int, [_P, _P, c_int, c_int, c_double, c_double, c_int, c_ulonglong, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "dfepe_lmeds_num_iters": (c_int, [c_int, c_double, c_int]),
    "dfepe_lmeds_workspace_bytes": (c_size_t, [c_int, c_int, c_double, c_int]),
    "dfepe_lmeds_fundamental": (c_int, [_P, c_int, c_int, c_double, c_int, c_ulonglong, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "dfepe_lmeds_essential": (c_int, [_P, _P, c_int, c_int, c_double, c_int, c_ulonglong, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "dfepe_correct_matches": (c_int, [_P, _P, c_long, _P, _P, c_int, c_int, _P, _P, _P]),
    "dfepe_pose_chain": (c_int, [_P, _P, _P, _P, c_long, c_int, c_int, _P]),
    "dfepe_snippet_errors": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P]),
    "dfepe_trajectory_align": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, _P, _P, _P]),
    "dfepe_kitti_odometry_errors": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P]),
    "dfepe_triangulate": (c_int, [_P, c_int, _P, c_int, _P, c_int, c_int, _P, _P]),
    "dfepe_two_view_structure": (c_int, [_P, c_uint, _P, _P, c_int, c_int, _P, _P, c_float, _P, _P, _P, _P]),
    "dfepe_reproject": (c_int, [_P, _P, c_int, c_uint, _P, c_int, c_int, c_int, c_float, c_float, _P, _P, _P, _P]),
    "dfepe_homography_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dfepe_ransac_homography": (c_int, [_P, _P, c_int, c_int, c_double, c_double, c_int, c_ulonglong, c_uint, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "dfepe_homography_transfer": (c_int, [_P, _P, _P, c_int, c_int, c_double, _P, _P, _P]),
    "dfepe_homography_corners": (c_int, [_P, _P, c_int, c_int, c_int, _P, c_int, _P, _P, _P]),
    "dfepe_keypoint_repeatability_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dfepe_keypoint_repeatability": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P, c_int, _P, _P, _P, _P, _P,
                                             _P, _P, _P, _P]),
    "dfepe_average_precision": (c_int, [_P, _P, _P, c_int, c_int, _P, _P, _P, _P, _P]),
    "dfepe_matching_score": (c_int, [_P, _P, _P, c_int, _P, _P]),
    "dfepe_sp_nms_capacity": (c_int, [c_int, c_int, c_int]),
    "dfepe_sp_nms_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dfepe_sp_soft_argmax_bwd_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "dfepe_sp_flatten": (c_int, [_P, c_int, c_int, c_int, _P, _P]),
    "dfepe_sp_flatten_bwd": (c_int, [_P, _P, c_int, c_int, c_int, _P, _P]),
    "dfepe_sp_nms": (c_int, [_P, c_int, c_int, c_int, c_float, c_int, c_int, _P, _P, _P, _P, _P, _P]),
    "dfepe_sp_soft_argmax": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P, _P]),
    "dfepe_sp_soft_argmax_bwd": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P, _P]),
    "dfepe_sp_sample_desc": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P]),
    "dfepe_gather_offsets_bwd": (c_int, [_P, c_int, c_int, c_int, _P, _P, _P, c_int, _P, _P, _P]),
    "dfepe_inlier_table": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, _P, c_int, _P, c_int, _P, _P, _P, _P, _P]),
    "dfepe_inlier_table_mean": (c_int, [_P, _P, c_int, c_int, c_int, _P, _P, _P]),
    "dfepe_epi_adjoint_chunk": (c_int, []),
    "dfepe_epi_adjoint_workspace_bytes": (c_size_t, [c_int, c_int]),
    "dfepe_epi_metrics_bwd": (c_int, [_P, c_int, _P, _P, _P, c_int, c_int, c_float, c_float, _P, _P, _P, _P, _P]),
    "dfepe_epi_residual_bwd_pts": (c_int, [_P, _P, _P, _P, c_int, c_int, c_float, _P, _P, _P]),
    "dfepe_epi_loss_fwd": (c_int, [_P, c_int, _P, _P, _P, _P, c_int, c_int, c_float, c_float, _P, _P]),
    "dfepe_epi_loss_bwd": (c_int, [_P, c_int, _P, _P, _P, _P, c_int, c_int, c_float, c_float, _P, _P, _P, _P, _P, _P]),
    "dfepe_dsac_hyps_per_block": (c_int, []),
    "dfepe_dsac_vote_chunk": (c_int, []),
    "dfepe_dsac_vote_tile": (c_int, []),
    "dfepe_dsac_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "dfepe_dsac": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_float, c_float, c_float, c_int] + [_P] * 12),
    "dfepe_eight_point_bwd_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dfepe_eight_point_bwd": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_uint, _P, _P, _P, _P, _P, _P]),
    "dfepe_dsac_bwd_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "dfepe_dsac_bwd": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_float, c_float, c_float, c_int] + [_P] * 20),
    "dfepe_sampler_scan_chunk": (c_int, []),
    "dfepe_sample_sets_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dfepe_sample_sets": (c_int, [_P, c_int, c_int, c_int, c_int, c_ulonglong, c_uint, _P, _P, _P, _P, _P, _P]),
    "dfepe_sampler_advance": (c_int, [_P, _P, c_uint]),
    "dfepe_sample_loss_max_virt": (c_int, []),
    "dfepe_sample_scatter_chunk": (c_int, []),
    "dfepe_sample_multisets": (c_int, [_P, c_int, c_int, c_int, c_int, c_ulonglong, c_uint, _P, _P, _P, _P, _P, _P]),
    "dfepe_topk_select": (c_int, [_P, _P, _P, c_int, c_int, c_int, _P, _P]),
    "dfepe_sample_gather": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P]),
    "dfepe_sample_floss_fwd": (c_int, [_P, _P, c_int, c_int, _P, _P, c_int, _P, _P, c_int, c_float, _P]),
    "dfepe_sample_floss_bwd": (c_int, [_P, _P, c_int, c_int, _P, _P, c_int, _P, _P, c_int, c_float, _P, _P]),
    "dfepe_sample_scatter_bwd": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None


class DfepeError(RuntimeError):
    pass


def lib() -> ctypes.CDLL:
    """Load (once) and return the HIP library; raises DfepeError when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DfepeError(
                f"{LIB_PATH} is missing: the HIP extension has not been built "
                "(run `python pytorch-deepfepe_amd/build.py` or `__graft_entry__.build()`); there is no CPU fallback"
            )
        l = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(code: int, what: str) -> None:
    if code != OK:
        msg = lib().dfepe_strerror(code).decode()
        raise DfepeError(f"{what} failed: {msg} (code {code})")
