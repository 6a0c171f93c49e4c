"""torch.autograd wrappers over the C ABI (device memory and streams come from PyTorch-ROCm; the
arithmetic is entirely in libdfepe_hip.so).

One module per kernel family, named after the csrc files it binds; this file only collects their names, so that callers keep
writing ``ops.<name>``.  The modules import from ``_base`` (and ``robust`` from ``geometry``, ``loss`` and ``geometry`` from
``fit``), never from here.  tests/test_ops_split_cpu.py holds the list below to what the modules define."""
from .. import _lib  # noqa: F401
from ._base import Tensor, _on, _on_gpu, _prep, _ptr, _shape, _stream, _workspace  # noqa: F401
from .dsac_loop import DSAC_LOSS_KINDS, dsac, dsac_bwd  # noqa: F401
from .epipolar import epi_loss, epi_metrics, epi_residual  # noqa: F401
from .evaluation import (INLIER_TABLE_OUTPUTS, METRIC_THS, average_precision, inlier_table, inlier_table_mean,  # noqa: F401
                         keypoint_repeatability, kitti_odometry_errors, matching_score, metrics_summary, pose_chain, snippet_errors,
                         trajectory_align)
from .fit import (alias_rows, eight_point, eight_point_rows, hartley_record, row_of, save_floats, stack_rows, unstack_rows,  # noqa: F401
                  w8pt, w8pt_backward, w8pt_forward, w8pt_raw, w8pt_raw_logits)
from .geometry import (camera_rotation, cheirality, congruence, congruence_diff, decompose_essential, deepf_input,  # noqa: F401
                       estimator_input, fit_pose, geo_misc, project_essential, rot_angle_deg, rot_to_quat, row_dot, vector_angle_deg)
from .inorm import inorm_lrelu  # noqa: F401
from .loss import _floss_args, _t_arg, floss, loss_stats, loss_tail_jac, pose_errors, pose_errors_packed  # noqa: F401
from .matching import gather_matches, knn_match, nn_match_two_way  # noqa: F401
from .robust import (_recover_pose_camera, homography_corners, homography_transfer, lmeds_essential, lmeds_essential_pose,  # noqa: F401
                     lmeds_fundamental, lmeds_pose, ransac_essential, ransac_essential_pose, ransac_fundamental, ransac_homography,
                     ransac_in_front, ransac_pose)
from .sample_loss import sample_fits, sample_floss, sample_gather, sample_multisets, sample_scatter_bwd, topk_select  # noqa: F401
from .sampler import sample_sets, sampler_advance  # noqa: F401
from .structure import correct_matches, reproject, triangulate, two_view_structure  # noqa: F401
from .superpoint import sp_flatten, sp_nms, sp_nms_capacity, sp_sample_desc, sp_soft_argmax  # noqa: F401
