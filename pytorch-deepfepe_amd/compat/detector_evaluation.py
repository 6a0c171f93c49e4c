"""Mirror of the reference's detector evaluation, evaluations/detector_evaluation.py: compute_repeatability (lines 150-279),
backed by ops.keypoint_repeatability (libdfepe_hip.so) instead of numpy over an N1 x N2 distance matrix.

What differs from the reference: the input is not mutated (the reference overwrites the caller's data['prob'][:, :2] with the
warped points, line 228); the print calls, `verbose` included, are not mirrored; among equal probabilities at the k-th place
select_k_best keeps the higher index (the rule of a stable argsort; numpy's default argsort, which the reference calls, leaves
that choice undefined); the inverse warp uses the adjugate of H, the same projective map as numpy.linalg.inv(H).  Not built:
the dense-map precision / recall curves (compute_tp_fp, compute_pr, compute_loc_error, compute_mAP) and drawing."""
import numpy as np
import torch

from .. import ops
from .descriptor_evaluation import warp_keypoints  # noqa: F401  (the reference defines it in this module)


def compute_repeatability_batch(kp1, kp2, H, shape, keep_k_points=300, distance_thresh=(3.0,), n1=None, n2=None):
    """B image pairs on the device: kp1 [B,N1,C], kp2 [B,N2,C] rows (x, y[, prob]) of data['prob'] and data['warped_prob'], C in
    {2, 3}; H [B,3,3]; shape = (height, width) of the image; distance_thresh: a sequence of T thresholds (or a [T] tensor on the
    device); n1, n2 [B] int32 on the device or None (the valid rows of each pair).  Returns the dict of ops.keypoint_repeatability:
    repeatability and loc_err [B,T] float64 (0 and -1 where nothing is counted), count1, count2, kept1, kept2, n_unwarped.  No host
    synchronisation."""
    th = distance_thresh if torch.is_tensor(distance_thresh) else torch.as_tensor([float(v) for v in distance_thresh], dtype=torch.float64,
                                                                                 device=kp1.device)
    return ops.keypoint_repeatability(kp1, kp2, H, int(shape[0]), int(shape[1]), int(keep_k_points), th, n1, n2)


def compute_repeatability(data, keep_k_points=300, distance_thresh=3, verbose=False):
    """evaluations/detector_evaluation.compute_repeatability with the reference's signature: data holds 'prob' and 'warped_prob'
    [N,2 or 3] rows (x, y[, prob]), 'homography' [3,3] and 'image' (only its shape (h, w) is read).  Returns (repeatability,
    localization_err), (0, -1) when nothing is counted -- in particular when either set is empty.  `data` is left unchanged, unlike
    in the reference; `verbose` prints nothing."""
    dev = torch.device("cuda")
    p1, p2 = np.asarray(data["prob"], dtype=np.float64), np.asarray(data["warped_prob"], dtype=np.float64)
    C = p1.shape[1] if p1.ndim == 2 and p1.shape[0] else (p2.shape[1] if p2.ndim == 2 and p2.shape[0] else 2)
    C = 3 if C > 2 else 2
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a.reshape(a.shape[0], -1)[:, :C] if a.shape[0] else np.zeros((0, C))),  # noqa: E731
                                  device=dev).unsqueeze(0)
    shape = np.asarray(data["image"]).shape
    H = torch.as_tensor(np.asarray(data["homography"], dtype=np.float64), device=dev).unsqueeze(0)
    out = compute_repeatability_batch(t(p1), t(p2), H, shape, keep_k_points, [float(distance_thresh)])
    count = int(out["count1"][0, 0]) + int(out["count2"][0, 0])
    if count == 0:
        return 0, -1
    return float(out["repeatability"][0, 0]), float(out["loc_err"][0, 0])
