"""Mirror of the correspondence evaluation of deepFEPE/evaluation_epiDist.py (run_eval_good.py --runCorr, :380-384, launches its
val_feature): epi_dist_from_matches (:276-326) and process_grey2tensor (:248-252) with the reference's signatures, and the batch
path the reference does not have, correspondence_eval_batch: from the two images' keypoints and descriptors to the table of
inlier ratios by match score without leaving the stream.

val_feature itself is a loop over a data loader around calls that all exist here: compat.model_wrap.PointTracker (update,
get_matches, get_mscores, clear_desc), epi_dist_from_matches below, and compat.eval_tools.Result_processor; INTEGRATION.md says
how the script is pointed at them."""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib, ops

Tensor = torch.Tensor


def process_grey2tensor(img, device="cpu"):
    """img [B,H,W] grey levels 0..255 -> float [B,1,H,W] in 0..1 on `device` (evaluation_epiDist.py:248-252)"""
    img = img.float().to(device) / 255.0
    img = img.unsqueeze(-1).permute(0, 3, 1, 2)
    return img


def epi_dist_from_matches(matches_use, sample, device, five_point=False):
    """matches_use np[1,N,4] (x1, y1, x2, y2), sample["F"] [batch,3,3] -> {"epi_dist_mean_gt": np[N] float32}: the distance dist3
    of epi_distance_np (dsac_tools/utils_F.py:363-385) of every match under the ground-truth F of the sample's first pair, which is
    the one value the reference keeps of val_rt's result (evaluation_epiDist.py:298-326).  One launch (dfepe_inlier_table with
    only dist_out): the pose errors val_rt also computes, and drops, are not computed.  The distance is evaluated in float64 and
    rounded once to float32 (the reference returns float64); `device` must be a GPU.  five_point is accepted and unused, as the
    value returned never depended on it."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.DfepeError("epi_dist_from_matches runs on the GPU (this package has no CPU path)")
    m = torch.as_tensor(np.ascontiguousarray(np.asarray(matches_use)[:1], np.float32)).to(dev)
    F = torch.as_tensor(sample["F"])[:1].to(dev, torch.float64)
    if m.shape[1] == 0:
        return {"epi_dist_mean_gt": np.zeros((0,), np.float32)}
    d = ops.inlier_table(matches=m, F=F, want=("dist_out",))["dist_out"]
    return {"epi_dist_mean_gt": d[0].cpu().numpy()}


def correspondence_eval_batch(pts, desc, F_gt, nn_thresh, inlier_thds, mask_thds=(1.0,), counts=None, noise=None) -> dict:
    """The correspondence table of B image pairs, on the device.
      pts        (pts1 [B,n1,2], pts2 [B,n2,2]) keypoints in pixels, e.g. from compat.superpoint_process
      desc       (desc1 [B,n1,D], desc2 [B,n2,D]) unit-norm descriptors, D a multiple of 32
      counts     None, or (count1 [B], count2 [B]) int32 on the device: the listed rows of each image.  The descriptors past a
                 count are zeroed here (sp_sample_desc already leaves them zero); a zero descriptor is at distance sqrt(2) from
                 everything, so nn_thresh must not exceed sqrt(2) when counts are given
      F_gt       [B,3,3] the ground-truth fundamental matrices
      nn_thresh  the tracker's threshold (PointTracker.nn_thresh)
      inlier_thds, mask_thds  1 .. 16 values each: device tensors, or host values that are uploaded (inside a graph capture pass
                 device tensors)
      noise      None or [B,n2,2]: added to pts2 before the matches are gathered (val_feature's rand_noise option,
                 evaluation_epiDist.py:166-170, with the noise drawn by the caller: the random stream stays the caller's)
    -> dict of device tensors: matches [B,n1,4] (x1, y1, x2, y2; zero rows past num_matches), mscores [B,n1], num_matches [B]
    int32, epi_dist_mean_gt [B,n1] float32 (0 past num_matches), cnt [B,Tm,Ti] int32, num [B,Tm] int32, ratio [B,Tm,Ti] float64,
    inlier_ratio [Tm,Ti] float64 (the mean over the pairs, NaN when a pair keeps nothing: Result_processor.inlier_ratio's value
    per mask threshold), num_corrs [Tm,B] int32.
    ops.nn_match_two_way -> ops.gather_matches (every position of the match list in order; the count stays on the device and
    becomes n_valid) -> ops.inlier_table -> ops.inlier_table_mean: no host copy, no synchronisation; capturable."""
    p1, p2 = pts
    d1, d2 = desc
    if not all(torch.is_tensor(t) and t.is_cuda for t in (p1, p2, d1, d2, F_gt)):
        raise _lib.DfepeError("correspondence_eval_batch takes tensors on the GPU (this package has no CPU path)")
    B, n1, n2 = p1.shape[0], p1.shape[1], p2.shape[1]
    if p1.shape != (B, n1, 2) or p2.shape != (B, n2, 2) or d1.shape[:2] != (B, n1) or d2.shape[:2] != (B, n2) or n1 < 1 or n2 < 1:
        raise ValueError("pts must be ([B,n1,2], [B,n2,2]) and desc ([B,n1,D], [B,n2,D]) with n1, n2 >= 1")
    dev = p1.device
    if counts is not None:
        if nn_thresh > 2.0 ** 0.5:
            raise ValueError("with counts, nn_thresh must not exceed sqrt(2): the rows past a count are zero descriptors")
        c1, c2 = (c.to(torch.int32).view(B, 1, 1) for c in counts)
        d1 = torch.where(torch.arange(n1, device=dev).view(1, n1, 1) < c1, d1, torch.zeros((), device=dev, dtype=d1.dtype))
        d2 = torch.where(torch.arange(n2, device=dev).view(1, n2, 1) < c2, d2, torch.zeros((), device=dev, dtype=d2.dtype))
    if noise is not None:
        p2 = p2 + noise.to(p2.dtype)
    m1, m2, sc, cnt = ops.nn_match_two_way(d1, d2, float(nn_thresh))
    # the match lists are written up to their count only: the rest is pointed at keypoint 0 so that every position can be gathered
    listed = torch.arange(n1, device=dev, dtype=torch.int32).view(1, n1) < cnt.view(B, 1)
    zero = torch.zeros((), device=dev, dtype=torch.int32)
    m1, m2 = torch.where(listed, m1, zero), torch.where(listed, m2, zero)
    sc = torch.where(listed, sc, torch.zeros((), device=dev, dtype=sc.dtype))
    choice = torch.arange(n1, device=dev, dtype=torch.int32).view(1, n1).expand(B, n1).contiguous()
    xs, _, q = ops.gather_matches(p1, p2, None, None, m1, m2, sc, choice)
    xs = torch.where(listed.unsqueeze(-1), xs, torch.zeros((), device=dev, dtype=xs.dtype))
    mscores = q.view(B, n1)
    r = ops.inlier_table(matches=xs, F=F_gt, scores=mscores, n_valid=cnt, inlier_thds=inlier_thds, mask_thds=mask_thds,
                         want=("cnt", "num", "ratio", "dist_out"))
    mean, num_T = ops.inlier_table_mean(r["ratio"], r["num"])
    return {"matches": xs, "mscores": mscores, "num_matches": cnt, "epi_dist_mean_gt": r["dist_out"], "cnt": r["cnt"], "num": r["num"],
            "ratio": r["ratio"], "inlier_ratio": mean, "num_corrs": num_T}
