"""The SuperPoint output processing behind the reference's process_SP_output (deepFEPE/train_good_utils.py:727-755):
``flattenDetection`` (superpoint.utils.utils) and ``SuperPointNet_process`` (superpoint.models.model_utils) with the methods
that function calls.  The superpoint package is not part of the reference's tree; these are the published algorithm as
include/dfepe.h states it (unpinned), on the GPU: one launch per step for the whole batch, and the gradient of the offsets
reaches ``semi`` through soft-argmax and softmax adjoints that are bit-identical from run to run.

What differs from a per-image numpy implementation, by design:
  * ties in the NMS order are broken by row-major index (the reference's argsort is unstable);
  * ``pred_soft_argmax`` returns ``pred`` as the padded list [B,cap,2] (rows in ``nonzero()`` order per image, zeros after
    the image's count) instead of one flat [sum(count),2] tensor, which would need the counts on the host;
  * ``batch_extract_features`` copies the B counts to the host once (the random crop/pad is the host's, drawn from numpy's
    global RNG like utils_misc.crop_or_pad_choice).
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib, ops
from .utils_misc import crop_or_pad_choice


def flattenDetection(semi, tensor=False):
    """semi [65,Hc,Wc] or [B,65,Hc,Wc] -> heatmap [1,H,W] or [B,1,H,W] (softmax over the channels, dustbin dropped, depth to
    space).  ``tensor`` is accepted for the reference's signature; the result is a tensor either way.  Differentiable."""
    if semi.dim() == 3:
        return ops.sp_flatten(semi.unsqueeze(0)).squeeze(0)
    return ops.sp_flatten(semi)


class SuperPointNet_process:
    """``SuperPointNet_process(**config)`` with the keys the reference's configs set (utils/eval_tools.py:655-662):
    out_num_points, patch_size, nms_dist, conf_thresh; and border_remove (default 4, SuperPoint's), the border that the NMS
    removes and that keeps every patch inside the image (patch_size <= 2 border_remove + 1)."""

    def __init__(self, **config):
        self.out_num_points = int(config.get("out_num_points", 500))
        self.patch_size = int(config.get("patch_size", 5))
        self.nms_dist = int(config.get("nms_dist", 4))
        self.conf_thresh = float(config.get("conf_thresh", 0.015))
        self.border_remove = int(config.get("border_remove", 4))
        self.align_corners = bool(config.get("align_corners", True))
        if self.patch_size % 2 == 0 or self.patch_size < 1 or self.patch_size > 2 * self.border_remove + 1:
            raise ValueError("patch_size must be odd and at most 2 border_remove + 1 (every patch must lie inside the image)")
        if self.nms_dist < 0 or self.out_num_points < 1:
            raise ValueError("nms_dist must be >= 0 and out_num_points >= 1")
        self._last = None  # (nms_map, pts, conf, count) of the last heatmap_to_nms

    # -- NMS ---------------------------------------------------------------------------------------------------------
    def heatmap_to_nms(self, heatmap, tensor=False, boxnms=False):
        """heatmap [B,1,H,W] -> the dense 0/1 map [B,1,H,W] of the greedy NMS (a tensor on the device with ``tensor=True``, else
        a numpy array).  The point list behind the map is kept for the two methods below."""
        if boxnms:
            raise NotImplementedError("boxnms (torchvision's box NMS) is not built; the reference's process_SP_output does not use it")
        out = ops.sp_nms(heatmap, self.conf_thresh, self.nms_dist, self.border_remove)
        self._last = (out["nms_map"], out["pts"], out["conf"], out["count"])
        return out["nms_map"] if tensor else out["nms_map"].cpu().numpy()

    def _list_of(self, nms_map):
        """The (pts, count) list of a dense map: the one kept by heatmap_to_nms when it is that map, else (a map from elsewhere)
        its non-zero pixels in row-major order, from a pass with distance 0 over the map itself."""
        if self._last is not None and nms_map is self._last[0]:
            return self._last[1], self._last[3]
        if not torch.is_tensor(nms_map):
            nms_map = torch.as_tensor(np.asarray(nms_map), dtype=torch.float32).cuda()
        out = ops.sp_nms(nms_map, 0.5, 0, self.border_remove)
        return out["pts"], out["count"]

    # -- sub-pixel offsets -----------------------------------------------------------------------------------------------
    def pred_soft_argmax(self, labels_2D, heatmap):
        """labels_2D: the dense NMS map; heatmap [B,1,H,W] -> {"pred": [B,cap,2] offsets (x, y), differentiable w.r.t. the
        heatmap, "patches": [B,cap,p,p] normalised patches}."""
        pts, count = self._list_of(labels_2D)
        pred, patches = ops.sp_soft_argmax(heatmap, pts, count, self.patch_size, self.border_remove, want_patches=True)
        return {"pred": pred, "patches": patches}

    # -- points, offsets, descriptors ------------------------------------------------------------------------------------
    def batch_extract_features(self, desc, heatmap_nms_batch, residual):
        """desc [B,D,Hc,Wc], the dense NMS map, residual = pred of pred_soft_argmax -> {"pts_int": [B,N,2] (x, y) float,
        "pts_offset": [B,N,2] (carries the gradient), "pts_desc": [B,N,D] (detached)}, N = out_num_points rows per image chosen
        by crop_or_pad_choice(count, N, shuffle=True).  One copy of the B counts to the host."""
        pts, count = self._list_of(heatmap_nms_batch)
        B, cap = pts.shape[0], pts.shape[1]
        if residual.shape != (B, cap, 2):
            raise ValueError(f"residual must be the [B,cap,2] = [{B},{cap},2] pred of pred_soft_argmax, got {tuple(residual.shape)}")
        pts_desc_all = ops.sp_sample_desc(desc, pts, residual, count, self.align_corners)
        counts = count.cpu().numpy()
        if (counts < 1).any():
            raise ValueError("batch_extract_features: an image without a keypoint cannot be padded (np.random.choice of nothing)")
        choice = np.stack([crop_or_pad_choice(int(n), self.out_num_points, shuffle=True) for n in counts]).astype(np.int32)
        choice_dev = torch.from_numpy(choice).to(pts.device)
        # the gather of the match construction with the identity as match list: rows pts[choice], residual[choice], and a
        # deterministic adjoint into residual where rows repeat
        ident = torch.arange(cap, device=pts.device, dtype=torch.int32).expand(B, cap).contiguous()
        pts_f = pts.float()
        xs, offs, _ = ops.gather_matches(pts_f, pts_f, residual, residual.detach(), ident, ident, pts_f[:, :, 0].contiguous(), choice_dev)
        idx = choice_dev.long().unsqueeze(-1).expand(B, self.out_num_points, pts_desc_all.shape[2])
        return {"pts_int": xs[:, :, :2], "pts_offset": offs[:, :, :2], "pts_desc": torch.gather(pts_desc_all, 1, idx)}

    @staticmethod
    def sample_desc_from_points(coarse_desc, pts, cell_size=8):
        """coarse_desc [1,D,Hc,Wc] (or [D,Hc,Wc]), pts [N,2] (x, y) in pixels, float -> [N,D] unit-norm descriptors."""
        if cell_size != 8:
            raise NotImplementedError("cell_size is 8 in SuperPoint; no other is built")
        if not torch.is_tensor(pts) or not pts.is_cuda:
            raise _lib.DfepeError("sample_desc_from_points: pts must live on the GPU (this package has no CPU path)")
        d = coarse_desc if coarse_desc.dim() == 4 else coarse_desc.unsqueeze(0)
        if d.shape[0] != 1 or pts.dim() != 2 or pts.shape[1] != 2:
            raise ValueError("sample_desc_from_points takes one image's descriptors and [N,2] points")
        p = pts.detach().float()
        whole = torch.floor(p)
        n = torch.tensor([p.shape[0]], device=p.device, dtype=torch.int32)
        return ops.sp_sample_desc(d, whole.to(torch.int32).unsqueeze(0), (p - whole).unsqueeze(0), n, True)[0]
