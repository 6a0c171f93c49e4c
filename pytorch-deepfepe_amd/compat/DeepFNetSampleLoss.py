"""Mirror of deepFEPE/models/DeepFNetSampleLoss.py: Fit (:122-436) with its top-K and sampled-set fits, and Norm8PointNet
(:438-683), the model the reference builds for ``if_sample_loss`` (utils/loader.py:125-126).  The draws, the gather, the fits of the
100 sets per pair, their adjoint and the loss are launches of libdfepe_hip.so (ops.sample_multisets / topk_select / sample_fits /
sample_floss); nothing loops over pairs or sets on the host unless the caller asks for the reference's own NumPy draw."""
import numpy as np
import torch
import torch.nn as nn

from .. import ops
from .DeepFNet import DeepFNet, NormalizeAndExpand_HW, _require_gpu  # noqa: F401
from .DeepFNet import Fit as _Fit


def _counts(matches_good_unique_nums, B, N):
    """matches_good_unique_nums as the reference indexes with it: None (every correspondence), a list, an array or a tensor."""
    if matches_good_unique_nums is None:
        return None
    if torch.is_tensor(matches_good_unique_nums):
        return matches_good_unique_nums.reshape(B)
    return torch.as_tensor(np.asarray(matches_good_unique_nums).reshape(B))


class Fit(_Fit):
    """forward(pts1 [B,N,3], pts2 [B,N,3], weights [B,1,N]) -> the reference's dict: out [B,3,3], residual [B,N], out_topK,
    residual_topK (the fit of the topK largest weights among the first matches_good_unique_nums), out_sample_selected_batch
    [B,selects_each_sample,3,3] and weights_sample_selected_accu_batch [B,selects_each_sample,1] (the fits of the drawn sets and
    prod(1000 w) of each set over the pair's sum).

    ``sampler``: a compat.DeviceSampler draws the sets on the stream (ops.sample_multisets: the law of np.random.choice(n, topK,
    p=p), Philox streams, no host synchronisation).  None: the sets are drawn with np.random.choice on the host exactly as the
    reference draws them (:401-409), so a seeded NumPy stream reproduces the reference's sets; that costs one device-to-host copy
    of the weights per call.  Gradients flow to the weights; the points are constants of the sampled fits."""

    topK = 20
    selects_each_sample = 100

    def __init__(self, is_cuda=True, is_test=False, if_cpu_svd=False, normalize_SVD=True, if_sample_loss=False, sampler=None):
        super().__init__(is_cuda, is_test, if_cpu_svd, normalize_SVD)
        self.if_sample_loss = if_sample_loss
        self.sampler = sampler

    def get_unique(self, xs, topk, matches_good_unique_nums, pts1, pts2):
        """xs [B,1,N] -> (xs_topk [B,1,topk], indices [B,topk] int64, pts1 [B,topk,3], pts2 [B,topk,3]) (:345-362)."""
        B, N = xs.shape[0], xs.shape[-1]
        nv = _counts(matches_good_unique_nums, B, N)
        idx = ops.topk_select(xs.reshape(B, N), topk, None if nv is None else nv.to(xs.device, torch.int32)).long()
        take = idx.unsqueeze(-1).expand(-1, -1, 3)
        return torch.gather(xs, 2, idx.unsqueeze(1)), idx, torch.gather(pts1, 1, take), torch.gather(pts2, 1, take)

    def draw_host(self, weights, matches_good_unique_nums):
        """The reference's own draw (:401-409), call for call: idx [B,selects_each_sample,topK] int32 on the host."""
        B, N = weights.shape[0], weights.shape[-1]
        nv = _counts(matches_good_unique_nums, B, N)
        nums = [N] * B if nv is None else [int(v) for v in nv.cpu().numpy()]
        sets = []
        for num, w in zip(nums, weights.detach().cpu().numpy()):
            p = w.flatten()[:num]
            p = p / np.sum(p)
            sets.append(np.stack([np.random.choice(num, self.topK, p=p) for _ in range(self.selects_each_sample)]))
        return torch.from_numpy(np.stack(sets).astype(np.int32))

    def draw(self, weights, matches_good_unique_nums):
        B, N = weights.shape[0], weights.shape[-1]
        if self.sampler is None:
            return self.draw_host(weights, matches_good_unique_nums).to(weights.device)
        if self.sampler.counter.device != weights.device:
            raise ValueError(f"compat.DeepFNetSampleLoss.Fit: the sampler lives on {self.sampler.counter.device}, the weights on {weights.device}")
        nv = _counts(matches_good_unique_nums, B, N)
        idx = ops.sample_multisets(weights.reshape(B, N), self.selects_each_sample, self.topK, seed=self.sampler.seed,
                                   counter=self.sampler.counter, n_valid=None if nv is None else nv.to(weights.device, torch.int32))
        ops.sampler_advance(self.sampler.counter)
        return idx

    def forward(self, pts1, pts2, weights, if_print=False, matches_good_unique_nums=None):
        _require_gpu(weights, "Fit")
        out, residual = self.weighted_svd(pts1, pts2, weights, if_print=if_print)
        out_dict = {"out": out, "residual": residual}
        out_dict.update(self.selected(pts1, pts2, weights, matches_good_unique_nums))
        return out_dict

    def selected(self, pts1, pts2, weights, matches_good_unique_nums=None):
        """out_topK, residual_topK (:375-394) and out_sample_selected_batch, weights_sample_selected_accu_batch (:399-433)."""
        p1, p2 = pts1.detach(), pts2.detach()
        weights_topK, _, pts1_topK, pts2_topK = self.get_unique(weights, self.topK, matches_good_unique_nums, p1, p2)
        out_topK, residual_topK = ops.w8pt(pts1_topK, pts2_topK, weights_topK, normalize_rows=self.normalize_SVD)
        idx = self.draw(weights, matches_good_unique_nums)
        F_sel, accu = ops.sample_fits(p1, p2, weights, idx, normalize_rows=self.normalize_SVD)
        return {"out_topK": out_topK, "residual_topK": residual_topK, "out_sample_selected_batch": F_sel,
                "weights_sample_selected_accu_batch": accu}


class Norm8PointNet(DeepFNet):
    """The reference's constructor and dict keys (:439,660-677) on compat.DeepFNet's loop: every layer's fit is followed by the
    top-K fit and the sampled fits of that layer's weights (Fit.selected).  One deviation at depth > 1, none at depth 1: the
    reference's loop concatenates 6 channels (:622) into an estimator built for 7 (:487) and cannot run; the recurrent input here is
    DeepFNet.py's (weights, epi_res, residual), the one its state_dict fits.  ``sampler``: see Fit."""

    def __init__(self, depth, image_size, if_quality, if_goodCorresArch=False, if_tri_depth=False, if_sample_loss=False,
                 if_learn_offsets=False, if_des=False, des_size=None, quality_size=0, is_cuda=True, is_test=False, if_cpu_svd=False,
                 sampler=None, **params):
        super().__init__(depth, image_size, if_quality, if_img_w=False, if_goodCorresArch=if_goodCorresArch, if_tri_depth=if_tri_depth,
                         if_learn_offsets=if_learn_offsets, if_des=if_des, des_size=des_size, quality_size=quality_size, is_cuda=is_cuda,
                         is_test=is_test, if_cpu_svd=if_cpu_svd, **params)
        self.if_sample_loss = if_sample_loss
        self.if_tri_depth = if_tri_depth
        self.if_des = if_des
        self.if_goodCorresArch = if_goodCorresArch
        self.depth_size = 0
        self.fit = Fit(is_cuda, is_test, if_cpu_svd, if_sample_loss=if_sample_loss, sampler=sampler)

    def _inputs(self, data_batch, offsets=None, recurrent_copies=0):
        r = super()._inputs(data_batch, offsets, recurrent_copies)
        self._pts = (r[1], r[2])  # what the layer's fits see: the sampled fits gather from the same points
        return r

    def _fit(self, matches, logits, data_batch, want_epi, dst=None):
        outs = super()._fit(matches, logits, data_batch, want_epi, dst)
        sel = self.fit.selected(self._pts[0], self._pts[1], outs[-1], data_batch["matches_good_unique_nums"])
        for key, rows in self._selected.items():
            rows.append(sel[key[:-len("_layers")]])
        return outs

    def _forward(self, data_batch):
        self._selected = {"out_topK_layers": [], "out_sample_selected_batch_layers": [], "weights_sample_selected_accu_batch_layers": []}
        try:
            preds = super()._forward(data_batch)
            preds.update(self._selected)
        finally:
            self._selected, self._pts = None, None
        return preds
