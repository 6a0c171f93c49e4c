"""Mirror of deepFEPE/dsac_tools/dsac.py (class DSAC, :13-200): the RANSAC-style hypothesis loop over essential matrices.

The reference runs the loop on the CPU, one hypothesis at a time ("working on CPU because of many, small matrices",
dsac.py:110): sample 10 correspondences -> _E_from_XY -> soft inlier count from Sampson distances -> refinement by a
weighted _E_from_XY over all correspondences -> loss, and returns the per-correspondence average score of the hypotheses
each correspondence was sampled into (:194).  Here the whole loop is ops.dsac (dfepe_dsac, include/dfepe.h): every pair of a
batch and all its hypotheses go through six launches, without a host synchronisation in between.  By default sampling uses
Python's `random.sample` with the reference's call sequence (one call per hypothesis), so a seeded run draws the same minimal sets.
With a DeviceSampler the sets are drawn on the stream instead (ops.sample_sets, dfepe_sample_sets): no host loop, no copy, uniformly
(random.sample's law for the set) or in proportion to per-correspondence weights, as DeepFNetSampleLoss.Fit.forward draws with
np.random.choice(n, topK, p=p) over the first matches_good_unique_num correspondences; the sampler's counter lives on the device
and advances on the stream, so a captured training step draws fresh hypotheses on every replay.
The reference calls an undefined `utils_F.E_to_F` at :67 (only `_E_to_F` exists); its evident intent, F = K^-T E K^-1, is
what is computed.  Its prints are not mirrored.

The adjoint of the loop is dfepe_dsac_bwd: dsac_batch and DSAC.expected_loss are differentiable w.r.t. X and Y through ops.dsac.
DSAC.__call__ is the reference's call and returns a CPU tensor without a graph: inputs that require grad raise NotImplementedError
there; expected_loss is the differentiable entry.  Not built: the gradient to K, a device sampler that replays random.sample's
Mersenne Twister stream (a DeviceSampler draws other sets than the seeded host draw), and `loss_function`s other than
H_loss.HLoss on the fused path: any other callable is evaluated per hypothesis on the refitted E, one call and its launches per
hypothesis -- the slow route, forward only.
"""
import random

import torch

from .. import _lib, ops
from .H_loss import HLoss

SAMPLE = 10  # correspondences per hypothesis (dsac.py:46)


def _device_of(*ts):
    for t in ts:
        if torch.is_tensor(t) and t.is_cuda:
            return t.device
    return torch.device("cuda", torch.cuda.current_device())


def _draw(N, hyps, sample, rng=random):
    """One random.sample per hypothesis, in hypothesis order (dsac.py:46, :138): raises ValueError when N < sample, as it does."""
    return [rng.sample(range(N), sample) for _ in range(hyps)]


class DeviceSampler:
    """The minimal sets drawn on the device (ops.sample_sets): Philox4x32-10 under ``seed``, at the stream offset held in ``counter``,
    one uint32 on the device that every draw advances by one ON THE STREAM (ops.sampler_advance).  Successive draws therefore
    differ, need no host work and no copy, and a draw captured in a hipGraph samples the next offset on every replay."""

    def __init__(self, seed, device=None):
        self.seed = int(seed) & ((1 << 64) - 1)
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.counter = torch.tensor([0], dtype=torch.uint32).to(dev)

    def draw(self, B, N, hyps, sample=SAMPLE, weights=None, n_valid=None):
        """idx [B,hyps,sample] int32 on the device, for the current value of the counter; then the counter advances.  ``weights``
        [B,N]: draw in proportion to them; ``n_valid`` [B] int32: only the first n_valid[b] correspondences (both on the device)."""
        idx = ops.sample_sets(B, N, hyps, sample, seed=self.seed, counter=self.counter, weights=weights, n_valid=n_valid)
        ops.sampler_advance(self.counter)
        return idx


class DSAC:
    def __init__(self, hyps, inlier_thresh, inlier_beta, inlier_alpha, K, loss_function, *, sampler=None):
        self.sampler = sampler  # None: the reference's random.sample sequence; a DeviceSampler: drawn on the stream
        self.hyps = hyps
        self.inlier_thresh = inlier_thresh
        self.inlier_beta = inlier_beta
        self.inlier_alpha = inlier_alpha
        self.loss_function = loss_function
        self.K = K

    def _sets(self, N, X, Y):
        """-> (the device, idx [hyps,SAMPLE] int32 on it, the same as a list of lists or None when it was drawn on the device).  The
        host draw comes first, as in the reference: its ValueError (N < 10) needs no device."""
        if self.sampler is None:
            idx_list = _draw(N, self.hyps, SAMPLE)
            dev = _device_of(X, Y)
            return dev, torch.tensor(idx_list, dtype=torch.int32).to(dev), idx_list
        dev = _device_of(X, Y)
        if self.sampler.counter.device != dev:
            raise ValueError(f"compat.dsac.DSAC: the sampler lives on {self.sampler.counter.device}, the points on {dev}")
        return dev, self.sampler.draw(1, N, self.hyps, SAMPLE)[0], None

    def __call__(self, X, Y, H_gt=None):
        """X, Y [N,2] pixel correspondences (CPU or GPU) -> [N,1] float32 CPU tensor: the average soft-inlier score of the
        hypotheses each correspondence was drawn into (dsac.py:194).  Sets inlier_scores [hyps,N], sampson_dists [hyps,N],
        max_score, best_H, best_H_idx, best_dists, best_corres_idx like the reference (the tensors stay on the device), and
        hyp_scores, hyp_losses [hyps], exp_loss, top_loss (the step the reference leaves commented out, :178-190)."""
        X, Y = torch.as_tensor(X), torch.as_tensor(Y)
        N, H = X.shape[0], self.hyps
        assert Y.shape[0] == N, "N mismatch between X and Y!"
        if any(torch.is_tensor(t) and t.requires_grad for t in (X, Y, self.K)):
            raise NotImplementedError("compat.dsac.DSAC: the adjoint of the hypothesis loop is not built; detach the inputs")
        self.N = N
        dev, idx, idx_list = self._sets(N, X, Y)
        X, Y = X.to(dev, torch.float32), Y.to(dev, torch.float32)
        K = torch.as_tensor(self.K, dtype=torch.float32).to(dev)
        fused = isinstance(self.loss_function, HLoss)
        r = ops.dsac(X[None], Y[None], K.reshape(1, 3, 3), idx[None], self.inlier_thresh, self.inlier_beta, self.inlier_alpha,
                     loss_kind=1 if fused else 0)
        self.inlier_scores, self.sampson_dists = r["soft"][0], r["sampson"][0]
        self.hyp_scores, E_refit = r["score"][0], r["E_refit"][0]
        self.hyp_losses = None
        self.exp_loss = self.top_loss = None
        if fused:
            self.hyp_losses, self.exp_loss, self.top_loss = r["loss"][0], r["exp_loss"][0], r["top_loss"][0]
        elif self.loss_function is not None:  # the slow route: one call of the user's function per hypothesis (dsac.py:157)
            self.hyp_losses = torch.stack([torch.as_tensor(self.loss_function(E_refit[h], X, Y), dtype=torch.float32, device=dev).reshape(())
                                           for h in range(H)])
        best = int(r["best"][0].item())  # the one host synchronisation of the call
        self.max_score = 0
        if best >= 0:  # the reference leaves these unset when no score is above 0 (:168)
            self.max_score = float(self.hyp_scores[best].item())
            self.best_H, self.best_H_idx, self.best_dists = E_refit[best], best, self.inlier_scores[best]
            self.best_corres_idx = idx_list[best] if idx_list is not None else idx[best].tolist()  # after the synchronisation above
        return r["quality"][0].unsqueeze(1).cpu()

    def expected_loss(self, X, Y):
        """The training step the reference leaves commented out (dsac.py:178-190), differentiable: X, Y [N,2] pixel
        correspondences -> (exp_loss, top_loss), device scalars; exp_loss = sum_h softmax(alpha score)_h loss_h carries the graph to
        X and Y (ops.dsac, dfepe_dsac_bwd), top_loss = loss[best] does not.  Draws the seeded minimal sets __call__ draws and sets
        the attributes __call__ sets (none of those carries a graph), plus ``quality`` [N,1] on the device with its graph.  Needs the
        fused loss, H_loss.HLoss: any other callable raises NotImplementedError.  K is a constant of the adjoint."""
        if not isinstance(self.loss_function, HLoss):
            raise NotImplementedError("compat.dsac.DSAC.expected_loss: only H_loss.HLoss is fused into the loop and its adjoint; "
                                      "the adjoint of an arbitrary loss_function is not built")
        X, Y = torch.as_tensor(X), torch.as_tensor(Y)
        N, H = X.shape[0], self.hyps
        assert Y.shape[0] == N, "N mismatch between X and Y!"
        self.N = N
        dev, idx, idx_list = self._sets(N, X, Y)
        X, Y = X.to(dev, torch.float32), Y.to(dev, torch.float32)
        K = torch.as_tensor(self.K, dtype=torch.float32).to(dev)
        r = ops.dsac(X[None], Y[None], K.reshape(1, 3, 3), idx[None], self.inlier_thresh, self.inlier_beta, self.inlier_alpha, loss_kind=1)
        self.inlier_scores, self.sampson_dists = r["soft"][0], r["sampson"][0]
        self.hyp_scores, E_refit = r["score"][0].detach(), r["E_refit"][0].detach()
        self.hyp_losses, self.exp_loss, self.top_loss = r["loss"][0].detach(), r["exp_loss"][0], r["top_loss"][0]
        self.quality = r["quality"][0].unsqueeze(1)
        best = int(r["best"][0].item())  # the one host synchronisation of the call
        self.max_score = 0
        if best >= 0:
            self.max_score = float(self.hyp_scores[best].item())
            self.best_H, self.best_H_idx, self.best_dists = E_refit[best], best, self.inlier_scores[best]
            self.best_corres_idx = idx_list[best] if idx_list is not None else idx[best].tolist()  # after the synchronisation above
        return self.exp_loss, self.top_loss


def dsac_batch(X, Y, K, hyps, inlier_thresh, inlier_beta, inlier_alpha=0.0, idx=None, seed=None, sample=SAMPLE, loss_kind=0,
               want=("soft", "sampson", "exp_loss", "top_loss"), sampler=None, weights=None, n_valid=None):
    """The loop for a batch on the device: X, Y [B,N,2], K [B,3,3] (or [3,3], shared) -> ops.dsac's dict (E_sample, score, E_refit,
    loss, quality [B,N], counts, best, and what ``want`` names), plus "idx".  ``idx`` [B,hyps,sample] int32 on the device is used
    as given; otherwise it is drawn on the host -- random.Random(seed), pair by pair, hypothesis by hypothesis, random.sample as
    the reference draws -- and copied once.  No host synchronisation after that.  With ``sampler``, a DeviceSampler, the sets are
    drawn on the stream instead (no host work, no copy; capturable, and every replay draws the next offset): uniformly, or with
    ``weights`` [B,N] in proportion to them, among the first ``n_valid`` [B] (int32) correspondences of each pair when given.  Both
    need a DeviceSampler: without one they raise ValueError (the host draw is uniform over all N)."""
    if not (torch.is_tensor(X) and X.is_cuda):
        raise _lib.DfepeError("compat.dsac.dsac_batch: X, Y must live on the GPU (this package has no CPU path)")
    B, N = X.shape[0], X.shape[1]
    K = torch.as_tensor(K, dtype=torch.float32).to(X.device)
    if K.dim() == 2:
        K = K.expand(B, 3, 3)
    if (weights is not None or n_valid is not None) and (sampler is None or idx is not None):
        raise ValueError("compat.dsac.dsac_batch: weights and n_valid steer a DeviceSampler's draw; pass sampler=DeviceSampler(seed) and no idx")
    if idx is None and sampler is not None:
        idx = sampler.draw(B, N, hyps, sample, weights=weights, n_valid=n_valid)
    elif idx is None:
        rng = random.Random(seed)
        idx = torch.tensor([_draw(N, hyps, sample, rng) for _ in range(B)], dtype=torch.int32).reshape(B, hyps, sample).to(X.device)
    out = ops.dsac(X, Y, K.contiguous(), idx, inlier_thresh, inlier_beta, inlier_alpha, loss_kind=loss_kind, want=want)
    out["idx"] = idx
    return out
