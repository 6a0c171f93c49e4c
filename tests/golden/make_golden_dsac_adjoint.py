#!/usr/bin/env python3
"""Golden vectors for the adjoint of the DSAC loop, from the reference itself: class DSAC of deepFEPE/dsac_tools/dsac.py with HLoss of
dsac_tools/H_loss.py, differentiated by torch autograd on the CPU, once in float64 and once in float32.  The reference is imported at
generation time only, with make_golden_dsac.py's loader and its two repairs (utils_F.E_to_F aliased to utils_F._E_to_F; H_gt a zero
matrix, not None).  The loss function is wrapped so that the per-hypothesis losses are recorded; nothing of the class is changed.
Only data is written.

    python tests/golden/make_golden_dsac_adjoint.py <path to the reference checkout>     # rewrites tests/golden/dsac_adjoint.npz

Two scalars are differentiated w.r.t. X and Y:
    exp_loss = sum_h softmax(alpha score)_h loss_h      the expectation dsac.py:178-190 leaves commented out, built from the
                                                        inlier_scores the class keeps (score_h = their row sums) and the recorded losses
    sum_n c_n quality_n                                 quality = what __call__ returns, c a fixed standard-normal vector
The reference's refit weight is sqrt(1 - sigmoid(beta (d - thresh))): once beta (d - thresh) exceeds about 17 (float32) or 37
(float64) the difference cancels to an exact 0 and sqrt backpropagates inf * 0 = NaN.  So the finite cases below keep
beta (d - thresh) <= 12 for every hypothesis and correspondence (asserted here), and the last case, at the reference's own beta = 0.02
with 20 % gross outliers, stores only the FACT that the reference's gradient is not finite there.

tests/golden/dsac_adjoint.npz (described here, not in MANIFEST.txt).  n_cases, and per case k:
    k_X, k_Y [N,2], k_K [3,3] float32       dsac_cases.scene(1, N, seed, outliers)
    k_seed, k_hyps, k_thresh, k_beta, k_alpha, k_outliers
    k_idx [hyps,10] int32                   the sampled correspondences: random.seed(k_seed) right before the call
    k_c [N] float32                         the weights of the quality objective
    k_finite                                whether the reference's float64 AND float32 gradients are finite
    k_max_arg                               max beta (d - thresh) of the float64 run
  and for finite cases, for <what> in (exp_loss, quality) and <g> in (gX, gY):
    k_<what>_<g> [N,2] float64              the reference's float64 gradient
    k_<what>_yard_<g>                       max |float32 gradient - float64 gradient|: the yardstick
"""
import contextlib
import io
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

THRESH, ALPHA = 100.0, 0.1
# (N, hyps, seed, outliers, beta)
CASES = ((10, 4, 31, 0.0, 0.02), (33, 8, 32, 0.0, 0.02), (64, 16, 33, 0.0, 0.002), (65, 16, 34, 0.0, 0.002), (33, 8, 32, 0.2, 2e-4),
         (33, 8, 32, 0.2, 0.02))
MAX_ARG = 12.0


class Recording:
    def __init__(self, inner):
        self.inner, self.losses = inner, []

    def __call__(self, H, X, Y):
        loss = self.inner(H, X, Y)
        self.losses.append(loss)
        return loss


def gradients(dsac, H_loss, case, c, dtype):
    """The reference's autograd in `dtype` -> {(what, g): array}, max beta (d - thresh)."""
    import torch

    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)   # the class and utils_F build their constants (torch.zeros, torch.tensor([[S1, ...]])) in the default dtype
    try:
        X = torch.tensor(case["X"], dtype=dtype, requires_grad=True)
        Y = torch.tensor(case["Y"], dtype=dtype, requires_grad=True)
        rec = Recording(H_loss.HLoss())
        d = dsac.DSAC(case["hyps"], case["thresh"], case["beta"], case["alpha"], torch.tensor(case["K"], dtype=dtype), rec)
        random.seed(case["seed"])
        with contextlib.redirect_stdout(io.StringIO()):
            quality = d(X, Y, torch.zeros(3, 3))
        scores = d.inlier_scores.sum(1)
        losses = torch.stack([v.reshape(()) for v in rec.losses])
        exp_loss = (torch.softmax(case["alpha"] * scores, 0) * losses).sum()
        out = {}
        for what, obj in (("exp_loss", exp_loss), ("quality", (torch.tensor(c, dtype=dtype) * quality[:, 0]).sum())):
            gX, gY = torch.autograd.grad(obj, (X, Y), retain_graph=True)
            out[what, "gX"], out[what, "gY"] = gX.numpy().astype(np.float64), gY.numpy().astype(np.float64)
        arg = float((case["beta"] * (d.sampson_dists.detach() - case["thresh"])).max())
    finally:
        torch.set_default_dtype(old)
    return out, arg


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    import torch

    import dsac_cases as dc
    import make_golden_dsac as mk

    dsac, H_loss = mk.load_reference(sys.argv[1])
    out = {"n_cases": np.int64(len(CASES))}
    for k, (N, hyps, seed, outliers, beta) in enumerate(CASES):
        X, Y, K = dc.scene(1, N, seed, outliers)
        case = {"X": X[0], "Y": Y[0], "K": K[0], "hyps": hyps, "seed": seed, "thresh": THRESH, "beta": beta, "alpha": ALPHA}
        random.seed(seed)
        idx = np.array([random.sample(range(N), 10) for _ in range(hyps)], np.int32)
        c = np.random.default_rng([seed, 99]).standard_normal(N).astype(np.float32)
        g64, arg = gradients(dsac, H_loss, case, c, torch.float64)
        g32, _ = gradients(dsac, H_loss, case, c, torch.float32)
        finite = all(np.isfinite(v).all() for v in g64.values()) and all(np.isfinite(v).all() for v in g32.values())
        last = k == len(CASES) - 1
        assert finite != last, (k, "the last case, and only it, is where the reference's gradient is not finite")
        for key in ("X", "Y", "K"):
            out[f"{k}_{key}"] = case[key]
        out[f"{k}_seed"], out[f"{k}_hyps"], out[f"{k}_idx"], out[f"{k}_c"] = np.int64(seed), np.int64(hyps), idx, c
        out[f"{k}_thresh"], out[f"{k}_beta"], out[f"{k}_alpha"] = np.float64(THRESH), np.float64(beta), np.float64(ALPHA)
        out[f"{k}_outliers"], out[f"{k}_finite"], out[f"{k}_max_arg"] = np.float64(outliers), np.bool_(finite), np.float64(arg)
        if not finite:
            print(f"case {k}: N {N} hyps {hyps} beta {beta} outliers {outliers}: max beta (d - thresh) {arg:.3g}, the reference's gradient is "
                  f"NOT finite (float64 finite: {all(np.isfinite(v).all() for v in g64.values())})")
            continue
        assert arg <= MAX_ARG, (k, arg)
        line = []
        for (what, g), v in g64.items():
            out[f"{k}_{what}_{g}"] = v
            out[f"{k}_{what}_yard_{g}"] = np.float64(np.abs(g32[what, g] - v).max())
            line.append(f"{what} {g} {float(out[f'{k}_{what}_yard_{g}']) / np.abs(v).max():.3g}")
        print(f"case {k}: N {N} hyps {hyps} beta {beta} outliers {outliers}: max beta (d - thresh) {arg:.3g}; float32 vs float64, relative "
              f"to the largest entry: " + ", ".join(line))
    path = os.path.join(HERE, "dsac_adjoint.npz")
    np.savez_compressed(path, **out)
    print(f"dsac_adjoint.npz: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
