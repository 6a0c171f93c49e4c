#!/usr/bin/env python3
"""Golden vectors for the sample-loss branch, from the reference itself: Fit.forward of deepFEPE/models/DeepFNetSampleLoss.py
(:364-436) and the if_sample_loss lines of get_all_loss_DeepF (deepFEPE/train_good_utils.py:387-426), run on the CPU in the
reference's own float32 and again in float64.  The reference is imported at generation time only, with the stub modules of
make_golden.py (cv2, pebble, superpoint; Tensor.cuda as identity) and one more, which is this repository's own code: `batch_svd`
(the un-vendored CUDA extension of :27) as a per-matrix torch.linalg.svd that returns (U, S, V) as torch.svd does.  Only data is
written.

    python tests/golden/make_golden_sample_loss.py <path to the reference checkout>     # rewrites tests/golden/sample_loss.npz

tests/golden/sample_loss.npz (38 arrays, 46996 bytes; described here, not in MANIFEST.txt, as make_golden_dsac.py describes its file).
Shape: B = 2, N = 64, H = 100, K = 20, depth 1, M = 100 virtual points, matches_good_unique_nums = [64, 50].  The sets are drawn by the
reference's own np.random.choice calls under np.random.seed(SEED) in the float32 run and recorded; the float64 run is handed the
recorded sets (its p differs from the float32 one in the last bits, which could move a draw across a boundary).

    matches [B,N,4], virt1, virt2 [B,M,3], logits [B,N] float32, nums [B], seed      the inputs
    idx [B,H,K] int32                                                                the sets np.random.choice drew
    f32_<key>, f64_<key>     out, residual, out_topK, residual_topK, out_sample_selected_batch, weights_sample_selected_accu_batch,
                             loss_selected_F, loss_selected_layers, g_weights, g_logits (d loss_selected_F / d weights and / d logits)
    yard_<key>               max |float32 - float64| of that quantity (F matrices after unit norm and sign alignment): the yardstick"""
import contextlib
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
SEED = 20201
B, N, M = 2, 64, 100
NUMS = [64, 50]
IMAGE_SIZE = [376, 1241, 3]
KEYS = ("out", "residual", "out_topK", "residual_topK", "out_sample_selected_batch", "weights_sample_selected_accu_batch")


def batch_svd(x):
    """The interface of torch-batch-svd: x [B,m,n] -> U [B,m,k], S [B,k], V [B,n,k], one LAPACK call per matrix."""
    import torch

    outs = [torch.linalg.svd(m, full_matrices=False) for m in x]
    return torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs]), torch.stack([o[2].transpose(0, 1) for o in outs])


def load_reference(root):
    import make_golden as mg

    mg.REF = root
    mg.install_stubs()
    mod = types.ModuleType("batch_svd")
    mod.batch_svd = batch_svd
    sys.modules["batch_svd"] = mod
    with contextlib.redirect_stdout(io.StringIO()):
        import models.DeepFNetSampleLoss as M
        import train_good_utils as tgu
    return M, tgu


def unit_aligned(a, ref):
    a, ref = a.reshape(-1, 9).astype(np.float64), ref.reshape(-1, 9).astype(np.float64)
    a, ref = a / np.linalg.norm(a, axis=1, keepdims=True), ref / np.linalg.norm(ref, axis=1, keepdims=True)
    return a * np.sign((a * ref).sum(1, keepdims=True)), ref


def run(M, tgu, dt, scene, logits32, recorded):
    """One run of the reference in dtype dt.  recorded None: np.random.choice draws (and the sets are returned); else they are replayed."""
    import torch

    import oracle.deepf_oracle as oracle

    sets = []
    real_choice = np.random.choice

    def choice(n, k, p=None):
        s = real_choice(n, k, p=p) if recorded is None else recorded[len(sets)]
        sets.append(np.asarray(s))
        return s

    logits = torch.from_numpy(logits32).to(dt).requires_grad_(True)
    weights = torch.softmax(logits.unsqueeze(1), dim=2)  # [B,1,N] (DeepFNetSampleLoss.py:583)
    weights.retain_grad()
    pts1, pts2, _ = oracle.normalize_hw(scene["matches_xy_ori"].to(dt), IMAGE_SIZE)
    T = oracle.hw_matrix(IMAGE_SIZE, dt).unsqueeze(0).expand(B, 3, 3)
    fit = M.Fit(is_cuda=False, if_sample_loss=True)
    for a in ("ones_b", "zero_b", "T_b", "mask"):
        setattr(fit, a, getattr(fit, a).to(dt))
    np.random.choice = choice
    try:
        np.random.seed(SEED)
        with contextlib.redirect_stdout(io.StringIO()):
            d = fit(pts1, pts2, weights, matches_good_unique_nums=torch.tensor(NUMS))
    finally:
        np.random.choice = real_choice
    outs = {"weights": weights, "F_est": d["out"], "T1": T, "T2": T, "out_layers": [d["out"]], "residual_layers": [d["residual"]],
            "weights_layers": [weights], "epi_res_layers": [], "out_sample_selected_batch_layers": [d["out_sample_selected_batch"]],
            "weights_sample_selected_accu_batch_layers": [d["weights_sample_selected_accu_batch"]]}
    lp = {"depth": 1, "clamp_at": 0.02, "if_tri_depth": False, "if_sample_loss": True, "topK": 8, "matches_good_unique_nums": NUMS}
    with contextlib.redirect_stdout(io.StringIO()):
        losses = tgu.get_all_loss_DeepF(outs, scene["pts1_virt_ori"].to(dt), scene["pts2_virt_ori"].to(dt), scene["Ks"].to(dt), lp,
                                        get_residual_summaries=False)[0]
    losses["loss_selected_F"].backward()
    res = {k: d[k].detach().numpy() for k in KEYS}
    res.update(loss_selected_F=losses["loss_selected_F"].detach().numpy(), loss_selected_layers=np.stack([x.detach().numpy() for x in losses["loss_selected_layers"]]),
               g_weights=weights.grad.numpy().reshape(B, N), g_logits=logits.grad.numpy())
    return res, np.stack(sets).reshape(B, -1, 20).astype(np.int32)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    import torch

    import make_golden as mg

    M, tgu = load_reference(sys.argv[1])
    scene = mg.synth.make_scene(B, N, seed=31, outlier_ratio=0.2, M_virt=M_VIRT, dtype=torch.float32)  # both runs start from the float32 inputs
    scene = {k: v.double() for k, v in scene.items()}
    logits32 = (0.5 * torch.randn(B, N, generator=torch.Generator().manual_seed(32))).numpy().astype(np.float32)
    f32, idx = run(M, tgu, torch.float32, scene, logits32, None)
    f64, idx2 = run(M, tgu, torch.float64, scene, logits32, list(idx.reshape(-1, 20)))
    assert (idx == idx2).all() and idx.shape == (B, 100, 20) and idx[1].max() < NUMS[1]
    out = {"matches": scene["matches_xy_ori"].numpy().astype(np.float32), "virt1": scene["pts1_virt_ori"].numpy().astype(np.float32),
           "virt2": scene["pts2_virt_ori"].numpy().astype(np.float32), "Ks": scene["Ks"].numpy().astype(np.float32), "logits": logits32,
           "nums": np.array(NUMS, np.int32), "seed": np.int64(SEED), "idx": idx}
    for k in f32:
        assert f32[k].dtype == np.float32 and f64[k].dtype == np.float64, k
        out["f32_" + k], out["f64_" + k] = f32[k], f64[k]
        if k.startswith("out"):
            a, r = unit_aligned(f32[k], f64[k])
            out["yard_" + k] = np.float64(np.abs(a - r).max())
        elif k.startswith("residual"):
            s = np.sign((f32[k].astype(np.float64) * f64[k]).sum(1, keepdims=True))
            out["yard_" + k] = np.float64(np.abs(f32[k] * s - f64[k]).max())
        else:
            out["yard_" + k] = np.float64(np.abs(f32[k].astype(np.float64) - f64[k]).max())
        print(f"{k}: yardstick {out['yard_' + k]:.3e}")
    path = os.path.join(HERE, "sample_loss.npz")
    np.savez_compressed(path, **out)
    print(f"sample_loss.npz: {len(out)} arrays, {os.path.getsize(path)} bytes")


M_VIRT = M

if __name__ == "__main__":
    main()
