"""The sample-loss objective end to end on the GPU: compat.DeepFNetSampleLoss.Norm8PointNet + compat.train_good_utils.get_all_loss_DeepF
(if_sample_loss) at depth 1, loss_selected_F and its gradient w.r.t. the logits against float64 -- the reference's own float64 run
recorded in tests/golden/sample_loss.npz at 2 x 64 x 100 x 20, and the float64 restatement (tests/sample_loss_ref.py) at
3 x 100 x 100 x 20.  The yardstick is the distance of the reference's own float32 run from its float64 run (recorded in the golden;
the restatement's float32 run at the second shape), the margin 4 x: the factor tests/test_refcfg_gpu.py uses for different but
equally valid float32 orderings.  The sets are the host draw under a seeded NumPy stream, so both sides fit the same sets."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_loss_cases as sc  # noqa: E402
import sample_loss_ref as slr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 4.0


class _FixedLogits(nn.Module):
    """Stands in for the estimator: the logits are the leaf the gradient is taken at."""

    def __init__(self, logits):
        super().__init__()
        self.logits = nn.Parameter(logits.clone())

    def forward(self, x):
        return self.logits


def _run(dfepe, matches, logits, virt1, virt2, Ks, nums, seed):
    C = dfepe.compat
    B, N = logits.shape
    net = C.DeepFNetSampleLoss.Norm8PointNet(1, sc.IMAGE_SIZE, False, if_sample_loss=True).to(DEV)
    net.input_weights = _FixedLogits(logits.reshape(B, 1, N).to(DEV))
    drawn = []
    draw = net.fit.draw
    net.fit.draw = lambda w, n: drawn.append(draw(w, n)) or drawn[-1]
    np.random.seed(seed)
    outs = net({"matches_xy_ori": matches.to(DEV), "matches_good_unique_nums": nums, "t_scene_scale": None})
    lp = {"depth": 1, "clamp_at": 0.02, "if_tri_depth": False, "if_sample_loss": True, "topK": 8, "matches_good_unique_nums": nums}
    losses = C.train_good_utils.get_all_loss_DeepF(outs, virt1.to(DEV), virt2.to(DEV), Ks.to(DEV), lp, get_residual_summaries=False)[0]
    losses["loss_selected_F"].backward()
    assert len(losses["loss_selected_layers"]) == 1 and len(drawn) == 1
    return outs, losses, net.input_weights.logits.grad.reshape(B, N).cpu().numpy(), drawn[0].cpu().numpy()


def _report(name, got, want, yard):
    err = float(np.abs(np.asarray(got, np.float64) - want).max())
    print(f"SAMPLE e2e {name}: |ours - f64| = {err:.3e}, reference's float32 = {yard:.3e}, ratio {err / yard:.2f} (bound {FACTOR})")
    return err / yard


def test_golden_shape(dfepe, golden):
    g = golden("sample_loss")
    T = torch.from_numpy
    outs, losses, g_logits, idx = _run(dfepe, T(g["matches"]), T(g["logits"]), T(g["virt1"]), T(g["virt2"]), T(g["Ks"]), T(g["nums"]), int(g["seed"]))
    assert (idx == g["idx"]).all()  # the seeded NumPy stream reproduces the reference's sets
    for key in ("out_topK_layers", "out_sample_selected_batch_layers", "weights_sample_selected_accu_batch_layers"):
        assert len(outs[key]) == 1
    assert tuple(outs["out_sample_selected_batch_layers"][0].shape) == (2, 100, 3, 3)
    assert tuple(outs["weights_sample_selected_accu_batch_layers"][0].shape) == (2, 100, 1)
    ratios = {}
    for key, name in (("out_layers", "out"), ("out_topK_layers", "out_topK"), ("out_sample_selected_batch_layers", "out_sample_selected_batch")):
        a, r = outs[key][0].detach().cpu().numpy().reshape(-1, 9).astype(np.float64), g["f64_" + name].reshape(-1, 9)
        a, r = a / np.linalg.norm(a, axis=1, keepdims=True), r / np.linalg.norm(r, axis=1, keepdims=True)
        ratios[name] = _report(name, a * np.sign((a * r).sum(1, keepdims=True)), r, float(g["yard_" + name]))
    ratios["accu"] = _report("accu", outs["weights_sample_selected_accu_batch_layers"][0].detach().cpu().numpy(),
                             g["f64_weights_sample_selected_accu_batch"], float(g["yard_weights_sample_selected_accu_batch"]))
    ratios["loss"] = _report("loss_selected_F", losses["loss_selected_F"].item(), float(g["f64_loss_selected_F"]), float(g["yard_loss_selected_F"]))
    ratios["g_logits"] = _report("d loss / d logits", g_logits, g["f64_g_logits"], float(g["yard_g_logits"]))
    assert all(v < FACTOR for v in ratios.values()), ratios


def test_three_pairs_of_a_hundred(dfepe):
    B, N = 3, 100
    s = dfepe.synth.make_scene(B, N, seed=61, outlier_ratio=0.2)
    logits = 0.5 * torch.randn(B, N, generator=torch.Generator().manual_seed(62))
    outs, losses, g_logits, idx = _run(dfepe, s["matches_xy_ori"], logits, s["pts1_virt_ori"], s["pts2_virt_ori"], s["Ks"], None, 63)
    oracle = __import__("oracle.deepf_oracle", fromlist=["x"])
    T = torch.from_numpy(sc.T_HW)
    ref = {}
    for dt in (torch.float32, torch.float64):  # the restatement in float64 and, for the yardstick, in the reference's float32
        lo = logits.detach().clone().to(dt).requires_grad_(True)
        p1, p2, _ = oracle.normalize_hw(s["matches_xy_ori"].to(dt), sc.IMAGE_SIZE)
        F_sel, _ = slr.fit_selected(p1, p2, torch.softmax(lo, 1), idx, dtype=dt)
        loss, _ = slr.loss_selected([F_sel], T.to(dt), T.to(dt), s["pts1_virt_ori"].to(dt), s["pts2_virt_ori"].to(dt))
        loss.backward()
        ref[dt] = (loss.item(), lo.grad.numpy().astype(np.float64))
    (l32, g32), (l64, g64) = ref[torch.float32], ref[torch.float64]
    ratios = {"loss": _report("loss_selected_F (3 x 100)", losses["loss_selected_F"].item(), l64, abs(l32 - l64)),
              "g_logits": _report("d loss / d logits (3 x 100)", g_logits, g64, float(np.abs(g32 - g64).max()))}
    assert all(v < FACTOR for v in ratios.values()), ratios
