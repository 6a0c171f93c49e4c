"""Time the SuperPoint output processing (ops.sp_flatten, sp_nms, sp_soft_argmax, sp_sample_desc and the two adjoints) with device
events after warm-up at the KITTI shape: 2 images of 376 x 1240 cropped to a multiple of 8 (368 x 1240), D = 256, the reference's
settings (nms_dist 4, conf_thresh 0.015, patch_size 5), next to stock torch where it has the same step (softmax + pixel_shuffle
for the heatmap, grid_sample + normalize for the descriptors): recorded, not gated.  The logits are seeded noise shaped so that
the heatmap has isolated peaks like a detector's.  Needs a GPU; prints one JSON line per measurement.

    python scripts/sp_process_time.py [--reps 50] [--out FILE.jsonl]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [REPO]
dfepe = importlib.import_module("pytorch-deepfepe_amd")

B, H, W, D = 2, 368, 1240, 256
NMS_DIST, CONF, PATCH, BORDER = 4, 0.015, 5, 4


def time_call(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / reps  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sp_process_time.py needs a GPU")
    dev = "cuda:0"
    ops = dfepe.ops
    Hc, Wc = H // 8, W // 8
    rng = np.random.default_rng(0)
    semi_np = rng.standard_normal((B, 65, Hc, Wc)).astype(np.float32)
    semi_np[:, 64] += 4.0                                         # most cells are background ...
    peak = rng.random((B, Hc, Wc)) < 0.35                         # ... about a third hold one clear corner
    ch = rng.integers(0, 64, (B, Hc, Wc))
    bb, yy, xx = np.nonzero(peak)
    semi_np[bb, ch[bb, yy, xx], yy, xx] += 7.0
    semi = torch.as_tensor(semi_np, device=dev).requires_grad_(True)
    desc = torch.as_tensor(rng.standard_normal((B, D, Hc, Wc)).astype(np.float32), device=dev)
    heat = ops.sp_flatten(semi)
    hd = heat.detach().requires_grad_(True)
    nms = ops.sp_nms(hd, CONF, NMS_DIST, BORDER)
    pts, count = nms["pts"], nms["count"]
    pred = ops.sp_soft_argmax(hd, pts, count, PATCH, BORDER)
    g_pred, g_heat = torch.randn_like(pred), torch.randn_like(heat)
    lines = []

    def rec(name, us, **extra):
        lines.append({"step": name, "us": round(us, 1), **extra})
        print(json.dumps(lines[-1]), flush=True)

    rec("shape", 0.0, B=B, H=H, W=W, D=D, cap=int(pts.shape[1]), kept=[int(c) for c in count.cpu()],
        candidates=[int(c) for c in (heat.detach() >= CONF).flatten(1).sum(1).cpu()])
    with torch.no_grad():
        rec("sp_flatten", time_call(lambda: ops.sp_flatten(semi), a.reps))
        rec("torch softmax + pixel_shuffle", time_call(lambda: torch.nn.functional.pixel_shuffle(torch.softmax(semi, 1)[:, :64], 8), a.reps))
        rec("sp_nms", time_call(lambda: ops.sp_nms(hd, CONF, NMS_DIST, BORDER), max(a.reps // 5, 3)))
        rec("sp_soft_argmax", time_call(lambda: ops.sp_soft_argmax(hd, pts, count, PATCH, BORDER), a.reps))
        rec("sp_sample_desc", time_call(lambda: ops.sp_sample_desc(desc, pts, pred, count), a.reps))
        n = int(count.min())
        pos = (pts[:, :n].float() + pred[:, :n]).detach()
        grid = torch.stack((pos[..., 0] / (W / 2) - 1, pos[..., 1] / (H / 2) - 1), -1)[:, None]
        rec("torch grid_sample + normalize", time_call(lambda: torch.nn.functional.normalize(
            torch.nn.functional.grid_sample(desc, grid, mode="bilinear", align_corners=True)[:, :, 0].transpose(1, 2), dim=2), a.reps), points=n)
    rec("sp_soft_argmax backward", time_call(lambda: torch.autograd.grad(ops.sp_soft_argmax(hd, pts, count, PATCH, BORDER), hd, g_pred), a.reps),
        note="forward + adjoint")
    rec("sp_flatten backward", time_call(lambda: torch.autograd.grad(ops.sp_flatten(semi), semi, g_heat), a.reps), note="forward + adjoint")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(l) + "\n" for l in lines)


if __name__ == "__main__":
    main()
