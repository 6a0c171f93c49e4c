"""Time one launch of the optimal correction (ops.correct_matches) and of the whole virtual-point generator
(compat.utils_misc.get_virt_x1x2_batch: the correction plus the homogeneous / inv(K) torch operations around it) with device
events after warm-up, at (B, M) = (8, 100) -- a training batch -- and (4096, 100), on the reference's 10 x 10 grid under the
ground-truth F of synthetic pairs.  For scale it also times the fp64 restatement of the tests (numpy.roots per point, one host
core), per sample of 100 points: recorded, not gated.  Needs a GPU; prints one JSON line per measurement.

    python scripts/correct_matches_time.py [--reps 20] [--out FILE.jsonl]
"""
import argparse
import importlib
import json
import os
import sys
import time

import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
dfepe = importlib.import_module("pytorch-deepfepe_amd")
import correct_matches_ref as ref  # noqa: E402

SHAPES = [(8, 100), (4096, 100)]
IM_SHAPE = (376, 1241)


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("correct_matches_time.py needs a GPU")
    lines = []
    um = dfepe.compat.utils_misc
    for B, M in SHAPES:
        sc = dfepe.synth.make_scene(B, M, seed=B + M, dtype=torch.float64)
        F, K = sc["F_gt"].cuda(), sc["Ks"].cuda()
        g = torch.as_tensor(um.get_virt_x1x2_grid(IM_SHAPE)[0]).cuda().expand(B, -1, -1).contiguous()
        us_k = time_call(lambda: dfepe.ops.correct_matches(F, g, g), a.reps)
        us_b = time_call(lambda: um.get_virt_x1x2_batch(IM_SHAPE, F, K), a.reps)
        lines.append({"what": "device", "B": B, "M": M, "correct_matches_us": round(us_k, 1),
                      "correct_matches_ns_per_point": round(us_k * 1e3 / (B * M), 2), "get_virt_x1x2_batch_us": round(us_b, 1)})
        print(json.dumps(lines[-1]), flush=True)
    sc = dfepe.synth.make_scene(8, 100, seed=108, dtype=torch.float64)
    g = ref.grid(IM_SHAPE)[0]
    t0 = time.perf_counter()
    for b in range(8):
        ref.correct_matches(sc["F_gt"][b].numpy(), g, g)
    lines.append({"what": "host restatement (numpy.roots, one core)", "M": 100, "ms_per_sample": round((time.perf_counter() - t0) * 1e3 / 8, 2)})
    print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(l) + "\n" for l in lines)


if __name__ == "__main__":
    main()
