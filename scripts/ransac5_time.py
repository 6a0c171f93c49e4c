"""Time the batched five-point RANSAC baseline (ops.ransac_essential, ops.ransac_essential_pose) with device events after
warm-up, at the shapes and thresholds of scripts/ransac_time.py: (B, N) in {(8, 1000), (64, 1000), (256, 1000), (4096, 100)},
max_iters 1000, 0.1 px and 1.0 px on synthetic pairs (30 % outliers, 0.5 px noise).  Each line also carries the 8-point estimator
(ops.ransac_fundamental / ops.ransac_pose) at the same shape and threshold, and the ratio: recorded, not gated -- the device
evaluates all max_iters iterations whatever the stopping rule finds, and a five-point iteration is a 10x20 elimination, a
degree-10 root search and up to ten hypotheses to sweep against the 7-point solve's cubic and three.  Needs a GPU; prints one
JSON line per measurement.

    python scripts/ransac5_time.py [--reps 10] [--out FILE.jsonl]
"""
import argparse
import importlib
import json
import os
import sys

import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [REPO]
dfepe = importlib.import_module("pytorch-deepfepe_amd")

SHAPES = [(8, 1000), (64, 1000), (256, 1000), (4096, 100)]


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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ransac5_time.py needs a GPU")
    fout = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        fout = open(a.out, "w")
    ops = dfepe.ops
    for B, N in SHAPES:
        sc = dfepe.synth.make_scene(B, N, seed=B + N, outlier_ratio=0.3)
        m, K = sc["matches_xy_ori"].cuda(), sc["Ks"].cuda()
        for t in (0.1, 1.0):
            out = ops.ransac_essential(m, K, threshold=t)
            it = out["iters_run"].float()
            us_e = time_call(lambda: ops.ransac_essential(m, K, threshold=t), a.reps)
            us_p = time_call(lambda: ops.ransac_essential_pose(m, K, threshold=t), a.reps)
            us_f8 = time_call(lambda: ops.ransac_fundamental(m, threshold=t), a.reps)
            us_p8 = time_call(lambda: ops.ransac_pose(m, K, threshold=t), a.reps)
            line = json.dumps({"what": "device", "B": B, "N": N, "threshold": t, "max_iters": 1000, "essential_us": round(us_e, 1),
                               "essential_us_per_pair": round(us_e / B, 3), "pose_us": round(us_p, 1),
                               "pose_us_per_pair": round(us_p / B, 3), "iters_run_mean": round(float(it.mean()), 1),
                               "iters_run_max": int(it.max()), "inliers_mean": round(float(out["n_inliers"].float().mean()), 1),
                               "eight_point_fundamental_us": round(us_f8, 1), "eight_point_pose_us": round(us_p8, 1),
                               "ratio_to_eight_point": round(us_e / us_f8, 2)})
            print(line, flush=True)
            if fout is not None:
                fout.write(line + "\n")
    if fout is not None:
        fout.close()


if __name__ == "__main__":
    main()
