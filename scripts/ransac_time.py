"""Time the batched RANSAC baseline (ops.ransac_fundamental, ops.ransac_pose) with device events after warm-up, at the shapes of
DESIGN.md §3 (B, N) in {(8, 1000), (64, 1000), (256, 1000), (4096, 100)}, max_iters 1000, thresholds 0.1 px and 1.0 px on
synthetic pairs (30 % outliers, 0.5 px noise: at 0.1 px few true points are inliers and every pair runs all 1000 iterations).
For scale, the fp64 numpy restatement of the same sequential algorithm (tests/ransac_ref.py) on ONE host core -- OpenCV is not
a dependency of the project, so it is not timed.  Needs a GPU; prints one JSON line per measurement.

    python scripts/ransac_time.py [--reps 20] [--host-pairs 2] [--out FILE.jsonl]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
dfepe = importlib.import_module("pytorch-deepfepe_amd")
import ransac_ref as ref  # noqa: E402

SHAPES = [(8, 1000), (64, 1000), (256, 1000), (4096, 100)]


def host_ransac(pts, t, seed=0, confidence=0.99, max_iters=1000):
    """The sequential algorithm in fp64 numpy (it stops at niters like OpenCV): (best count, iterations)."""
    best, niters, k = 0, max_iters, 0
    while k < niters:
        idx = ref.draw_sample(seed, k, pts)
        if idx is None:
            break
        for F in ref.seven_point(pts[idx]):
            c = int((ref.errors(F, pts) <= t * t).sum())
            if c > max(best, 6):
                best = c
                niters = ref.update_num_iters(confidence, (len(pts) - c) / len(pts), niters)
        k += 1
    return best, k


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
    ap.add_argument("--host-pairs", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ransac_time.py needs a GPU")
    fout = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        fout = open(a.out, "w")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if fout is not None:
            fout.write(line + "\n")

    for B, N in SHAPES:
        sc = dfepe.synth.make_scene(B, N, seed=B + N, outlier_ratio=0.3)
        m, K = sc["matches_xy_ori"].cuda(), sc["Ks"].cuda()
        for t in (0.1, 1.0):
            out = dfepe.ops.ransac_fundamental(m, threshold=t)
            it = out["iters_run"].float()
            us_f = time_call(lambda: dfepe.ops.ransac_fundamental(m, threshold=t), a.reps)
            us_p = time_call(lambda: dfepe.ops.ransac_pose(m, K, threshold=t), a.reps)
            emit({"what": "device", "B": B, "N": N, "threshold": t, "max_iters": 1000, "fundamental_us": round(us_f, 1),
                  "fundamental_us_per_pair": round(us_f / B, 3), "pose_us": round(us_p, 1), "pose_us_per_pair": round(us_p / B, 3),
                  "iters_run_mean": round(float(it.mean()), 1), "iters_run_max": int(it.max()),
                  "inliers_mean": round(float(out["n_inliers"].float().mean()), 1)})
            pts = sc["matches_xy_ori"].numpy()
            t0 = time.perf_counter()
            host = [host_ransac(pts[b], t) for b in range(min(a.host_pairs, B))]
            dt = (time.perf_counter() - t0) / len(host)
            emit({"what": "host fp64 numpy restatement, one core (not OpenCV)", "N": N, "threshold": t, "ms_per_pair": round(dt * 1e3, 1),
                  "iters": [h[1] for h in host], "device_iters": out["iters_run"][:len(host)].tolist()})
    if fout is not None:
        fout.close()


if __name__ == "__main__":
    main()
