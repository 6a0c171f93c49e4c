"""Time the batched RANSAC homography estimator (ops.ransac_homography) and the two evaluation measures with device events after
warm-up, at (B, N) in {(8, 1000), (64, 1000), (256, 1000), (4096, 100)}, max_iters 2000 (cv2's default), thresholds 1 / 3 / 5 px
on synthetic pairs of a 240 x 320 image (30 % outliers, 0.5 px noise).  For scale, the fp64 numpy restatement of the same
sequential algorithm (tests/homography_ref.py) on ONE host core -- OpenCV is not a dependency of the project, so it is not
timed.  Needs a GPU; prints one JSON line per measurement.

    python scripts/homography_time.py [--reps 20] [--host-pairs 2] [--out FILE.jsonl] [--shapes 8x1000,64x1000]
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
import homography_cases as hc  # noqa: E402
import homography_ref as ref  # noqa: E402

SHAPES = [(8, 1000), (64, 1000), (256, 1000), (4096, 100)]


def host_ransac(pts, t, seed=0, confidence=0.995, max_iters=2000):
    """The sequential algorithm in fp64 numpy (it stops at niters like OpenCV), refit and refinement included: (count, iterations)."""
    best, niters, k, Hb = 0, max_iters, 0, None
    while k < niters:
        idx = ref.draw_sample(seed, k, pts)
        if idx is None:
            break
        H, _ = ref.solve4(pts[idx])
        if H is not None:
            c = int((ref.errors(H, pts) <= t * t).sum())
            if c > max(best, 3):
                best, Hb = c, H
                niters = ref.update_num_iters4(confidence, (len(pts) - c) / len(pts), niters)
        k += 1
    if Hb is not None:
        pin = pts[ref.errors(Hb, pts) <= t * t]
        Hr = ref.refit(pin)
        ref.lm_refine((Hb if Hr is None else Hr).reshape(-1)[:8], pin)
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
    ap.add_argument("--shapes", default=None, help="comma-separated BxN list instead of the default four")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("homography_time.py needs a GPU")
    shapes = SHAPES if a.shapes is None else [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    fout = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        fout = open(a.out, "w")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if fout is not None:
            fout.write(line + "\n")

    for B, N in shapes:
        gen = [hc.synth(10 * B + b, N, 0.3, 0.5) for b in range(B)]
        pts = np.stack([g[0] for g in gen])
        m = torch.as_tensor(pts, device="cuda")
        Hgt = torch.as_tensor(np.stack([g[1] for g in gen]), device="cuda")
        th = torch.tensor([1.0, 3.0, 5.0], dtype=torch.float64, device="cuda")
        for t in (1.0, 3.0, 5.0):
            out = dfepe.ops.ransac_homography(m, threshold=t)
            it = out["iters_run"].float()
            us = time_call(lambda: dfepe.ops.ransac_homography(m, threshold=t), a.reps)
            us_nr = time_call(lambda: dfepe.ops.ransac_homography(m, threshold=t, refine=False), a.reps)
            us_tr = time_call(lambda: dfepe.ops.homography_transfer(out["H"], m, None, t), a.reps)
            us_co = time_call(lambda: dfepe.ops.homography_corners(out["H"], Hgt, hc.HEIGHT, hc.WIDTH, th), a.reps)
            md, ok = dfepe.ops.homography_corners(out["H"], Hgt, hc.HEIGHT, hc.WIDTH, th)
            emit({"what": "device", "B": B, "N": N, "threshold": t, "max_iters": 2000, "homography_us": round(us, 1),
                  "homography_us_per_pair": round(us / B, 3), "no_refine_us": round(us_nr, 1), "transfer_us": round(us_tr, 1),
                  "corners_us": round(us_co, 1), "iters_run_mean": round(float(it.mean()), 1), "iters_run_max": int(it.max()),
                  "inliers_mean": round(float(out["n_inliers"].float().mean()), 1), "correct_at_1_3_5": ok.float().mean(0).tolist()})
            if a.host_pairs < 1:
                continue
            t0 = time.perf_counter()
            host = [host_ransac(pts[b], t) for b in range(min(a.host_pairs, B))]
            dt = (time.perf_counter() - t0) / len(host)
            emit({"what": "host fp64 numpy restatement, one core (not OpenCV)", "N": N, "threshold": t, "ms_per_pair": round(dt * 1e3, 1),
                  "iters": [h[1] for h in host], "device_iters": out["iters_run"][:len(host)].tolist()})
    if fout is not None:
        fout.close()


if __name__ == "__main__":
    main()
