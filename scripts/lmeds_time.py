"""Time the batched LMedS estimators (ops.lmeds_fundamental, ops.lmeds_essential) with device events after warm-up, at the two
shapes of profiles/lmeds.md: 8 pairs x 1000 correspondences (a validation batch) and 4096 pairs x 14 (the sparse pairs OpenCV
hands to LMedS), defaults otherwise (300 resp. the five-point rule's iterations), on synthetic pairs with 30 % outliers and 0.5 px
noise.  Next to each figure the RANSAC estimator of the same model on the same input (ops.ransac_fundamental at 0.1 px from 15
correspondences on, ops.ransac_essential at 1 px): context, not a bar.  Needs a GPU; prints one JSON line per measurement.

    python scripts/lmeds_time.py [--reps 10] [--out FILE.jsonl]

The split over the three launches comes from the same script under the profiler:
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/lmeds_time.py --reps 3
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

SHAPES = [(8, 1000), (4096, 14)]


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
        raise SystemExit("lmeds_time.py needs a GPU")
    fout = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        fout = open(a.out, "w")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if fout is not None:
            fout.write(line + "\n")

    ops = dfepe.ops
    for B, N in SHAPES:
        sc = dfepe.synth.make_scene(B, N, seed=B + N, outlier_ratio=0.3)
        m, K = sc["matches_xy_ori"].cuda(), sc["Ks"].cuda()
        out = ops.lmeds_fundamental(m)
        rec = {"B": B, "N": N, "max_iters": 1000,
               "lmeds_fundamental_us": round(time_call(lambda: ops.lmeds_fundamental(m), a.reps), 1),
               "lmeds_fundamental_niters": int(out["iters_run"].max()),
               "lmeds_fundamental_inliers_mean": round(float(out["n_inliers"].float().mean()), 1),
               "lmeds_pose_us": round(time_call(lambda: ops.lmeds_pose(m, K), a.reps), 1)}
        if N >= 15:  # below, the RANSAC entry refuses: that is the case LMedS exists for
            rec["ransac_fundamental_us"] = round(time_call(lambda: ops.ransac_fundamental(m, threshold=0.1), a.reps), 1)
        out = ops.lmeds_essential(m, K)
        rec.update({"lmeds_essential_us": round(time_call(lambda: ops.lmeds_essential(m, K), a.reps), 1),
                    "lmeds_essential_niters": int(out["iters_run"].max()),
                    "lmeds_essential_inliers_mean": round(float(out["n_inliers"].float().mean()), 1),
                    "ransac_essential_us": round(time_call(lambda: ops.ransac_essential(m, K, threshold=1.0), a.reps), 1)})
        emit(rec)
    if fout is not None:
        fout.close()


if __name__ == "__main__":
    main()
