"""Time the detector evaluation (ops.keypoint_repeatability: its three launches; ops.average_precision) with device events after
warm-up, at B in {1, 64} pairs of N = 300 and N = 1000 keypoints per image (keep_k = 300, one threshold; the average precision
over M = N entries), and for scale the fp64 restatement of the tests (numpy, one host core) per pair: recorded, not gated.  Needs
a GPU; prints one JSON line per measurement.

    python scripts/detector_eval_time.py [--reps 50] [--out FILE.jsonl]
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
import detector_eval_cases as dc  # noqa: E402
import detector_eval_ref as dr  # noqa: E402

SHAPES = [(1, 300), (64, 300), (1, 1000), (64, 1000)]
KEEP_K = 300


def time_call(fn, reps):
    for _ in range(5):
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
        raise SystemExit("detector_eval_time.py needs a GPU")
    lines = []
    dev = "cuda:0"
    th = torch.tensor([3.0], dtype=torch.float64, device=dev)
    for B, N in SHAPES:
        pairs = [dc.seeded_pair(1000 + b, N, N) for b in range(B)]
        kp1 = torch.as_tensor(np.stack([p[0] for p in pairs]), device=dev)
        kp2 = torch.as_tensor(np.stack([p[1] for p in pairs]), device=dev)
        H = torch.as_tensor(np.stack([p[2] for p in pairs]), device=dev)
        us = time_call(lambda: dfepe.ops.keypoint_repeatability(kp1, kp2, H, dc.HEIGHT, dc.WIDTH, KEEP_K, th), a.reps)
        vec = [dc.ap_vector(2000 + b, N, "tied") for b in range(B)]
        lab = torch.as_tensor(np.stack([v[0] for v in vec]), device=dev)
        sc = torch.as_tensor(np.stack([v[1] for v in vec]), device=dev)
        us_ap = time_call(lambda: dfepe.ops.average_precision(lab, sc), a.reps)
        n_host = min(B, 4)
        dr.repeatability_pair(*pairs[0], dc.HEIGHT, dc.WIDTH, KEEP_K, [3.0])  # untimed: numpy's first-call costs
        t0 = time.perf_counter()
        for b in range(n_host):
            dr.repeatability_pair(*pairs[b], dc.HEIGHT, dc.WIDTH, KEEP_K, [3.0])
        ms_rep = (time.perf_counter() - t0) * 1e3 / n_host
        t0 = time.perf_counter()
        for b in range(n_host):
            dr.average_precision(*vec[b])
        ms_ap = (time.perf_counter() - t0) * 1e3 / n_host
        lines.append({"B": B, "N": N, "keypoint_repeatability_us": round(us, 1), "average_precision_us": round(us_ap, 1),
                      "host_restatement_repeatability_ms_per_pair": round(ms_rep, 2), "host_restatement_ap_ms_per_pair": round(ms_ap, 2)})
        print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(l) + "\n" for l in lines)


if __name__ == "__main__":
    main()
