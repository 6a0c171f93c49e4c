"""Time the correspondence evaluation with device events after warm-up: one compat.correspondence_eval_batch (descriptor matching,
gather, ops.inlier_table, ops.inlier_table_mean) at B = 8 pairs of n = 1000 keypoints with 256-dimensional descriptors, 16 inlier
and 16 mask thresholds, and its two table launches alone; for scale the same table from the same matches by the fp64 numpy
restatement of the tests (tests/corr_eval_ref.py, one host core).  Recorded, not gated.  Needs a GPU; prints one JSON line.

    python scripts/corr_eval_time.py [--reps 50] [--out FILE.jsonl]
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
import corr_eval_cases as cc  # noqa: E402
import corr_eval_ref as cr  # noqa: E402

B, N, D = 8, 1000, 256


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


def inputs():
    """Image 2 holds a permuted, perturbed copy of image 1's descriptors; the keypoints are a corr_eval_cases scene."""
    g = np.random.RandomState(5)
    m, F, _ = cc.scene(6, B, N)
    d1 = g.randn(B, N, D)
    d1 /= np.linalg.norm(d1, axis=2, keepdims=True)
    d2, p2 = np.zeros_like(d1), np.zeros((B, N, 2), np.float32)
    for b in range(B):
        perm = g.permutation(N)
        moved = d1[b] + g.randn(N, D) / np.sqrt(D) * g.uniform(0.05, 0.9, (N, 1))
        d2[b, perm] = moved / np.linalg.norm(moved, axis=1, keepdims=True)
        p2[b, perm] = m[b, :, 2:]
    return m[:, :, :2].copy(), p2, d1.astype(np.float32), d2.astype(np.float32), F


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("corr_eval_time.py needs a GPU")
    dev = "cuda:0"
    p1, p2, d1, d2, F = (torch.as_tensor(v, device=dev) for v in inputs())
    it = torch.tensor(cc.ITHDS[16], dtype=torch.float64, device=dev)
    mt = torch.tensor(cc.MTHDS[16], dtype=torch.float64, device=dev)
    run = lambda: dfepe.compat.correspondence_eval_batch((p1, p2), (d1, d2), F, 0.7, it, mt)  # noqa: E731
    out = run()
    us_batch = time_call(run, a.reps)
    xs, sc, nv = out["matches"], out["mscores"], out["num_matches"]

    def tables():
        r = dfepe.ops.inlier_table(matches=xs, F=F, scores=sc, n_valid=nv, inlier_thds=it, mask_thds=mt, want=("cnt", "num", "ratio", "dist_out"))
        return dfepe.ops.inlier_table_mean(r["ratio"], r["num"])

    us_tables = time_call(tables, a.reps)
    host = [v.cpu().numpy() for v in (xs, F, sc, nv)]
    cr.inlier_table(matches=host[0], F=host[1], scores=host[2], n_valid=host[3], inlier_thds=cc.ITHDS[16], mask_thds=cc.MTHDS[16])  # untimed
    t0 = time.perf_counter()
    ref = cr.inlier_table(matches=host[0], F=host[1], scores=host[2], n_valid=host[3], inlier_thds=cc.ITHDS[16], mask_thds=cc.MTHDS[16])
    ms_host = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(ref["num"], out["num"].cpu().numpy())
    line = {"B": B, "n": N, "D": D, "Ti": 16, "Tm": 16, "matches_per_pair": [int(v) for v in host[3]],
            "correspondence_eval_batch_us": round(us_batch, 1), "inlier_table_and_mean_us": round(us_tables, 1),
            "host_restatement_table_ms": round(ms_host, 2)}
    print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
