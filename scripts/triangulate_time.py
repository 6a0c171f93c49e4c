"""Time one launch of the two-view structure entry points -- ops.triangulate, ops.two_view_structure (all outputs) and
ops.reproject -- with device events (3 warm-ups, 10 calls), at (B, N) = (8, 1000), the reference's own shape, and (4096, 1000),
BASELINE config 5's.  Alternating in the same run it also times ops.ransac_in_front on the same inputs: the existing kernel that
runs a one-candidate fp64 DLT per correspondence and stores 1 byte instead of up to 36.  Needs a GPU; prints one JSON line per
shape.

    python scripts/triangulate_time.py [--reps 10] [--rounds 3] [--out FILE.jsonl]
"""
import argparse
import importlib
import json
import os
import sys

import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)
dfepe = importlib.import_module("pytorch-deepfepe_amd")

SHAPES = [(8, 1000), (4096, 1000)]


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
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the four kernels; the minimum per kernel is reported")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("triangulate_time.py needs a GPU")
    ops = dfepe.ops
    lines = []
    for B, N in SHAPES:
        sc = dfepe.synth.make_scene(B, N, seed=B + N, outlier_ratio=0.3)
        m, K, E = sc["matches_xy_ori"].float().cuda(), sc["Ks"].float().cuda(), sc["E_gt"].float().cuda()
        Rt_cam, winner, _ = ops.cheirality(E, K, m, 50.0)
        X = ops.two_view_structure(Rt_cam, K, m, winner=winner)["X"]
        P1 = torch.cat((K, torch.zeros(B, 3, 1, device=K.device)), 2)
        R = Rt_cam[:, :, :3].transpose(1, 2)
        P2 = K @ torch.cat((R, -(R @ Rt_cam[:, :, 3:])), 2)
        calls = {
            "triangulate": lambda: ops.triangulate(P1, P2, m),
            "two_view_structure": lambda: ops.two_view_structure(Rt_cam, K, m, winner=winner),
            "reproject": lambda: ops.reproject(X, Rt_cam, K, 1241.0, 376.0, camera_motion=True),
            "ransac_in_front": lambda: ops.ransac_in_front(E, K, m, winner, 50.0),
        }
        best = {k: float("inf") for k in calls}
        for _ in range(a.rounds):
            for k, fn in calls.items():
                best[k] = min(best[k], time_call(fn, a.reps))
        line = {"B": B, "N": N}
        line.update({k + "_us": round(v, 1) for k, v in best.items()})
        line["two_view_structure_ns_per_point"] = round(best["two_view_structure"] * 1e3 / (B * N), 3)
        lines.append(line)
        print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(l) + "\n" for l in lines)


if __name__ == "__main__":
    main()
