"""Timing of the on-device odometry evaluation (compat.eval_tools.odometry_summary: dfepe_pose_chain + dfepe_snippet_errors) for one
KITTI-sized sequence (S = 1, n = 1591 relative poses, snippets of L = 5) and for a batch of eleven of them (S = 11), against the
numpy restatement of the reference's loops (tests/odometry_ref.py) on the same machine's host.  No speed bar is attached: the work
is a few hundred kilobytes and launch-latency-sized; the figures say what completing the path on the stream costs.

Method: HIP events around `reps` back-to-back calls after a warm-up, in several blocks; median (min .. max) of the blocks; the two
kernels also one by one (ops.pose_chain, ops.snippet_errors).  The host side is timed once per case with time.perf_counter.  Prints
a markdown table (profiles/odometry.md is this output).

    python scripts/odometry_time.py [--reps 50] [--blocks 5]"""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def block(f, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("odometry_time.py needs a GPU: nothing is measured without one")
    d = importlib.import_module("pytorch-deepfepe_amd")
    import odometry_cases as C
    import odometry_ref as R

    n, L = 1591, 5
    print(f"device: {torch.cuda.get_device_name(0)}; {args.blocks} blocks of {args.reps} calls, HIP events; median (min .. max) of the "
          f"blocks; n = {n} relative poses per sequence, L = {L}\n")
    print("| S | odometry_summary us | pose_chain us | snippet_errors us | host restatement ms (chain + snippets) |")
    print("|---|---|---|---|---|")
    for S in (1, 11):
        pairs = [C.trajectory(50 + s, n) for s in range(S)]
        g = np.random.RandomState(S)
        rel = np.stack([C.random_poses(g, n, max_angle=0.05) for _ in range(S)])
        c2b = C.random_poses(g, S, max_angle=0.2)
        gt = np.stack([p[1] for p in pairs])
        rel_d, c2b_d, gt_d = (torch.as_tensor(a, device="cuda") for a in (rel.reshape(S, n, 3, 4), c2b.reshape(S, 3, 4), gt.reshape(S, n + 1, 3, 4)))
        abs_d = d.ops.pose_chain(rel_d, cam2body=c2b_d)
        wn = torch.full((S,), n + 1 - L, dtype=torch.int32, device="cuda")
        fs = {"summary": lambda: d.compat.eval_tools.odometry_summary(rel_d, c2b_d, gt_d, L),
              "chain": lambda: d.ops.pose_chain(rel_d, cam2body=c2b_d),
              "snippets": lambda: d.ops.snippet_errors(abs_d, gt_d, L, windows=wn, capacity=n + 1 - L)}
        for f in fs.values():
            for _ in range(5):
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in fs}
        for _ in range(args.blocks):
            for k, f in fs.items():
                times[k].append(block(f, args.reps))
        fmt = lambda k: f"{statistics.median(times[k]) * 1e6:.1f} ({min(times[k]) * 1e6:.1f} .. {max(times[k]) * 1e6:.1f})"
        t0 = time.perf_counter()
        for s in range(S):
            a = R.chain_sequential(rel[s], c2b[s])
            R.snippet_errors(a, gt[s], n + 1 - L, L)
        host = time.perf_counter() - t0
        print(f"| {S} | {fmt('summary')} | {fmt('chain')} | {fmt('snippets')} | {host * 1e3:.0f} |", flush=True)


if __name__ == "__main__":
    main()
