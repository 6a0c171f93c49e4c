"""Timing of the on-device KITTI odometry table (compat.eval_tools.odometry_table: dfepe_pose_chain + dfepe_trajectory_align +
dfepe_kitti_odometry_errors) for one KITTI-sized sequence (S = 1, n = 1591 frames) and for a batch of eleven of them (S = 11),
against the numpy restatement of the same evaluation (tests/kitti_odom_ref.py) on the same machine's host.  No speed bar is
attached: the work is a few hundred kilobytes and launch-latency-sized; the figures say what finishing the evaluation on the
stream costs.

Method: HIP events around `reps` back-to-back calls after a warm-up, in several blocks; median (min .. max) of the blocks; the two
new kernels also one by one (ops.trajectory_align, ops.kitti_odometry_errors).  The host side is timed once per case with
time.perf_counter.  Prints a markdown table (profiles/kitti_odom.md is this output).

    python scripts/kitti_odom_time.py [--reps 50] [--blocks 5]"""
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
        raise SystemExit("kitti_odom_time.py needs a GPU: nothing is measured without one")
    d = importlib.import_module("pytorch-deepfepe_amd")
    import kitti_odom_cases as C
    import kitti_odom_ref as K

    n = 1591
    print(f"device: {torch.cuda.get_device_name(0)}; {args.blocks} blocks of {args.reps} calls, HIP events; median (min .. max) of the "
          f"blocks; n = {n} frames per sequence, alignment scale_7dof, step 10\n")
    print("| S | odometry_table us | trajectory_align us | kitti_odometry_errors us | host restatement ms |")
    print("|---|---|---|---|---|")
    for S in (1, 11):
        pairs = [C.trajectory(np.random.RandomState(70 + s), n) for s in range(S)]
        est, gt = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        # relative camera motions whose chain is the estimate: rel_k = inv(abs_k) abs_k-1, so that pose_chain has real work
        rel = np.stack([K.mul(K.inv(e[1:], "closed"), e[:-1]) for e in est])
        rel_d = torch.as_tensor(rel.reshape(S, n - 1, 3, 4), device="cuda")
        est_d, gt_d = (torch.as_tensor(a.reshape(S, n, 3, 4), device="cuda") for a in (est, gt))
        al = d.ops.trajectory_align(est_d, gt_d, "scale_7dof")
        fs = {"table": lambda: d.compat.eval_tools.odometry_table(rel_d, None, gt_d),
              "align": lambda: d.ops.trajectory_align(est_d, gt_d, "scale_7dof"),
              "errors": lambda: d.ops.kitti_odometry_errors(al["est"], al["gt"])}
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
            K.evaluate(est[s], gt[s], "scale_7dof")
        host = time.perf_counter() - t0
        print(f"| {S} | {fmt('table')} | {fmt('align')} | {fmt('errors')} | {host * 1e3:.0f} |", flush=True)


if __name__ == "__main__":
    main()
