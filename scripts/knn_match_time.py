"""Timing of the ratio-test 2-NN matcher (ops.knn_match) against the project's own two-way matcher (ops.nn_match_two_way) at the same
B, N and D -- the same MFMA work -- and against the fp32 MFMA roofline; for context, the host cost of the float64 restatement
(tests/knn_ref.py) per pair.  Same method as scripts/match_time.py: HIP events around `reps` back-to-back calls after a warm-up, here
in several blocks that alternate the two ops, so that a drift of the clocks or a neighbour on the host shows as spread, not as a
difference.  Prints a markdown table (profiles/knn_match.md is this output).

    python scripts/knn_match_time.py [--reps 100] [--blocks 7]"""
import argparse
import importlib
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
PEAK_FP32_MFMA = 157.3e12  # FLOP/s, the figure scripts/match_time.py uses


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
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--blocks", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("knn_match_time.py needs a GPU: nothing is measured without one")
    d = importlib.import_module("pytorch-deepfepe_amd")
    import knn_ref as kr

    print(f"device: {torch.cuda.get_device_name(0)}; {args.blocks} alternating blocks of {args.reps} calls per op, HIP events; "
          f"median (min .. max) of the blocks\n")
    print("| B | N1 = N2 | D | knn_match ms | nn_match_two_way ms | ratio | knn_match TFLOP/s (share of fp32 MFMA peak) | good rows / pair |")
    print("|---|---|---|---|---|---|---|---|")
    host = None
    for B, N, D in ((64, 1024, 128), (64, 2000, 128), (64, 1024, 256)):
        g = torch.Generator().manual_seed(0)
        d1 = torch.nn.functional.normalize(torch.randn(B, N, D, generator=g), dim=2)
        d2 = torch.nn.functional.normalize(d1[:, torch.randperm(N, generator=g)] + 0.05 * torch.randn(B, N, D, generator=g), dim=2)
        a, b = d1.cuda(), d2.cuda()
        ops = {"knn": lambda: d.ops.knn_match(a, b, 0.8), "nn": lambda: d.ops.nn_match_two_way(a, b, 0.7)}
        for f in ops.values():  # warm-up: code objects, the allocator's blocks of both ops
            for _ in range(5):
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in ops}
        for _ in range(args.blocks):
            for k, f in ops.items():
                times[k].append(block(f, args.reps))
        med = {k: statistics.median(v) for k, v in times.items()}
        fmt = lambda k: f"{med[k] * 1e3:.3f} ({min(times[k]) * 1e3:.3f} .. {max(times[k]) * 1e3:.3f})"
        flop = 2.0 * B * N * N * D
        good = d.ops.knn_match(a, b, 0.8)[7].float().mean().item()
        print(f"| {B} | {N} | {D} | {fmt('knn')} | {fmt('nn')} | {med['knn'] / med['nn']:.2f} | "
              f"{flop / med['knn'] / 1e12:.1f} ({100 * flop / med['knn'] / PEAK_FP32_MFMA:.0f} %) | {good:.0f} |", flush=True)
        if (B, N, D) == (64, 1024, 128):
            t0 = time.perf_counter()
            for k in range(4):
                kr.PairRef(d1[k].numpy(), d2[k].numpy()).answer(0.8)
            host = (time.perf_counter() - t0) / 4
    print(f"\nhost cost of the float64 restatement (tests/knn_ref.py, numpy) at 1024 x 1024 x 128: {host * 1e3:.0f} ms per pair")


if __name__ == "__main__":
    main()
