"""Time the sampling of the DSAC minimal sets, on the host and on the device, and the training step with either; the median over
blocks, the routes alternating inside every block, at B x N x H = 1 x 1000 x 64, 8 x 1000 x 128, 8 x 2000 x 256 and 64 x 100 x 64
(scripts/dsac_adjoint_time.py's sizes, scene and settings).

  1  the host route of compat.dsac_batch without a sampler: random.sample per hypothesis (perf_counter around the list comprehension
     alone: host_draw), then torch.tensor and the copy, ended by a synchronise (host_route)
  2  ops.sample_sets, uniform and weighted (device events around the calls: the host cost of the eager call is inside)
  3  the step = compat.dsac_batch forward + autograd of exp_loss + sum(quality):
       host_step     the host draw included (a fresh seed every call)
       device_step   with a compat.DeviceSampler, eager
       graph_step    the same, captured once in a torch.cuda.graph and replayed (every replay draws the next offset)
     device events around the calls AND perf_counter around the same calls ended by a synchronise (wall): the host draw happens
     while the stream is idle, so both contain it.

The condition set beforehand: at every size device_step is not slower than host_step by more than the block-to-block spread of the
two (max - min over the blocks).  Printed per size as `condition_holds`.

    python scripts/dsac_sampler_time.py [--blocks 9] [--reps 5] [--out FILE.json]
"""
import argparse
import importlib
import json
import os
import random
import statistics
import sys
import time

import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "scripts")]
dfepe = importlib.import_module("pytorch-deepfepe_amd")
import dsac_cases as dc  # noqa: E402
import dsac_time as dt  # noqa: E402

BETA = 0.002


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dsac_sampler_time.py needs a GPU")
    C = dfepe.compat
    rows = []
    for B, N, H in dt.SIZES:
        X, Y, K = (torch.from_numpy(t).to(dt.DEV) for t in dc.scene(B, N, 5, 0.0))
        X.requires_grad_()
        Y.requires_grad_()
        weights = torch.rand(B, N, device=dt.DEV) + 0.01
        seeds = iter(range(1, 1 << 30))
        sampler = C.DeviceSampler(5, dt.DEV)
        host_draw = []

        def host_route():
            rng = random.Random(next(seeds))
            t0 = time.perf_counter()
            lists = [C.dsac._draw(N, H, dt.S, rng) for _ in range(B)]
            host_draw.append((time.perf_counter() - t0) * 1e6)
            return torch.tensor(lists, dtype=torch.int32).reshape(B, H, dt.S).to(dt.DEV)

        def uniform():
            return dfepe.ops.sample_sets(B, N, H, dt.S, seed=5, counter=sampler.counter)

        def weighted():
            return dfepe.ops.sample_sets(B, N, H, dt.S, seed=5, counter=sampler.counter, weights=weights)

        def step(**kw):
            out = C.dsac_batch(X, Y, K, H, dc.THRESH, BETA, dc.ALPHA, loss_kind=1, want=("exp_loss",), **kw)
            return torch.autograd.grad(out["exp_loss"].sum() + out["quality"].sum(), (X, Y))

        def host_step():
            return step(seed=next(seeds))

        def device_step():
            return step(sampler=sampler)

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                device_step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            device_step()

        routes = {"host_route": host_route, "uniform": uniform, "weighted": weighted, "host_step": host_step, "device_step": device_step,
                  "graph_step": graph.replay}
        for fn in routes.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        host_draw.clear()
        ev, wall = {k: [] for k in routes}, {k: [] for k in routes}
        for _ in range(a.blocks):
            for k, fn in routes.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                for _ in range(a.reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                wall[k].append((time.perf_counter() - t0) * 1e6 / a.reps)
                ev[k].append(e0.elapsed_time(e1) * 1e3 / a.reps)
        row = {"B": B, "N": N, "H": H, "launches": {k: dt.launches(routes[k]) for k in ("uniform", "weighted", "host_step", "device_step")}}
        per_block = [statistics.mean(host_draw[i * a.reps:(i + 1) * a.reps]) for i in range(a.blocks)]
        row["host_draw_us"] = round(statistics.median(per_block), 1)
        row["host_draw_us_min_max"] = [round(min(per_block), 1), round(max(per_block), 1)]
        for k in routes:
            src = wall if k == "host_route" else ev  # nothing of the host route but its copy is on the stream
            row[f"{k}_us"] = round(statistics.median(src[k]), 1)
            row[f"{k}_us_min_max"] = [round(min(src[k]), 1), round(max(src[k]), 1)]
            if k.endswith("_step"):
                row[f"{k}_wall_us"] = round(statistics.median(wall[k]), 1)
        spread = max(max(ev[k]) - min(ev[k]) for k in ("host_step", "device_step"))
        row["spread_us"] = round(spread, 1)
        row["condition_holds"] = bool(row["device_step_us"] <= row["host_step_us"] + spread)
        rows.append(row)
        print(json.dumps(row), flush=True)
    line = {"what": "DSAC sampling, host and device, and the step with either; us per call, median over blocks", "blocks": a.blocks,
            "reps": a.reps, "condition_holds_everywhere": all(r["condition_holds"] for r in rows), "rows": rows}
    print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
