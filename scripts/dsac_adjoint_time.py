"""Time forward + backward of the DSAC loop with device events after warm-up, the median over blocks, the routes alternating inside
every block:
  fused      ops.dsac with X and Y requiring grad, then autograd of exp_loss + sum(quality): dfepe_dsac (six launches) and
             dfepe_dsac_bwd (eight launches)
  composed   scripts/dsac_time.py's `composed` loop with X and Y requiring grad, the same scalar built in torch, then autograd: every
             op of it has an adjoint (ops.eight_point, ops.epi_metrics, ops.epi_loss, torch's own)
  forward    ops.dsac without grad, for the share of the forward
at B x N x H = 1 x 1000 x 64, 8 x 1000 x 128, 8 x 2000 x 256 and 64 x 100 x 64.  The scene has no outliers and beta = 0.002: the
composed route's float32 sqrt(1 - sigmoid) backpropagates NaN as soon as one weight is exactly 0, the fused route does not care.
Also printed: the launches per call (torch's profiler, outside the timed window) and the largest difference of the two gradients.
Recorded, not gated.

    python scripts/dsac_adjoint_time.py [--blocks 9] [--reps 5] [--out FILE.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

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
    ap.add_argument("--routes", default="fused,composed,forward", help="comma-separated subset of the routes (a kernel trace wants one)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dsac_adjoint_time.py needs a GPU")
    rows = []
    for B, N, H in dt.SIZES:
        X, Y, K = (torch.from_numpy(t).to(dt.DEV) for t in dc.scene(B, N, 5, 0.0))
        idx = torch.from_numpy(dc.draw(B, N, H, dt.S, 5)).to(dt.DEV)
        X.requires_grad_()
        Y.requires_grad_()

        def fused():
            out = dfepe.ops.dsac(X, Y, K, idx, dc.THRESH, BETA, dc.ALPHA, loss_kind=1, want=("exp_loss",))
            return torch.autograd.grad(out["exp_loss"].sum() + out["quality"].sum(), (X, Y))

        def composed():
            quality, score, loss = dt.composed(X, Y, K, idx, dc.THRESH, BETA)
            exp_loss = (torch.softmax(dc.ALPHA * score, 1) * loss).sum()
            return torch.autograd.grad(exp_loss + quality.sum(), (X, Y))

        def forward():
            with torch.no_grad():
                return dfepe.ops.dsac(X, Y, K, idx, dc.THRESH, BETA, dc.ALPHA, loss_kind=1, want=("exp_loss",))["quality"]

        routes = {k: fn for k, fn in (("fused", fused), ("composed", composed), ("forward", forward)) if k in a.routes.split(",")}
        row = {"B": B, "N": N, "H": H, "launches": {k: dt.launches(fn) for k, fn in routes.items()}}
        if "fused" in routes and "composed" in routes:
            gf, gc = fused(), composed()
            torch.cuda.synchronize()
            row.update(fused_finite=bool(torch.isfinite(gf[0]).all() and torch.isfinite(gf[1]).all()),
                       composed_finite=bool(torch.isfinite(gc[0]).all() and torch.isfinite(gc[1]).all()),
                       grad_max_rel_diff=[float(((u - v).abs().max() / u.abs().max()).item()) for u, v in zip(gf, gc)])
        for fn in routes.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in routes}
        for _ in range(a.blocks):
            for k, fn in routes.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / a.reps)
        for k, v in times.items():
            row[f"{k}_us"] = round(statistics.median(v), 1)
            row[f"{k}_us_min_max"] = [round(min(v), 1), round(max(v), 1)]
        rows.append(row)
        print(json.dumps(row), flush=True)
    line = {"what": "DSAC loop forward + backward, us per call, median over blocks; launches per call", "blocks": a.blocks, "reps": a.reps,
            "rows": rows}
    print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
