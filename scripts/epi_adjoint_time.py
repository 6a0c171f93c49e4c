"""Time forward + backward of a clamped _sym_epi_dist mean loss (get_loss_softmax, train_good_utils.py:55-61) with gradients to F and
to both point sets, with device events after warm-up, the median over blocks, the routes alternating inside every block:
  kernel    compat.train_good_utils.get_loss_softmax: dfepe_epi_metrics, torch's mean, dfepe_epi_metrics_bwd
  reduced   ops.epi_loss(0, ..., reduction="mean"): dfepe_epi_loss_fwd / dfepe_epi_loss_bwd, the per-point losses never written
  torch     compat._autograd_paths.sym_epi_dist(...).mean(): the route the mirrors took before the adjoint kernels existed
at 4096 x 100, 4096 x 1000 and 8 x 2000 homogeneous points [B,N,3].  With the times go the algorithmic bytes per second of the two
kernel routes (bytes the algorithm has to move, from the shapes: 24 B per point to read X and Y, 24 B to write their gradients,
4 B for a per-point loss or upstream value; F and g_F are 72 B per pair).  Every route's gradients are also compared with the torch
expressions evaluated in float64 on the same inputs (largest difference over the largest entry), so that a difference between the
routes can be read.  Recorded, not gated.  Needs a GPU; prints one JSON line and rewrites the two generated tables of
profiles/epi_adjoint.md (the text between its `<!-- generated: ... -->` markers; the prose around them is written by hand).

    python scripts/epi_adjoint_time.py [--blocks 15] [--reps 20] [--out FILE.jsonl] [--md profiles/epi_adjoint.md]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
dfepe = importlib.import_module("pytorch-deepfepe_amd")
import epi_adjoint_cases as ac  # noqa: E402

SIZES = ((4096, 100), (4096, 1000), (8, 2000))
CLAMP = 0.5


def bytes_of(route, B, N):
    """Algorithmic bytes of forward + backward."""
    pts, pair = B * N, B * 72
    if route == "reduced":   # fwd: read X, Y, F, write [B]; bwd: read X, Y, F, g_sum, write g_X, g_Y, g_F
        return (24 * pts + pair + 4 * B) + (48 * pts + 2 * pair + 4 * B)
    # fwd: + the [B,N] losses written, read by the mean; bwd: + the [B,N] upstream written by the mean's adjoint and read
    return (28 * pts + pair) + 4 * pts + 4 * pts + (52 * pts + 2 * pair)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--md", default=os.path.join(REPO, "profiles", "epi_adjoint.md"), help="the document whose generated tables are rewritten")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("epi_adjoint_time.py needs a GPU")
    dev = "cuda:0"
    ap_ = dfepe.compat._autograd_paths
    rows = []
    for B, N in SIZES:
        case = ac.make("scene", 0, B, N, True, seed=1)
        F, X, Y = (torch.as_tensor(case[k], device=dev).requires_grad_(True) for k in ("F", "X", "Y"))
        routes = {
            "kernel": lambda: dfepe.compat.train_good_utils.get_loss_softmax(F, X, Y, CLAMP)[0],
            "reduced": lambda: dfepe.ops.epi_loss(0, F, X, Y, clamp_at=CLAMP, eps=1e-10, reduction="mean"),
            "torch": lambda: ap_.sym_epi_dist(F, X, Y, True, CLAMP, eps=1e-10).mean(),
        }
        step = {k: (lambda fn=fn: torch.autograd.grad(fn(), (F, X, Y))) for k, fn in routes.items()}
        grads = {k: s() for k, s in step.items()}
        F64, X64, Y64 = (t.detach().double().requires_grad_(True) for t in (F, X, Y))
        exact = torch.autograd.grad(ap_.sym_epi_dist(F64, X64, Y64, True, CLAMP, eps=1e-10).mean(), (F64, X64, Y64))
        agree = {k: max(((g.double() - t).abs().max() / t.abs().max()).item() for g, t in zip(grads[k], exact)) for k in step}
        for s in step.values():  # warm-up of every shape the timed window uses
            for _ in range(10):
                s()
        torch.cuda.synchronize()
        times = {k: [] for k in step}
        for _ in range(a.blocks):
            for k, s in step.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    s()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / a.reps)
        row = {"B": B, "N": N}
        for k, v in times.items():
            row[f"{k}_us"] = round(statistics.median(v), 1)
            row[f"{k}_us_min_max"] = [round(min(v), 1), round(max(v), 1)]
        for k in ("kernel", "reduced"):
            row[f"{k}_algorithmic_GBps"] = round(bytes_of(k, B, N) / (row[f"{k}_us"] * 1e-6) / 1e9, 1)
        for k in step:
            row[f"{k}_max_grad_diff_vs_float64_rel"] = float(np.format_float_scientific(agree[k], 2))
        rows.append(row)
    line = {"what": "forward + backward of the clamped sym-epi mean loss, gradients to F, X, Y; us per step, median over blocks",
            "blocks": a.blocks, "reps": a.reps, "rows": rows}
    print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    write_tables(a.md, {"times": table(rows), "accuracy": accuracy_table(rows)})


def write_tables(path, tables):
    """Replace what stands between `<!-- generated: NAME -->` and `<!-- end: NAME -->` in the document; a new document is the tables."""
    text = open(path).read() if os.path.exists(path) else "".join(f"<!-- generated: {k} -->\n<!-- end: {k} -->\n\n" for k in tables)
    for name, body in tables.items():
        head, tail = f"<!-- generated: {name} -->\n", f"<!-- end: {name} -->"
        if head in text and tail in text:
            text = text[:text.index(head) + len(head)] + body + text[text.index(tail):]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)


def accuracy_table(rows):
    out = ["| pairs x points | torch route (fp32) | kernel route | reduced form |", "|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['B']} x {r['N']} | " + " | ".join(f"{r[k + '_max_grad_diff_vs_float64_rel']:.1e}" for k in ("torch", "kernel", "reduced")) + " |")
    return "\n".join(out) + "\n"


def table(rows):
    out = ["| pairs x points | torch route (us) | kernel route (us) | reduced form (us) | kernel route GB/s | reduced form GB/s |", "|---|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['B']} x {r['N']} | {r['torch_us']} ({r['torch_us_min_max'][0]} .. {r['torch_us_min_max'][1]}) | "
                   f"{r['kernel_us']} ({r['kernel_us_min_max'][0]} .. {r['kernel_us_min_max'][1]}) | "
                   f"{r['reduced_us']} ({r['reduced_us_min_max'][0]} .. {r['reduced_us_min_max'][1]}) | {r['kernel_algorithmic_GBps']} | "
                   f"{r['reduced_algorithmic_GBps']} |")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    main()
