"""Time forward + backward of the textbook eight-point essential-matrix solver (_E_from_XY after the K^-1 step) with gradients to the
points and the weights, with device events after warm-up, the median over blocks, the routes alternating inside every block:
  kernel    ops.eight_point: dfepe_w8pt_fwd, then dfepe_eight_point_bwd (one launch, two with several weight sets)
  forward   the same without a gradient: the forward launch alone, so that kernel - forward is what the adjoint costs
  torch     compat._autograd_paths.eight_point, one problem at a time: the route the mirrors took before the adjoint kernel existed
at DSAC's two shapes: 64 pairs x 16 hypotheses of 10 sampled points (1024 problems of 10 points, one weight set) and 8 pairs x 16
weight sets x 1000 points.  With the times goes, for pair 0 under its first weight set, the largest difference of each route's point
gradient from the fp64 restatement of the reference's rule (tests/eight_point_adjoint_ref.py: Hartley transforms constant), over the
largest entry: the torch route differentiates the transforms, so its figure is the size of that term, not a rounding error.
Recorded, not gated.  Needs a GPU; prints one JSON line and rewrites the generated table of profiles/eight_point_adjoint.md (the text
between its `<!-- generated: ... -->` markers; the prose around it is written by hand).

    python scripts/eight_point_adjoint_time.py [--blocks 7] [--reps 10] [--out FILE.jsonl] [--md profiles/eight_point_adjoint.md]
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
import eight_point_adjoint_cases as ec  # noqa: E402
import eight_point_adjoint_ref as er  # noqa: E402

SHAPES = ((1024, 1, 10, "64 pairs x 16 fits of 10 points"), (8, 16, 1000, "8 pairs x 16 weight sets x 1000 points"))


def inputs(B, S, N, dev):
    rng = np.random.default_rng(5)
    X, Y = np.empty((B, N, 2), np.float32), np.empty((B, N, 2), np.float32)
    for b in range(B):
        X[b], Y[b] = ec.scene_pair(N, rng, 1.0)
    w = None if S == 1 else rng.uniform(0.2, 1.2, (S, B, N)).astype(np.float32)
    G = rng.standard_normal((S, B, 3, 3)).astype(np.float32)
    t = lambda a, g=False: None if a is None else torch.as_tensor(a, device=dev).requires_grad_(g)  # noqa: E731
    return t(X, True), t(Y, True), t(w, True), t(G if S > 1 else G[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--md", default=os.path.join(REPO, "profiles", "eight_point_adjoint.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eight_point_adjoint_time.py needs a GPU")
    dev = "cuda:0"
    ap_ = dfepe.compat._autograd_paths
    rows = []
    for B, S, N, label in SHAPES:
        X, Y, w, G = inputs(B, S, N, dev)
        leaves = [t for t in (X, Y, w) if t is not None]

        def kernel():
            return torch.autograd.grad(dfepe.ops.eight_point(X, Y, w, essential=True), leaves, G)

        def forward():
            with torch.no_grad():
                return dfepe.ops.eight_point(X, Y, w, essential=True)

        def torch_route():
            outs = [ap_.eight_point(X[b], Y[b], None if w is None else w[s, b], essential=True) for s in range(S) for b in range(B)]
            return torch.autograd.grad(torch.stack(outs).reshape(G.shape), leaves, G)

        got = {"kernel": kernel(), "torch": torch_route()}
        Fk = forward().detach().cpu().numpy().reshape(S, B, 3, 3)
        Ft = torch.stack([ap_.eight_point(X[0].detach(), Y[0].detach(), None if w is None else w[0, 0].detach(), essential=True)])
        Gn = G.cpu().numpy().reshape(S, B, 3, 3)
        agree = {}
        for k, F0 in (("kernel", Fk[0, 0]), ("torch", Ft[0].cpu().numpy())):
            r = er.problem(X[0].detach().cpu().numpy(), Y[0].detach().cpu().numpy(), None if w is None else w[0, 0].detach().cpu().numpy(),
                           True, True, F0, Gn[0, 0])
            if S == 1:
                agree[k] = float(np.abs(got[k][0][0].cpu().numpy() - r.gX).max() / np.abs(r.gX).max())
            else:  # the point gradient is a sum over the sets: compare the weight gradient of the one problem instead
                agree[k] = float(np.abs(got[k][2][0, 0].cpu().numpy() - r.gw).max() / np.abs(r.gw).max())
        steps = {"kernel": (kernel, a.reps), "forward": (forward, a.reps), "torch": (torch_route, 1)}
        for fn, _ in steps.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in steps}
        for _ in range(a.blocks):
            for k, (fn, reps) in steps.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / reps)
        row = {"shape": label, "problems": B * S, "N": N}
        for k, v in times.items():
            row[f"{k}_us"] = round(statistics.median(v), 1)
            row[f"{k}_us_min_max"] = [round(min(v), 1), round(max(v), 1)]
        row["kernel_vs_restatement_rel"] = float(np.format_float_scientific(agree["kernel"], 2))
        row["torch_vs_restatement_rel"] = float(np.format_float_scientific(agree["torch"], 2))
        rows.append(row)
    line = {"what": "forward + backward of the eight-point E solver, gradients to points and weights; us per step, median over blocks",
            "blocks": a.blocks, "reps": a.reps, "rows": rows}
    print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    write_tables(a.md, {"times": table(rows)})


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


def table(rows):
    out = ["| shape | kernel route fwd+bwd (us) | forward alone (us) | torch route (us) | kernel vs fp64 rule | torch vs fp64 rule |",
           "|---|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['shape']} | {r['kernel_us']} ({r['kernel_us_min_max'][0]} .. {r['kernel_us_min_max'][1]}) | "
                   f"{r['forward_us']} ({r['forward_us_min_max'][0]} .. {r['forward_us_min_max'][1]}) | "
                   f"{r['torch_us']} ({r['torch_us_min_max'][0]} .. {r['torch_us_min_max'][1]}) | "
                   f"{r['kernel_vs_restatement_rel']:.1e} | {r['torch_vs_restatement_rel']:.1e} |")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    main()
