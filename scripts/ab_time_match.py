"""Same-box A/B timing of the two descriptor matchers between two builds of libdfepe_hip.so, one process per library and round.
usage (GPU box), alternately, at least 5 rounds:
    DFEPE_LIB_PATH=<build A> python scripts/ab_time_match.py >> a.jsonl
    DFEPE_LIB_PATH=<build B> python scripts/ab_time_match.py >> b.jsonl
    python scripts/ab_time_match.py --table a.jsonl b.jsonl
A run times ops.nn_match_two_way and ops.knn_match at the shapes of scripts/knn_match_time.py (B = 64; N1 = N2 = 1024 and 2000 at
D = 128, 1024 at D = 256): blocks of 100 calls between device events after a warm-up, one JSON line per op and shape with the median
of 7 blocks.  --table: per op and shape the median over the rounds of A and of B, A's own spread s = (max - min) / median over its
rounds, the ratio B / A, and whether B <= A (1 + s)."""
import importlib, json, os, statistics, sys
SHAPES = ((64, 1024, 128), (64, 2000, 128), (64, 1024, 256))
def table(path_a, path_b):
    rounds = []
    for p in (path_a, path_b):
        r = {}
        for line in open(p):
            if line.startswith("{"):
                j = json.loads(line)
                r.setdefault((j["op"], j["B"], j["N"], j["D"]), []).append(j["ms"])
        rounds.append(r)
    print("| op | B | N1 = N2 | D | A ms (median of rounds) | B ms | rounds | s = A's (max - min) / median | B / A | B <= A (1 + s) |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    ok = True
    for key, a in rounds[0].items():
        b = rounds[1][key]
        ma, mb = statistics.median(a), statistics.median(b)
        s = (max(a) - min(a)) / ma
        ok &= mb <= ma * (1 + s)
        print(f"| {key[0]} | {key[1]} | {key[2]} | {key[3]} | {ma:.4f} | {mb:.4f} | {len(a)} / {len(b)} | {s:.4f} | {mb / ma:.4f} | "
              f"{'yes' if mb <= ma * (1 + s) else 'NO'} |")
    return 0 if ok else 1
if len(sys.argv) == 4 and sys.argv[1] == "--table":
    sys.exit(table(sys.argv[2], sys.argv[3]))
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
d = importlib.import_module("pytorch-deepfepe_amd")
def t(f, n=100):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n
for B, N, D in SHAPES:
    g = torch.Generator().manual_seed(0)
    d1 = torch.nn.functional.normalize(torch.randn(B, N, D, generator=g), dim=2)
    d2 = torch.nn.functional.normalize(d1[:, torch.randperm(N, generator=g)] + 0.05 * torch.randn(B, N, D, generator=g), dim=2)
    a, b = d1.cuda(), d2.cuda()
    ops = {"nn_match_two_way": lambda: d.ops.nn_match_two_way(a, b, 0.7), "knn_match": lambda: d.ops.knn_match(a, b, 0.8)}
    for f in ops.values():
        for _ in range(20): f()
    torch.cuda.synchronize()
    ts = {k: [] for k in ops}
    for blk in range(7):
        for k, f in ops.items(): ts[k].append(t(f))
    for k in ops:
        print(json.dumps({"lib": d._lib.LIB_PATH, "op": k, "B": B, "N": N, "D": D, "ms": statistics.median(ts[k]),
                          "min": min(ts[k]), "max": max(ts[k])}), flush=True)
