"""Shared inputs of the correspondence-evaluation tests and the one check() that the host build of csrc/corr_eval_math.h and the
kernels of csrc/corr_eval.hip both go through (tests/test_corr_eval_ref_cpu.py, tests/test_corr_eval_gpu.py).

A case is a dict: matches [B,N,4] fp32 with F [B,3,3] fp64, or dist [B,N] fp32; scores [B,N] fp32 or None; n_valid [B] or None;
ithds, mthds (fp64 lists); listed: the undecided (pair, match, inlier threshold) triples the case is allowed, by index.  The random
cases list none: their undecided set must be empty (asserted by the CPU test, so the GPU test runs on decided inputs).
"""
import functools

import numpy as np

import corr_eval_ref as cr

IMAGE_W, IMAGE_H = 1241.0, 376.0
ITHDS = {1: [1.0], 2: [0.5, 2.0], 16: [float(v) for v in np.geomspace(0.05, 20.0, 16)]}
MTHDS = {1: [1.0], 2: [0.4, 1.0], 16: [float(v) for v in np.linspace(0.1, 1.3, 16)]}


def _rodrigues(w):
    th = np.linalg.norm(w)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def fundamental(g):
    """A KITTI-like ground-truth F of unit Frobenius norm: K^-T [t]x R K^-1 with a small rotation and a mostly forward motion."""
    K = np.array([[718.856, 0.0, 607.19], [0.0, 718.856, 185.22], [0.0, 0.0, 1.0]])
    R = _rodrigues(0.05 * g.randn(3) + 1e-3)
    t = g.randn(3) * np.array([0.1, 0.05, 0.3]) + np.array([0.0, 0.0, 1.0])
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K)
    F = Ki.T @ tx @ R @ Ki
    return F / np.linalg.norm(F)


def scene(seed, B, N):
    """(matches [B,N,4] fp32, F [B,3,3] fp64, scores [B,N] fp32): image-2 points on the epipolar line of their image-1 point, moved
    along the line's normal by 10^U(-2, 1.5) pixels, so the distances spread over every threshold; scores uniform in (0, 1.3)."""
    g = np.random.RandomState(seed)
    m = np.zeros((B, N, 4), np.float32)
    F = np.zeros((B, 3, 3))
    for b in range(B):
        F[b] = fundamental(g)
        x1 = g.rand(N, 2) * np.array([IMAGE_W, IMAGE_H])
        line = np.concatenate([x1, np.ones((N, 1))], 1) @ F[b].T
        nrm = line[:, :2] / np.linalg.norm(line[:, :2], axis=1, keepdims=True)
        foot = g.rand(N, 2) * np.array([IMAGE_W, IMAGE_H])
        foot = foot - nrm * ((np.sum(foot * line[:, :2], 1) + line[:, 2]) / np.linalg.norm(line[:, :2], axis=1))[:, None]
        off = 10.0 ** g.uniform(-2.0, 1.5, N) * g.choice([-1.0, 1.0], N)
        m[b] = np.concatenate([x1, foot + nrm * off[:, None]], 1).astype(np.float32)
    scores = (g.rand(B, N) * 1.3).astype(np.float32)
    return m, F, scores


def _case(name, seed, B, N, n_valid, Ti, Tm, with_scores=True):
    m, F, sc = scene(seed, B, N)
    return {"name": name, "matches": m, "F": F, "scores": sc if with_scores else None,
            "n_valid": None if n_valid is None else np.asarray(n_valid, np.int32), "ithds": ITHDS[Ti], "mthds": MTHDS[Tm] if with_scores else None,
            "listed": set()}


# every N of the launch (the empty pair, one row, one row either side of a wavefront and of the workgroup, several strides), every
# B, every n_valid kind mixed within a batch (0, 1, N - 1, N, N + 5 and -2: both clamped), every Ti and Tm
SHAPES = (
    ("n0", 101, 1, 0, None, 1, 1),
    ("n1", 102, 3, 1, [0, 1, 6], 2, 2),
    ("n63", 103, 1, 63, None, 16, 16),
    ("n64", 104, 3, 64, [63, 64, -2], 2, 1),
    ("n65", 105, 8, 65, [0, 1, 64, 65, 70, -2, 33, 65], 1, 2),
    ("n255", 106, 1, 255, None, 2, 2),
    ("n256", 107, 3, 256, [255, 256, 261], 16, 1),
    ("n257", 108, 3, 257, [257, 1, 0], 1, 16),
    ("n1000", 109, 8, 1000, [1000, 999, 1005, -2, 0, 1, 512, 257], 16, 16),
)


@functools.lru_cache(maxsize=None)
def shape_case(name):
    for s in SHAPES:
        if s[0] == name:
            return _case(*s)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def no_mask_case():
    """scores = None: everything is kept (Tm = 1 without a mask threshold)."""
    return _case("nomask", 110, 3, 130, [130, 7, 129], 2, 1, with_scores=False)


@functools.lru_cache(maxsize=None)
def edge_case():
    """The constructed edges, B = 4, N = 70 (more than one wavefront):
      pair 0  a scene with planted scores: equal to a mask threshold (not kept: strict), one fp32 step below it (kept), NaN and
              +inf (not kept); inlier threshold 1 is the restatement's own fp64 distance of match 5 (strict: no inlier where the
              evaluations agree to the bit; listed as undecided, being within the bound by construction)
      pair 1  F = [e]x with the integer epipole e = (3, 5): match 0 has x1 = e, so F x = 0 exactly and the distance is 0 * inf = NaN;
              match 1 has x2 = e (F^T y = 0): NaN too.  Both are kept by their scores and stay in the denominator
      pair 2  F = (0; 0; (1, 2, 3)): (F x)_12 = 0 for every x with a numerator that is not 0: every distance is +inf
      pair 3  every score above every mask threshold: nothing kept, ratio NaN, and the mean NaN
    The inlier thresholds end with +inf: every finite distance passes it, +inf and NaN do not."""
    B, N = 4, 70
    m, F, sc = scene(111, B, N)
    sc[0, 0] = 0.5
    sc[0, 1] = np.nextafter(np.float32(0.5), np.float32(0))
    sc[0, 2] = np.nan
    sc[0, 3] = np.inf
    sc[0, 4] = 1.0
    g = np.random.RandomState(112)
    F[1] = np.array([[0.0, -1.0, 5.0], [1.0, 0.0, -3.0], [-5.0, 3.0, 0.0]])
    m[1] = g.randint(0, 300, (N, 4)).astype(np.float32)
    m[1, 0, :2] = (3.0, 5.0)
    m[1, 1, 2:] = (3.0, 5.0)
    sc[1] = 0.1
    F[2] = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [1.0, 2.0, 3.0]])
    m[2] = g.randint(0, 300, (N, 4)).astype(np.float32)
    sc[2] = 0.3
    sc[3] = 2.0
    d5 = float(cr.dist3(F[0], m[0])[5])
    return {"name": "edge", "matches": m, "F": F, "scores": sc, "n_valid": None, "ithds": [1.0, d5, float("inf")], "mthds": [0.5, 1.0],
            "listed": {(0, 5, 1)}}


@functools.lru_cache(maxsize=None)
def dist_case():
    """dist input, B = 2, N = 66: distances equal to an inlier threshold, one fp32 step either side, 0, +inf and NaN; scores equal
    to a mask threshold.  Nothing is computed before the comparisons, so everything is decided."""
    B, N = 2, 66
    g = np.random.RandomState(113)
    d = (10.0 ** g.uniform(-2, 1.5, (B, N))).astype(np.float32)
    one = np.float32(1.0)
    d[0, :8] = (0.5, np.nextafter(np.float32(0.5), np.float32(0)), np.nextafter(np.float32(0.5), one), 1.0, np.nextafter(one, np.float32(0)),
                np.nextafter(one, np.float32(2)), 0.0, np.inf)
    d[1, 64:] = (np.nan, 0.5)
    sc = (g.rand(B, N) * 1.3).astype(np.float32)
    sc[0, :4] = (0.4, 1.0, 0.4, np.nextafter(one, np.float32(0)))
    sc[1, 64:] = (0.1, 0.1)
    return {"name": "dist", "dist": d, "F": None, "scores": sc, "n_valid": np.asarray([66, 70], np.int32), "ithds": [0.5, 1.0],
            "mthds": [0.4, 1.0], "listed": set()}


GOLDEN_SIZES = (1, 5, 40, 64, 65, 100, 130, 17, 33, 80, 200, 12)
GOLDEN_ITHDS = [0.1, 0.5, 1.0, 2.0, 5.0]
GOLDEN_MTHDS = [0.5, 1.0]
GOLDEN_NONE_KEPT = (3, 11)  # pairs whose scores are all >= 1: nothing kept under either mask threshold


def golden_inputs():
    """The dozen pairs of tests/golden/corr_eval.npz: a list of (matches [n,4] fp32, F [3,3] fp64, scores [n] fp32)."""
    out = []
    for k, n in enumerate(GOLDEN_SIZES):
        m, F, sc = scene(200 + k, 1, n)
        if k in GOLDEN_NONE_KEPT:
            sc = sc + np.float32(1.0)
        out.append((m[0], F[0], sc[0]))
    return out


def golden_padded():
    """golden_inputs() as one padded case."""
    pairs = golden_inputs()
    N = max(len(p[0]) for p in pairs)
    m, sc = np.zeros((len(pairs), N, 4), np.float32), np.zeros((len(pairs), N), np.float32)
    for b, (pm, _, ps) in enumerate(pairs):
        m[b, :len(pm)], sc[b, :len(pm)] = pm, ps
    return {"name": "golden", "matches": m, "F": np.stack([p[1] for p in pairs]), "scores": sc,
            "n_valid": np.asarray([len(p[0]) for p in pairs], np.int32), "ithds": GOLDEN_ITHDS, "mthds": GOLDEN_MTHDS, "listed": set()}


_EXPECTED = {}


def expected(case):
    """(the restatement's outputs, und [B,Tm,Ti]: the undecided kept matches per cell, the undecided triples) -- computed once."""
    key = case["name"]
    if key not in _EXPECTED:
        ref = cr.inlier_table(matches=case.get("matches"), F=case.get("F"), dist=case.get("dist"), scores=case["scores"],
                              n_valid=case["n_valid"], inlier_thds=case["ithds"], mask_thds=case["mthds"])
        B, Tm, Ti = ref["cnt"].shape
        und = np.zeros((B, Tm, Ti), np.int64)
        triples = set()
        if case.get("matches") is not None:
            n = cr.clamp_n(case["n_valid"], B, case["matches"].shape[1])
            for b in range(B):
                k = int(n[b])
                u = cr.undecided(case["F"][b], case["matches"][b, :k], case["ithds"])
                triples |= {(b, int(i), int(t)) for i, t in zip(*np.nonzero(u))}
                for m in range(Tm):
                    keep = np.ones(k, bool) if case["scores"] is None else case["scores"][b, :k].astype(np.float64) < case["mthds"][m]
                    und[b, m] = (u & keep[:, None]).sum(0)
        _EXPECTED[key] = (ref, und, triples)
    return _EXPECTED[key]


def _same(a, b):
    """Bit for bit, any NaN standing for any other (0 / 0 has the sign bit set on some machines and not on others)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def check(case, got):
    """got: dict of numpy arrays with any of cnt, num, ratio, dist_out, mean, num_T.  Outside the case's undecided set every count is
    exact; the ratios are the fp64 quotient of the counts bit for bit; dist_out is the fp32 rounding of the fp64 distance; the mean adds the ratios in
    index order; the undecided set is the one the case lists."""
    ref, und, triples = expected(case)
    assert triples == case["listed"], (case["name"], sorted(triples))
    if "num" in got:
        assert np.array_equal(got["num"], ref["num"]), case["name"]
    if "cnt" in got:
        diff = np.abs(got["cnt"].astype(np.int64) - ref["cnt"])
        assert (diff <= und).all(), (case["name"], np.argwhere(diff > und)[:5])
    if "ratio" in got:
        with np.errstate(all="ignore"):
            if "cnt" in got and "num" in got:
                assert _same(got["ratio"], got["cnt"].astype(np.float64) / got["num"].astype(np.float64)[:, :, None]), case["name"]
            assert _same(np.where(und == 0, got["ratio"], 0.0), np.where(und == 0, ref["ratio"], 0.0)), case["name"]
    if "dist_out" in got:
        assert got["dist_out"].dtype == np.float32
        assert _same(got["dist_out"], ref["dist_out"]), case["name"]
    if "mean" in got:
        src = got["ratio"] if "ratio" in got else ref["ratio"]
        assert _same(got["mean"], cr.table_mean(src)), case["name"]
    if "num_T" in got:
        assert np.array_equal(got["num_T"], ref["num"].T), case["name"]
