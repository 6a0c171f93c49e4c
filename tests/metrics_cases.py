"""Case table of the validation summary (ops.metrics_summary; csrc/metrics.hip: epi_counts_kernel, err_stats_kernel), shared by
tests/test_metrics_ref_cpu.py and tests/test_metrics_edges_gpu.py.  Deterministic (numpy.random.default_rng(SEED + offset)), float32
throughout.  err_stats_kernel runs 256 lanes per workgroup and counts ranks over the whole vector, so B straddles 256 and 512;
epi_counts_kernel runs min(ceil(n / 2048), 1024) workgroups of 256 lanes and strides by the grid: up to 8 trips per lane below
1024 * 2048 elements, a ninth from 1024 * 2048 + 1 on, where the grid no longer grows."""
import functools

import numpy as np

SEED = 9300
ERR_B = (1, 2, 3, 64, 255, 256, 257, 513)
ERR_FAMILIES = ("random", "all_equal", "two_values", "tie_block", "ascending", "descending")
EPI_N = (0, 1, 2047, 2048, 2049, 1024 * 2048, 1024 * 2048 + 1)
METRIC_THS = (0.0, 0.01, 0.03, 0.05, 0.1, 0.3, 0.5, 1.0, 2.0, 5.0, 10.0, 90.0, 180.0)
F32 = np.float32


def _rng(k):
    return np.random.default_rng(SEED + k)


@functools.lru_cache(maxsize=None)
def err_vector(family, B, which=0):
    """One float32 error vector of length B in [0, 180] (which = 0 / 1: two different draws, for err_q and err_t)."""
    g = _rng(1000 * ERR_FAMILIES.index(family) + 10 * B + which)
    if family == "random":
        x = g.uniform(0.0, 180.0, B)
    elif family == "all_equal":
        x = np.full(B, g.uniform(0.0, 180.0))
    elif family == "two_values":
        # half and half, shuffled: at even B the two middle order statistics differ, and their float64 mean is no float32
        lo = F32(g.uniform(0.0, 90.0))
        x = np.where(np.arange(B) < B // 2, lo, np.nextafter(lo, F32(np.inf)))
        x = g.permutation(x)
    elif family == "tie_block":
        # a block of equal values over the ranks B/4 .. 3B/4 (both middle ranks inside it), distinct values on either side, shuffled
        x = np.sort(g.uniform(0.0, 180.0, B))
        x[B // 4:max(3 * B // 4, B // 4 + 1)] = x[B // 2]
        x = g.permutation(x)
    elif family == "ascending":
        x = np.sort(g.uniform(0.0, 180.0, B))
    else:
        x = np.sort(g.uniform(0.0, 180.0, B))[::-1]
    x = np.ascontiguousarray(x, dtype=F32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def edge_values():
    """Every histogram edge as float32 with its float32 neighbours on both sides; 0, 180 and the float32 above 180; small negatives
    and -0.0; +inf: 46 values.  float32(0.01) < 0.01 < float32(0.03) ...: which side of the float64 edge a rounded edge falls on differs
    from edge to edge, and np.histogram decides in float64."""
    v = []
    for th in METRIC_THS:
        t = F32(th)
        v += [np.nextafter(t, F32(-np.inf)), t, np.nextafter(t, F32(np.inf))]
    v += [F32(-0.0), F32(-1e-6), F32(-1e-30), F32(-1e-45), F32(1e-45), F32(np.inf), F32(179.99998)]
    x = np.array(v, dtype=F32)
    x.setflags(write=False)
    return x


def special_err_cases():
    """name -> (err_q, err_t): NaN placements (err_q and err_t are handled independently) and the -0.0 cases of the maximum."""
    nan, nz = F32(np.nan), F32(-0.0)
    r257, s257 = err_vector("random", 257, 0), err_vector("random", 257, 1)
    with_nan = r257.copy()
    with_nan[256] = nan  # the one live lane of the last workgroup
    ev = edge_values()
    return {
        "edges": (ev, ev[::-1].copy()),
        "nan_only_element": (np.array([nan], F32), np.array([1.5], F32)),
        "nan_in_last_partial_block": (with_nan, s257),
        "nan_in_err_t_only": (r257, np.concatenate((s257[:100], [nan], s257[101:])).astype(F32)),
        "nan_in_both": (with_nan, with_nan[::-1].copy()),
        "negzero_with_positives": (np.array([nz, 1.0, 2.0, 0.5], F32), np.array([0.25, nz, nz, 0.125], F32)),
        "negzero_with_nan": (np.array([nz, nan, 3.0], F32), np.array([nan, nz, nz], F32)),
        "negzero_with_inf": (np.array([nz, np.inf, 3.0], F32), np.array([nz, 1e-45, nz], F32)),
        "all_negzero": (np.full(5, nz, F32), np.full(5, nz, F32)),
        "negzero_at_block_edges": (np.concatenate((r257[:255], [nz, nz])).astype(F32), np.concatenate(([nz], s257[1:])).astype(F32)),
        "zeros_of_both_signs": (np.array([nz, 0.0, nz, 0.0], F32), np.array([0.0, nz, 0.0, nz], F32)),
    }


def epi_specials():
    """The thresholds float32(0.1) and 1.0f with their neighbours, zeros, negatives, NaN, infinities."""
    t01, t1 = F32(0.1), F32(1.0)
    up, dn = F32(np.inf), F32(-np.inf)
    return np.array([np.nextafter(t01, dn), t01, np.nextafter(t01, up), np.nextafter(t1, dn), t1, np.nextafter(t1, up), 0.0, -0.0, -1.0, -1e-30,
                     np.nan, np.inf, -np.inf, 1e-45, 3e38], dtype=F32)


@functools.lru_cache(maxsize=None)
def epi_vectors(n):
    """(est, gt) float32 [n]: log-uniform in [1e-3, 30] (about a third below 0.1, a third above 1), the specials scattered through est
    and gt at different places (so that every TP / FP / FN combination of them occurs), the last element of both a special."""
    g = _rng(50000 + n % 9973)
    est = (10.0 ** g.uniform(-3.0, 1.5, n)).astype(F32)
    gt = (est * (10.0 ** g.uniform(-0.7, 0.7, n))).astype(F32)
    sp = epi_specials()
    if n >= 2 * len(sp) * len(sp):
        pos = g.choice(n - 1, size=len(sp) * len(sp), replace=False)
        est[pos] = np.repeat(sp, len(sp))
        gt[pos] = np.tile(sp, len(sp))
    if n:
        est[-1], gt[-1] = F32(0.1), np.nextafter(F32(0.1), F32(-np.inf))  # the tail element: FN at 0.1, TP at 1.0
    for x in (est, gt):
        x.setflags(write=False)
    return est, gt
