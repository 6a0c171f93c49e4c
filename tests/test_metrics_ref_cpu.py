"""The numpy restatement of the validation summary (tests/metrics_ref.py) and its case table (tests/metrics_cases.py) are themselves
right: against brute-force Python loops over every case, against oracle.metrics_summary_np on ordinary data, and on the inputs of
tests/golden/metrics.npz (what the reference project's own write_metrics_summary logged).  Also pins which median the contract is:
the float64 mean of the two middle float32 values, which np.median of the float32 array rounds away.  Runs without a GPU."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_cases as cs  # noqa: E402
import metrics_ref as ref  # noqa: E402


def same(a, b):
    """== for floats, with NaN equal to NaN."""
    return (a == b) or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def loops_err_stats(x):
    """bin counts, maximum, median by Python loops over Python floats (a float32 widens to a Python float exactly)."""
    v = [float(a) for a in x]
    th = cs.METRIC_THS
    hist = [0] * 12
    for a in v:
        for k in range(12):
            if th[k] <= a and (a < th[k + 1] or (k == 11 and a == th[12])):
                hist[k] += 1
    if any(math.isnan(a) for a in v):
        return hist, math.nan, math.nan
    mx = v[0]
    for a in v:
        if a > mx:
            mx = a
    s = sorted(v)
    n = len(s)
    return hist, mx, 0.5 * (s[(n - 1) // 2] + s[n // 2])


def loops_epi_counts(est, gt):
    t01, t1 = float(np.float32(0.1)), 1.0
    c = [0] * 8
    for i in range(len(est)):
        e = float(est[i])
        c[0] += e < t01
        c[1] += e < t1
        if gt is not None:
            g = float(gt[i])
            for base, t in ((2, t01), (5, t1)):
                c[base] += (g < t) and (e < t)
                c[base + 1] += (not g < t) and (e < t)
                c[base + 2] += (g < t) and (not e < t)
    return c


def all_err_pairs():
    for fam in cs.ERR_FAMILIES:
        for B in cs.ERR_B:
            yield f"{fam}[{B}]", cs.err_vector(fam, B, 0), cs.err_vector(fam, B, 1)
    for name, (q, t) in cs.special_err_cases().items():
        yield name, q, t


def test_err_stats_against_loops():
    for name, q, t in all_err_pairs():
        for x in (q, t):
            hist, mx, med = ref.err_stats(x)
            lh, lmx, lmed = loops_err_stats(x)
            assert hist.tolist() == lh, name
            assert same(mx, lmx), (name, mx, lmx)
            assert same(med, lmed), (name, med, lmed)
    assert ref.err_stats(np.zeros(0, np.float32))[1:] == (0.0, 0.0)


def test_the_case_table_is_what_it_says():
    for B in cs.ERR_B:
        x = np.sort(cs.err_vector("two_values", B))
        if B > 1:
            assert len(np.unique(x)) == 2 and (x == x[0]).sum() == B // 2
        if B % 2 == 0:
            lo, hi = x[B // 2 - 1], x[B // 2]
            assert hi == np.nextafter(lo, np.float32(np.inf))
            med = ref.err_stats(x)[2]
            # THE contract: the float64 mean of two neighbouring float32 values is no float32; np.median of the float32 array rounds it
            assert float(lo) < med < float(hi) and float(np.median(x)) != med and np.float32(med) in (lo, hi)
        x = np.sort(cs.err_vector("tie_block", B))
        if B >= 3:
            assert x[(B - 1) // 2] == x[B // 2] and (x == x[B // 2]).sum() >= max(B // 2, 2) - 1
            assert x[B // 4] == x[B // 2] and (B < 8 or x[B // 4 - 1] < x[B // 2] < x[3 * B // 4])
        assert len(np.unique(cs.err_vector("all_equal", B))) == 1
        assert (np.diff(cs.err_vector("ascending", B)) >= 0).all() and (np.diff(cs.err_vector("descending", B)) <= 0).all()
        assert not np.array_equal(cs.err_vector("random", B, 0), cs.err_vector("random", B, 1))
    ev = cs.edge_values()
    assert len(ev) == 46 and np.isinf(ev).sum() == 1 and np.signbit(ev).sum() >= 4 and np.float32(180.0) in ev
    assert np.nextafter(np.float32(180.0), np.float32(np.inf)) in ev
    # the rounded edges fall on both sides of the float64 edges: np.histogram in float64 is not np.histogram in float32
    below = [float(np.float32(t)) < t for t in cs.METRIC_THS]
    above = [float(np.float32(t)) > t for t in cs.METRIC_THS]
    assert any(below) and any(above)
    h64 = ref.err_stats(ev)[0]
    h32 = np.histogram(ev[np.isfinite(ev)], bins=np.array(cs.METRIC_THS, np.float32))[0]
    assert h64.sum() == h32.sum() and h64.tolist() != h32.tolist()
    # numpy drops NaN and values outside [0, 180] by itself
    with np.errstate(invalid="ignore"):
        h = np.histogram(np.array([np.nan, 1.0, -1.0, 181.0, np.inf, 180.0]), bins=np.array(cs.METRIC_THS))[0]
    assert h.tolist() == [0] * 7 + [1, 0, 0, 0, 1]
    sp = cs.special_err_cases()
    assert np.signbit(sp["all_negzero"][0]).all() and ref.err_stats(sp["all_negzero"][0])[1] == 0.0
    assert ref.err_stats(sp["negzero_with_positives"][0])[1] == 2.0 and math.isnan(ref.err_stats(sp["negzero_with_nan"][0])[1])
    assert np.isnan(sp["nan_in_last_partial_block"][0]).nonzero()[0].tolist() == [256] and not np.isnan(sp["nan_in_last_partial_block"][1]).any()
    # every error vector of the table has an entry that is >= 0 or NaN: np.amax and the kernel's maximum over max(x, +0) agree
    for name, q, t in all_err_pairs():
        for x in (q, t):
            assert ((x >= 0) | np.isnan(x)).any(), name


@pytest.mark.parametrize("n", [n for n in cs.EPI_N if n <= 2049])
def test_epi_counts_against_loops(n):
    est, gt = cs.epi_vectors(n)
    assert ref.epi_counts(est, gt) == loops_epi_counts(est, gt)
    assert ref.epi_counts(est, None) == loops_epi_counts(est, None)
    if n >= 2047:
        c = ref.epi_counts(est, gt)
        assert min(c) > 0 and np.isnan(est).sum() >= 15 and np.isinf(gt).sum() >= 15
        sp = cs.epi_specials()
        assert (est[:, None] == sp[None, :6]).any(0).all()  # each threshold and both neighbours are there


def test_epi_vectors_at_the_grid_edge_are_what_they_say():
    for n in cs.EPI_N[-2:]:
        est, gt = cs.epi_vectors(n)
        assert est.shape == gt.shape == (n,) and est.dtype == np.float32 and est.nbytes <= 8 * 1024 * 1024 + 4
        c = ref.epi_counts(est, gt)
        assert 0.2 * n < c[0] < 0.6 * n < c[1] < 0.8 * n and min(c) > 1000
        # the tail element alone: est == float32(0.1) is not below it, gt just is
        assert ref.epi_counts(est[-1:], gt[-1:]) == [0, 1, 0, 0, 1, 1, 0, 0]
    assert ref.summary(np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.float32))["F1_1"] == 0.0
    assert ref.f1(0, 0, 0) == 0.0 and ref.f1(1, 0, 0) == 1.0 and ref.f1(1, 1, 1) == 0.5


def test_summary_against_the_oracle_on_ordinary_data(oracle):
    g = np.random.default_rng(1)
    for B, n in ((64, 6400), (257, 1000), (5, 50)):
        est = g.gamma(1.0, 0.5, n).astype(np.float32)
        gt = g.gamma(1.0, 0.3, n).astype(np.float32)
        q, t = g.gamma(1.0, 2.0, B).astype(np.float32), g.uniform(0, 180, B).astype(np.float32)
        mine, theirs = ref.summary(est, gt, q, t), oracle.metrics_summary_np(est, gt, q, t)
        for k, v in theirs.items():
            if k.startswith("median"):  # the oracle's np.median of the float32 array rounds the mean to float32
                assert np.float32(mine[k]) == np.float32(v) or abs(mine[k] - v) <= np.spacing(np.float32(v)), k
            elif k.startswith("ratio_q") or k.startswith("ratio_t"):  # the oracle sums hist / B, the summary divides the summed counts
                assert [round(x * B) for x in mine[k]] == [round(x * B) for x in v] and np.abs(np.array(mine[k]) - np.array(v)).max() <= 2.0 ** -50, k
            else:
                assert mine[k] == v, k


def test_summary_on_the_golden_inputs(golden):
    """tests/golden/metrics.npz: the inputs in float32 (what the kernel is given) against the scalars the reference logged from them in
    float64.  Maxima and medians agree to the float32 rounding of an input; a count moves only where that rounding crosses a threshold,
    which on these inputs it does for no element."""
    g = golden("metrics")
    want = dict(zip([str(t) for t in g["tags"]], g["values"]))
    d = {}
    for k in g.files:
        if k.startswith("in_"):
            metric, tag = k[3:].rsplit("_", 1)
            d.setdefault(metric, {})[tag] = np.stack([a for a in g[k]])
    gt = d["epi_dists"]["gt"].reshape(-1)
    for tag in d["epi_dists"]:
        est, q, t = d["epi_dists"][tag].reshape(-1), d["err_q"][tag].reshape(-1), d["err_t"][tag].reshape(-1)
        for x, ths in ((est, (0.1, 1.0)), (gt, (0.1, 1.0)), (q, cs.METRIC_THS), (t, cs.METRIC_THS)):
            x32 = x.astype(np.float32).astype(np.float64)
            for th in ths:
                th = float(np.float32(th)) if ths == (0.1, 1.0) else th
                assert ((x < th) == (x32 < th)).all()
        sm = ref.summary(est.astype(np.float32), gt.astype(np.float32), q.astype(np.float32), t.astype(np.float32))
        assert abs(sm["ratio_0.1"] - want[f"val-Error-epi_dists/{tag}-0.1"]) < 1e-12 and abs(sm["ratio_1"] - want[f"val-Error-epi_dists/{tag}-1"]) < 1e-12
        assert abs(sm["F1_0.1"] - want[f"val-Error-F1/{tag}-0.1"]) < 1e-12 and abs(sm["F1_1"] - want[f"val-Error-F1/{tag}-1"]) < 1e-12
        for k, th in enumerate(cs.METRIC_THS[1:]):
            assert abs(sm["ratio_q"][k] - want[f"val-Error-ratio/ratio_q{th}_{tag}"]) < 1e-12
            assert abs(sm["ratio_t"][k] - want[f"val-Error-ratio/ratio_t{th}_{tag}"]) < 1e-12
        for mine, key in ((sm["median_err_q"], f"val-Error-Median/err_q-{tag}"), (sm["median_err_t"], f"val-Error-Median/err_t-{tag}"),
                          (sm["max_err_q"], f"val-Error-MAX/err_q_MAX_{tag}")):
            assert abs(mine - want[key]) <= 2.0 ** -24 * abs(want[key]), key
