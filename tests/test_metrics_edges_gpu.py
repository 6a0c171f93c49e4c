"""ops.metrics_summary on the device (csrc/metrics.hip: epi_counts_kernel, err_stats_kernel) against the numpy restatement of
tests/metrics_ref.py over the case table of tests/metrics_cases.py.  Everything is compared exactly: every quantity is an integer
count (read back from its ratio as count / n), one of the input values, or the float64 mean of two of them.  No tolerance anywhere."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_cases as cs  # noqa: E402
import metrics_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL_EPI = 2049


def dev(x):
    return None if x is None else torch.as_tensor(np.array(x, order="C"), device=DEV)  # a copy: the table's arrays are read-only


def same(a, b):
    return a == b or (a is not None and b is not None and math.isnan(a) and math.isnan(b))


def compare(got, want, n_epi, B, tag):
    """got = ops.metrics_summary's dict, want = metrics_ref.summary's: integers as integers, floats with == (NaN equals NaN)."""
    n, Bd = max(n_epi, 1), max(B, 1)
    print(f"METRICS {tag}: counts {want['counts']} median {got['median_err_q']!r} {got['median_err_t']!r} max {got['max_err_q']!r} {got['max_err_t']!r}")
    assert round(got["ratio_0.1"] * n) == want["counts"][0] and round(got["ratio_1"] * n) == want["counts"][1], tag
    for key in ("ratio_0.1", "ratio_1", "F1_0.1", "F1_1"):
        assert same(got[key], want[key]), (tag, key, got[key], want[key])
    for key, hist in (("ratio_q", "hist_q"), ("ratio_t", "hist_t")):
        counts = np.diff(np.concatenate(([0.0], np.asarray(got[key]) * Bd)))
        assert [round(c) for c in counts] == want[hist], (tag, key, counts, want[hist])
        assert got[key] == want[key], (tag, key)
    for key in ("median_err_q", "median_err_t", "max_err_q", "max_err_t"):
        assert isinstance(got[key], float) and same(got[key], want[key]), (tag, key, got[key], want[key])


def run(dfepe, est, gt, q, t, tag):
    got = dfepe.ops.metrics_summary(dev(est), dev(gt), dev(q), dev(t))
    compare(got, ref.summary(est, gt, q, t), est.size, q.size, tag)
    return got


@pytest.mark.parametrize("B", cs.ERR_B)
def test_err_stats_at_every_block_edge(dfepe, B):
    """B on either side of one and two workgroups; random, constant, two-valued, tied-across-the-middle and sorted vectors: the bin
    counts, the maximum, and the median as the float64 mean of the two middle float32 order statistics."""
    est, gt = cs.epi_vectors(SMALL_EPI)
    for fam in cs.ERR_FAMILIES:
        q, t = cs.err_vector(fam, B, 0), cs.err_vector(fam, B, 1)
        got = run(dfepe, est, gt, q, t, f"{fam}[{B}]")
        if fam == "two_values" and B % 2 == 0:
            s = np.sort(q)
            assert float(s[B // 2 - 1]) < got["median_err_q"] < float(s[B // 2])  # between two neighbouring float32: not a float32
        # err_q and err_t are handled independently: swapped, the results swap
        sw = dfepe.ops.metrics_summary(dev(est), dev(gt), dev(t), dev(q))
        for a, b in (("median_err_q", "median_err_t"), ("max_err_q", "max_err_t"), ("ratio_q", "ratio_t")):
            assert sw[a] == got[b] and sw[b] == got[a], (fam, B, a)


@pytest.mark.parametrize("name", list(cs.special_err_cases()))
def test_err_stats_special_values(dfepe, name):
    """Histogram edges and their float32 neighbours, values outside [0, 180], +inf; a NaN alone, in the last partial workgroup, in one
    vector only; -0.0 next to positive values, next to a NaN, next to +inf, alone (csrc/metrics.hip: the maximum is an atomicMax over
    bit patterns, and the pattern of -0.0 is the largest there is)."""
    q, t = cs.special_err_cases()[name]
    est, gt = cs.epi_vectors(SMALL_EPI)
    got = run(dfepe, est, gt, q, t, name)
    if name == "negzero_with_positives":
        assert got["max_err_q"] == 2.0 and got["max_err_t"] == 0.25
    if name == "negzero_with_nan":
        assert math.isnan(got["max_err_q"]) and math.isnan(got["max_err_t"]) and math.isnan(got["median_err_q"])
    if name == "negzero_with_inf":
        assert got["max_err_q"] == math.inf and got["max_err_t"] == float(np.float32(1e-45))
    if name in ("all_negzero", "zeros_of_both_signs"):
        assert got["max_err_q"] == 0.0 and got["median_err_q"] == 0.0 and got["ratio_q"] == [1.0] * 12
    if name == "nan_in_err_t_only":
        assert math.isfinite(got["median_err_q"]) and math.isfinite(got["max_err_q"]) and math.isnan(got["median_err_t"]) and math.isnan(got["max_err_t"])
        assert got["ratio_t"][-1] == 256 / 257 and got["ratio_q"][-1] == 1.0  # np.histogram drops the NaN
    if name == "nan_only_element":
        assert math.isnan(got["median_err_q"]) and math.isnan(got["max_err_q"]) and got["ratio_q"] == [0.0] * 12 and got["median_err_t"] == 1.5


def test_empty_error_vectors_give_the_zeroed_record(dfepe):
    est, gt = cs.epi_vectors(SMALL_EPI)
    e = np.zeros(0, np.float32)
    got = run(dfepe, est, gt, e, e, "B = 0")
    assert got["median_err_q"] == 0.0 and got["max_err_t"] == 0.0 and got["ratio_q"] == [0.0] * 12 and got["ratio_t"] == [0.0] * 12
    got = run(dfepe, e, e, e, e, "nothing at all")
    assert got["ratio_0.1"] == 0.0 and got["F1_1"] == 0.0
    assert dfepe.ops.metrics_summary(dev(e), None, dev(e), dev(e))["F1_0.1"] is None


@pytest.mark.parametrize("with_gt", [True, False])
@pytest.mark.parametrize("n", cs.EPI_N)
def test_epi_counts_at_every_grid_edge(dfepe, n, with_gt):
    """n_epi = 0 (what write_metrics_summary passes for a tag without distances), one element, either side of one workgroup's 2048, the
    largest grid exactly full and one element more (another trip of the grid-stride loop); thresholds, their neighbours, NaN,
    infinities and negatives in both vectors; the tail element counted once."""
    est, gt = cs.epi_vectors(n)
    q, t = cs.err_vector("random", 64, 0), cs.err_vector("tie_block", 64, 1)
    got = run(dfepe, est, gt if with_gt else None, q, t, f"n_epi = {n}, gt {with_gt}")
    if not with_gt:
        assert got["F1_0.1"] is None and got["F1_1"] is None
    elif n:
        assert 0.0 < got["F1_0.1"] < 1.0 or n == 1


def test_f1_with_nothing_positive_and_strided_inputs(dfepe):
    q, t = cs.err_vector("random", 3, 0), cs.err_vector("random", 3, 1)
    # nothing below 1.0 in either vector: TP = FP = FN = 0 and F1 = 0.0, not 0 / 0
    far = np.linspace(1.0, 50.0, 300, dtype=np.float32)
    got = run(dfepe, far, far[::-1].copy(), q, t, "no positives")
    assert got["F1_0.1"] == 0.0 and got["F1_1"] == 0.0 and got["ratio_1"] == 0.0
    # all positive and all agreeing: F1 = 1
    near = np.full(300, 0.05, np.float32)
    assert run(dfepe, near, near, q, t, "all positives")["F1_0.1"] == 1.0
    # a 2-D, non-contiguous view: every other column of [64, 80]
    est, gt = cs.epi_vectors(64 * 80)
    wide_e, wide_g = dev(est.reshape(64, 80)), dev(gt.reshape(64, 80))
    ve, vg = wide_e[:, ::2], wide_g[:, ::2]
    assert not ve.is_contiguous() and ve.shape == (64, 40)
    got = dfepe.ops.metrics_summary(ve, vg, dev(q), dev(t))
    compare(got, ref.summary(est.reshape(64, 80)[:, ::2].copy(), gt.reshape(64, 80)[:, ::2].copy(), q, t), 64 * 40, 3, "strided")
    assert np.array_equal(wide_e.cpu().numpy().reshape(-1), est, equal_nan=True)  # the input is left alone


def test_ten_runs_give_the_same_bytes(dfepe):
    """Integer atomics only: the 288-byte record of one mixed case (ties, a partial workgroup, 513 errors, 20000 distances) is the same
    ten times over, straight from the C entry point on one stream."""
    L = dfepe._lib.lib()
    est, gt = (dev(x) for x in cs.epi_vectors(20000))
    q, t = dev(cs.err_vector("tie_block", 513, 0)), dev(cs.err_vector("random", 513, 1))
    nbytes = int(L.dfepe_metrics_summary_bytes())
    assert nbytes == 288  # 8 counts, 2 x 12 bins, 2 maxima, 2 x 2 order statistics, 8 bytes of padding
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    records = []
    for _ in range(10):
        out = torch.full((nbytes // 8 + 2,), -1, dtype=torch.int64, device=DEV)  # one word of sentinel behind the record
        assert L.dfepe_metrics_summary(est.data_ptr(), gt.data_ptr(), est.numel(), q.data_ptr(), t.data_ptr(), 513, out.data_ptr(), st) == 0
        records.append(out)
    torch.cuda.synchronize()
    raw = [r.cpu().numpy().tobytes() for r in records]
    assert all(r == raw[0] for r in raw)
    assert raw[0][nbytes:] == b"\xff" * 16
    want = ref.summary(*cs.epi_vectors(20000), cs.err_vector("tie_block", 513, 0), cs.err_vector("random", 513, 1))
    assert np.frombuffer(raw[0], np.uint64, 8).tolist() == want["counts"]
    assert np.frombuffer(raw[0], np.uint64, 24, 64).tolist() == want["hist_q"] + want["hist_t"]
    assert np.frombuffer(raw[0], np.float32, 2, 256).tolist() == [want["max_err_q"], want["max_err_t"]]
