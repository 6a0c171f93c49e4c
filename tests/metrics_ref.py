"""Plain numpy restatement of the validation summary (ops.metrics_summary / dfepe_metrics_summary, csrc/metrics.hip: epi_counts_kernel
and err_stats_kernel; the reference project's write_metrics_summary, train_good_utils.py:758-856) on the float32 inputs as they are
given.  No sklearn, no GPU, nothing of the product.  Every quantity is an integer count, one of the input values, or the float64 mean
of two of them, so tests/test_metrics_edges_gpu.py compares with == and no tolerance.

The contracts this pins:
  epipolar counts   x < float32(0.1) and x < 1.0f, compared in float32 (a float32 numpy array against a Python scalar does that);
                    NaN is below nothing
  histogram         np.histogram of the values widened to float64 against the float64 edges METRIC_THS: bins [a, b), the last one
                    [10... 90, 180] closed; values outside [0, 180] and NaN are dropped; ratios are cumsum / B
  maximum           np.amax: NaN if any entry is NaN.  The kernel takes the maximum over the entries that are > 0 or NaN, starting
                    from +0.0: the same number whenever one entry is >= 0 or NaN (angles are), and 0.0 == -0.0 for zeros of either sign
  median            np.median of the values WIDENED TO FLOAT64: the float64 mean of the two middle float32 order statistics, not
                    rounded back to float32 (np.median of the float32 array would round); NaN if any entry is NaN
  empty inputs      B = 0: median, maximum 0.0 and all ratios 0.0; n_epi = 0: ratios 0.0, F1 0.0 (None without epi_gt)"""
import numpy as np

METRIC_THS = (0.0, 0.01, 0.03, 0.05, 0.1, 0.3, 0.5, 1.0, 2.0, 5.0, 10.0, 90.0, 180.0)
TH_01, TH_1 = np.float32(0.1), np.float32(1.0)


def _f32(x):
    a = np.asarray(x)
    assert a.dtype == np.float32, "the reference takes the float32 values the kernel is given"
    return a.reshape(-1)


def epi_counts(epi_est, epi_gt=None):
    """The eight integers of epi_counts_kernel: est < 0.1, est < 1, then TP, FP, FN at 0.1 and at 1.0 (zeros without epi_gt)."""
    e = _f32(epi_est)
    e01, e1 = e < TH_01, e < TH_1
    c = [int(e01.sum()), int(e1.sum()), 0, 0, 0, 0, 0, 0]
    if epi_gt is not None:
        g = _f32(epi_gt)
        assert g.shape == e.shape
        g01, g1 = g < TH_01, g < TH_1
        c[2:] = [int((g01 & e01).sum()), int((~g01 & e01).sum()), int((g01 & ~e01).sum()),
                 int((g1 & e1).sum()), int((~g1 & e1).sum()), int((g1 & ~e1).sum())]
    return c


def f1(tp, fp, fn):
    """sklearn's binary F1 = 2 TP / (2 TP + FP + FN), 0.0 when nothing is positive anywhere."""
    tp, fp, fn = float(tp), float(fp), float(fn)
    return float(2 * tp / (2 * tp + fp + fn)) if (2 * tp + fp + fn) > 0 else 0.0


def err_stats(err):
    """(bin counts [12] int, maximum, median) of one error vector; zeros for an empty one."""
    x = _f32(err)
    if x.size == 0:
        return np.zeros(len(METRIC_THS) - 1, np.int64), 0.0, 0.0
    x64 = x.astype(np.float64)
    hist = np.histogram(x64[~np.isnan(x64)], bins=np.array(METRIC_THS))[0].astype(np.int64)  # numpy drops NaN itself; said here
    with np.errstate(invalid="ignore"):
        return hist, float(np.amax(x)), float(np.median(x64))


def summary(epi_est, epi_gt, err_q, err_t):
    """The dict of ops.metrics_summary, plus the raw integers under "counts", "hist_q", "hist_t"."""
    e = _f32(epi_est)
    c = epi_counts(e, epi_gt)
    n, B = max(e.size, 1), max(_f32(err_q).size, 1)
    assert _f32(err_q).size == _f32(err_t).size
    hq, mq, medq = err_stats(err_q)
    ht, mt, medt = err_stats(err_t)
    return {"ratio_0.1": c[0] / n, "ratio_1": c[1] / n,
            "F1_0.1": f1(*c[2:5]) if epi_gt is not None else None, "F1_1": f1(*c[5:8]) if epi_gt is not None else None,
            "median_err_q": medq, "median_err_t": medt, "max_err_q": mq, "max_err_t": mt,
            "ratio_q": (np.cumsum(hq.astype(np.float64)) / B).tolist(), "ratio_t": (np.cumsum(ht.astype(np.float64)) / B).tolist(),
            "counts": c, "hist_q": hq.tolist(), "hist_t": ht.tolist()}
