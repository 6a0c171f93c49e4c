"""fp64 restatement of the least-median-of-squares estimators the tests hold csrc/lmeds.hip and csrc/lmeds_math.h to: OpenCV
3.4's LMeDSPointSetRegistrator::run as include/dfepe.h (dfepe_lmeds_fundamental) specifies it in six steps.  Sampling, the minimal
solvers and the error formulas are those of ransac_ref.py and ransac5_ref.py; new here are the fixed iteration count, the median
of the fp32-rounded errors, the strict-minimum rule, sigma and the inlier bound.  numpy only.

Next to every median the restatement returns a bound on how far a correct device median may lie from it.  The bound is derived
here, not tuned:

  * Order statistics are monotone: when every error e_i moves by at most d_i, the k-th smallest stays between the k-th smallest
    of (e_i - d_i) and the k-th smallest of (e_i + d_i).  So the device's median lies between the medians of those two sets
    (median_bound below; one more fp32 rounding for the sum of the two middle values of an even N).  This is never wider than
    the sup-norm form |median_device - median_ref| <= max_i d_i and much narrower where the largest d_i belongs to an outlier far
    above the median.  The sorted medians of an iteration's roots differ by at most the largest bound among them.
  * The bound of one error q = r^2 / s is a forward bound from the magnitudes of its terms.  With u = 2^-53, r a sum of 9
    products and each line coefficient a sum of 3:  dr = 16 u S + S_m,  S = sum |h2_i| |M_ij| |h1_j|,  S_m the same sum with the
    model uncertainty dM in place of |M|;  da = 4 u sum|terms| + (dM terms), likewise db;  ds = 2|a| da + 2|b| db + da^2 + db^2
    + 4 u s;  and, while ds < s / 2,  dq = ((2 |r| dr + dr^2) / s + q ds / s) / (1 - ds / s) + 4 u q.  max(d1^2, d2^2) is
    1-Lipschitz, so the F error takes the larger dq.  dr^2 / s is the absolute term: at the points of the sample itself r is
    pure rounding noise (1e-28 px^2 at N = 8), and a relative tolerance would mean nothing there.
  * One rounding to fp32 adds 2^-24 (q + dq) + 2^-150.
  * The model uncertainty dM.  Device and restatement solve the same sample by different stable methods (Householder QR and a
    closed-form cubic resp. Nister's elimination there, SVD and an interpolated cubic resp. an action matrix here).  A
    backward-stable solver returns the exact solution of inputs perturbed by c u (relative), c of the order of the operations
    along its longest dependency chain: normalisation (~30), seven reflections over nine rows (~130), the cubic with its Newton
    steps (~40), de-normalisation (~20): c <= 256, also for the longer five-point chain's dominant stages.  The solution's response
    to an input perturbation is measured: the sample is solved again with every coordinate multiplied by 1 + eps xi, eps = 2^-44
    (far above u, so the measurement is not itself rounding noise), xi uniform in [-1, 1]: D = |M' - M|.  A random direction can
    miss the worst one by a factor of a few (8 allowed), and two solvers can be c u away from the exact solution in opposite
    directions (2):  dM = D * 2 * 8 * 256 u / eps = 8 D, plus the floor 2 * 8 * 256 u max|M| = 2^12 u max|M| of a perfectly
    conditioned sample.  Where the second solve has a different number of roots the iteration sits on a double root and is not
    compared.
"""
import math

import numpy as np

import ransac5_ref as ref5
import ransac_ref as ref7

U = 2.0 ** -53
EPS_PROBE = 2.0 ** -44
NO_ROOT, NO_SAMPLE = -1.0, -2.0
DBL_MAX = float(np.finfo(np.float64).max)
OUTLIER_RATIO = 0.45


def num_iters(model_points, confidence, max_iters):
    """Step 1: RANSACUpdateNumIters(confidence, 0.45, m, max_iters), fixed for the whole run."""
    rule = ref7.update_num_iters if model_points == 7 else ref5.update_num_iters
    return rule(confidence, OUTLIER_RATIO, max_iters)


def to_f32(err):
    """Step 3's rounding: fp64 errors -> fp32; anything that is not a finite non-negative number counts as +inf."""
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.asarray(err, np.float64).astype(np.float32)
    e[~(np.isfinite(e) & (e >= 0))] = np.inf
    return e


def f_errors(F, pts):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return ref7.errors(F, np.asarray(pts, np.float32).astype(np.float64))


def e_errors(E, q):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return ref5.sampson(E, q)


def median32(e32):
    """Step 4: OpenCV's median of the sorted fp32 errors (the sum of the two middle values in fp32)."""
    s = np.sort(np.asarray(e32, np.float32))
    n = len(s)
    if n % 2:
        return float(s[n // 2])
    with np.errstate(over="ignore"):
        return float(np.float32(np.float32(s[n // 2 - 1] + s[n // 2]) * np.float32(0.5)))


def select(table, niters):
    """Step 5 over a median table [niters, roots] -> (min_median, best k, best root, iterations the loop went through)."""
    best, bk, br, k = DBL_MAX, -1, -1, 0
    while k < niters:
        if table[k][0] == NO_SAMPLE:
            break
        for r in range(len(table[k])):
            m = float(table[k][r])
            if m >= 0.0 and m < best:
                best, bk, br = m, k, r
        k += 1
    return best, bk, br, k


def sigma_of(min_median, N, model_points):
    """Step 6, in OpenCV's order of operations."""
    return max(2.5 * 1.4826 * (1.0 + 5.0 / (N - model_points)) * math.sqrt(min_median), 0.001)


def bound32(sigma):
    with np.errstate(over="ignore"):
        return np.float32(sigma * sigma)


# ---- the bound ------------------------------------------------------------------------------------------------------------
def _line_terms(M, dM, h, transpose):
    """Coefficients (a, b) of the lines M h (or M^T h) with their uncertainties (da, db)."""
    A, dA = (M.T, dM.T) if transpose else (M, dM)
    ab = h @ A.T[:, :2]
    mag = np.abs(h) @ np.abs(A).T[:, :2]
    dab = 4 * U * mag + np.abs(h) @ dA.T[:, :2]
    return ab, dab


def _quotient_bound(r, dr, s, ds):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q = r * r / s
        dq = ((2 * np.abs(r) * dr + dr * dr) / s + q * ds / s) / (1.0 - ds / s) + 4 * U * q
    dq[~(ds < 0.5 * s)] = np.inf
    return q, dq


def error_bounds(M, dM, x, sampson):
    """Per-correspondence bound of the fp32-rounded error of model M (3x3) with uncertainty dM over x [N,4] (pixels for F,
    normalised coordinates for E)."""
    M, dM, x = np.asarray(M, np.float64).reshape(3, 3), np.asarray(dM, np.float64).reshape(3, 3), np.asarray(x, np.float64)
    h1 = np.c_[x[:, :2], np.ones(len(x))]
    h2 = np.c_[x[:, 2:], np.ones(len(x))]
    r = ((h2 @ M) * h1).sum(1)
    dr = 16 * U * ((np.abs(h2) @ np.abs(M)) * np.abs(h1)).sum(1) + ((np.abs(h2) @ dM) * np.abs(h1)).sum(1)
    ab2, dab2 = _line_terms(M, dM, h1, False)   # M h1: the line in image 2
    ab1, dab1 = _line_terms(M, dM, h2, True)    # M^T h2: the line in image 1
    s2, s1 = (ab2 ** 2).sum(1), (ab1 ** 2).sum(1)
    ds2 = (2 * np.abs(ab2) * dab2 + dab2 ** 2).sum(1) + 4 * U * s2
    ds1 = (2 * np.abs(ab1) * dab1 + dab1 ** 2).sum(1) + 4 * U * s1
    if sampson:
        q, dq = _quotient_bound(r, dr, s1 + s2, ds1 + ds2)
    else:
        q2, dq2 = _quotient_bound(r, dr, s2, ds2)
        q1, dq1 = _quotient_bound(r, dr, s1, ds1)
        q, dq = np.fmax(q1, q2), np.fmax(dq1, dq2)
    with np.errstate(invalid="ignore", over="ignore"):
        out = dq + 2.0 ** -24 * (q + dq) + 2.0 ** -150
    out[~np.isfinite(out)] = np.inf
    return out


def median_bound(e, d):
    """(median, bound) of the fp32-rounded errors e (fp64 [N]) whose device values lie within d of them."""
    e = np.asarray(e, np.float64)
    e = np.where(np.isfinite(e) & (e >= 0), e, np.inf)
    d = np.where(np.isfinite(d), d, np.inf)
    med = median32(to_f32(e))
    with np.errstate(invalid="ignore"):
        lo = np.where(np.isfinite(d), np.maximum(e - d, 0.0), 0.0)
        hi = np.where(np.isfinite(e), e + d, np.inf)
    m_lo, m_hi = median32(to_f32(lo)), median32(to_f32(hi))
    if not np.isfinite(m_hi):
        return med, (0.0 if not np.isfinite(med) and not np.isfinite(m_lo) else np.inf)
    return med, max(m_hi - med, med - m_lo) + 2.0 ** -24 * m_hi + 2.0 ** -149


def _probe(k, shape):
    return 1.0 + EPS_PROBE * np.random.default_rng(1000003 + k).uniform(-1.0, 1.0, shape)


def _uncertainty(M, M2):
    M = np.asarray(M, np.float64)
    return 8.0 * np.abs(np.asarray(M2, np.float64) - M) + 2.0 ** 12 * U * np.abs(M).max()


def models_f(pts, seed, niters):
    """Per iteration: None (no sample) or a list of (F, dF | None); dF None: the probe solve has another number of roots."""
    pts = np.asarray(pts, np.float32)
    out = []
    for k in range(niters):
        idx = ref7.draw_sample(seed, k, pts)
        if idx is None:
            out.append(None)
            continue
        p7 = pts[idx].astype(np.float64)
        Fs, Fp = ref7.seven_point(p7), ref7.seven_point(p7 * _probe(k, p7.shape))
        same = len(Fs) == len(Fp)
        out.append([(F, _uncertainty(F, Fp[i]) if same else None) for i, F in enumerate(Fs)])
    return out


def models_e(q, seed, niters):
    """The same for five-point models on normalised coordinates q [N,4]; the probe's roots are matched to the nearest."""
    out = []
    for k in range(niters):
        q5 = q[ref5.draw_sample(seed, k, len(q))]
        Es, Ep = ref5.five_point(q5), ref5.five_point(q5 * _probe(k, q5.shape))
        same = len(Es) == len(Ep)
        row = []
        for E in Es:
            dE = None
            if same:
                j = int(np.argmin([np.abs(G - E).max() for G in Ep]))
                dE = _uncertainty(E, Ep[j])
            row.append((E, dE))
        out.append(row)
    return out


def median_table(models, x, roots, sampson):
    """Median table [niters, roots] of the restatement and the bound of every entry (inf: not comparable)."""
    n = len(models)
    med = np.full((n, roots), NO_ROOT)
    bnd = np.zeros((n, roots))
    for k, row in enumerate(models):
        if row is None:
            med[k] = NO_SAMPLE
            continue
        for r, (M, dM) in enumerate(row):
            e = e_errors(M, x) if sampson else f_errors(M, x)
            if dM is None:
                med[k, r], bnd[k, r] = median32(to_f32(e)), np.inf
            else:
                med[k, r], bnd[k, r] = median_bound(e, error_bounds(M, dM, x, sampson))
    return med, bnd


def is_ambiguous(med, bnd, niters):
    """True when, among the entries the rule reads, a second median lies within the summed bounds of the minimum (or the minimum
    itself is not comparable): the winner is then the implementation's."""
    best, bk, br, it = select(med, niters)
    if bk < 0:
        return False
    if not np.isfinite(bnd[bk, br]):
        return True
    for k in range(it):
        for r in range(med.shape[1]):
            if (k, r) != (bk, br) and med[k, r] >= 0 and med[k, r] - best <= bnd[k, r] + bnd[bk, br]:
                return True
    return False
