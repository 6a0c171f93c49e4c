"""fp64 restatement of the correspondence evaluation the tests hold csrc/corr_eval.hip and csrc/corr_eval_math.h to: the distance
dist3 of epi_distance_np (deepFEPE/dsac_tools/utils_F.py:363-385) and Result_processor's table (deepFEPE/utils/eval_tools.py:
inlier_ratio :70-104, get_mask :145-147, inlier_ratio_from_est :164-174) as include/dfepe.h specifies them.  numpy only, written
from the specification: the distance is evaluated on whole arrays with the associations the header spells out, the masks and the
counts are numpy's boolean sums, the mean adds the pairs in index order.  A 50-digit mpmath twin covers the distance.

The bound (u = 2^-53; on |an fp64 evaluation of dist3 - the exact value|, for ANY order of the three-term sums and with or without
fused multiply-adds, so it also covers numpy's BLAS products in the reference; two evaluations differ by at most twice the bound)
----------------------------------------------------------------------------------------------------------------------------------
numerator   a_j = x2 F0j + y2 F1j + F2j is two products and two sums, |da_j| <= 3u A_j with A_j = |x2 F0j| + |y2 F1j| + |F2j|;
            nominator = |a0 x1 + a1 y1 + a2| adds two products and two sums on top: |dnom| <= 6u S, S = A0 |x1| + A1 |y1| + A2
            (first order; SLACK = 1 + 2^-20 on the final bound covers the second-order terms).
norms       p_i = Fi0 x1 + Fi1 y1 + Fi2: |dp_i| <= 3u P_i, P_i the sum of the absolute terms.  n = sqrt(p0^2 + p1^2): the squares and
            their sum carry 2u relative, the root halves it and rounds once, 2u n; moving (p0, p1) by (dp0, dp1) moves the norm by
            at most |dp0| + |dp1|.  dn <= 3u (P0 + P1) + 2u n.  The other norm alike with F transposed.
reciprocal  r = 1 / n: |dr| <= r (dn / n) / (1 - dn / n) + u r; dn >= n leaves no bound (the norm may be zero): +inf.
distance    d = nom (r1 + r2): |dd| <= dnom (r1 + r2) + nom (dr1 + dr2) + 2u d   (the sum of the reciprocals and the product).
A norm that is exactly zero in exact arithmetic gives +inf or NaN there and here alike when its terms are exact (the constructed
cases use integer F and integer points for that); the bound is then taken as 0 and the special value is the expected one.

Decided set.  A match is UNDECIDED for an inlier threshold t when the 50-digit distance lies within TOL * bound of t (TOL = 2: any
two fp64 evaluations lie within twice the bound of each other, so outside that margin the kernel, this restatement and the
reference's numpy all decide as the exact value does).  Scores are compared as given (fp32 widened exactly), so the mask decisions are always decided.
"""
import numpy as np

U = 2.0 ** -53
SLACK = 1.0 + 2.0 ** -20
TOL = 2.0


def _split(F, matches):
    F = np.asarray(F, np.float64).reshape(9)
    m = np.asarray(matches, np.float32).reshape(-1, 4).astype(np.float64)  # the kernel reads fp32 and widens exactly
    return F, m[:, 0], m[:, 1], m[:, 2], m[:, 3]


def dist3(F, matches):
    """F [3,3] (or [9]) fp64, matches [n,4] fp32 -> dist3 [n] fp64 by the header's sequence of operations."""
    F, x1, y1, x2, y2 = _split(F, matches)
    with np.errstate(all="ignore"):
        a0 = (x2 * F[0] + y2 * F[3]) + F[6]
        a1 = (x2 * F[1] + y2 * F[4]) + F[7]
        a2 = (x2 * F[2] + y2 * F[5]) + F[8]
        nom = np.abs((a0 * x1 + a1 * y1) + a2)
        p0 = (F[0] * x1 + F[1] * y1) + F[2]
        p1 = (F[3] * x1 + F[4] * y1) + F[5]
        q0 = (F[0] * x2 + F[3] * y2) + F[6]
        q1 = (F[1] * x2 + F[4] * y2) + F[7]
        r1 = 1.0 / np.sqrt(p0 * p0 + p1 * p1)
        r2 = 1.0 / np.sqrt(q0 * q0 + q1 * q1)
        return nom * (r1 + r2)


def dist3_bound(F, matches):
    """The bound above, per match ([n] fp64; 0 where a norm is exactly zero, +inf where a norm cannot be told from zero)."""
    F, x1, y1, x2, y2 = _split(F, matches)
    aF = np.abs(F)
    ax1, ay1, ax2, ay2 = np.abs(x1), np.abs(y1), np.abs(x2), np.abs(y2)
    with np.errstate(all="ignore"):
        A0, A1, A2 = ax2 * aF[0] + ay2 * aF[3] + aF[6], ax2 * aF[1] + ay2 * aF[4] + aF[7], ax2 * aF[2] + ay2 * aF[5] + aF[8]
        S = A0 * ax1 + A1 * ay1 + A2
        a0, a1, a2 = x2 * F[0] + y2 * F[3] + F[6], x2 * F[1] + y2 * F[4] + F[7], x2 * F[2] + y2 * F[5] + F[8]
        nom = np.abs(a0 * x1 + a1 * y1 + a2)
        dnom = 6 * U * S

        def recip(c0, c1, C0, C1):
            n = np.sqrt(c0 * c0 + c1 * c1)
            dn = 3 * U * (C0 + C1) + 2 * U * n
            rel = dn / n
            r = 1.0 / n
            dr = np.where(rel < 1.0, r * rel / (1.0 - rel) + U * r, np.inf)
            return n, r, dr

        n1, r1, dr1 = recip(F[0] * x1 + F[1] * y1 + F[2], F[3] * x1 + F[4] * y1 + F[5], aF[0] * ax1 + aF[1] * ay1 + aF[2],
                            aF[3] * ax1 + aF[4] * ay1 + aF[5])
        n2, r2, dr2 = recip(F[0] * x2 + F[3] * y2 + F[6], F[1] * x2 + F[4] * y2 + F[7], aF[0] * ax2 + aF[3] * ay2 + aF[6],
                            aF[1] * ax2 + aF[4] * ay2 + aF[7])
        d = nom * (r1 + r2)
        bound = SLACK * (dnom * (r1 + r2) + nom * (dr1 + dr2) + 2 * U * d)
    special = ~np.isfinite(d)  # an exactly zero norm: the value is +inf or NaN in every evaluation of exact terms
    return np.where(special, 0.0, bound)


def dist3_mp(F, matches):
    """The 50-digit twin: a list of mpmath numbers (mpf('inf') / mpf('nan') where a norm is exactly zero)."""
    import mpmath as mp

    F, x1, y1, x2, y2 = _split(F, matches)
    out = []
    with mp.workdps(50):
        f = [mp.mpf(float(v)) for v in F]
        for i in range(len(x1)):
            X1, Y1, X2, Y2 = (mp.mpf(float(v[i])) for v in (x1, y1, x2, y2))
            a0, a1, a2 = X2 * f[0] + Y2 * f[3] + f[6], X2 * f[1] + Y2 * f[4] + f[7], X2 * f[2] + Y2 * f[5] + f[8]
            nom = abs(a0 * X1 + a1 * Y1 + a2)
            n1 = mp.sqrt((f[0] * X1 + f[1] * Y1 + f[2]) ** 2 + (f[3] * X1 + f[4] * Y1 + f[5]) ** 2)
            n2 = mp.sqrt((f[0] * X2 + f[3] * Y2 + f[6]) ** 2 + (f[1] * X2 + f[4] * Y2 + f[7]) ** 2)
            if n1 == 0 or n2 == 0:
                out.append(mp.nan if nom == 0 else mp.inf)
            else:
                out.append(nom * (1 / n1 + 1 / n2))
    return out


def undecided(F, matches, inlier_thds):
    """[n,Ti] bool: match i is undecided for threshold t (the 50-digit distance lies within TOL * bound of it).  The 50-digit twin
    is evaluated only for the matches whose fp64 distance lies within (TOL + 1) * bound of a threshold: the fp64 distance is
    within one bound of the exact one (held against the twin by tests/test_corr_eval_ref_cpu.py), so no other match can be."""
    import mpmath as mp

    thds = np.asarray(inlier_thds, np.float64).reshape(-1)
    d = dist3(F, matches)
    bound = dist3_bound(F, matches)
    out = np.zeros((len(d), len(thds)), bool)
    finite_t = np.isfinite(thds)
    with np.errstate(all="ignore"):
        near = (np.abs(d[:, None] - thds[None, :]) <= (TOL + 1.0) * bound[:, None]) & finite_t[None, :] & np.isfinite(d)[:, None]
        near |= (~np.isfinite(bound))[:, None] & finite_t[None, :]
    rows = np.nonzero(near.any(1))[0]
    if len(rows) == 0:
        return out
    m = np.asarray(matches, np.float32).reshape(-1, 4)
    exact = dist3_mp(F, m[rows])
    with mp.workdps(50):
        for i, e in zip(rows, exact):
            if mp.isnan(e) or mp.isinf(e):
                continue  # NaN and +inf fail every `<` in every evaluation
            for t in np.nonzero(finite_t)[0]:
                if not np.isfinite(bound[i]) or abs(e - mp.mpf(float(thds[t]))) <= mp.mpf(TOL * float(bound[i])):
                    out[i, t] = True
    return out


def clamp_n(n_valid, B, N):
    if n_valid is None:
        return np.full(B, N, np.int64)
    return np.clip(np.asarray(n_valid, np.int64), 0, N)


def pair_table(dist, scores, inlier_thds, mask_thds):
    """One pair: dist [n] fp64, scores [n] or None -> (cnt [Tm,Ti] int, num [Tm] int, ratio [Tm,Ti] fp64), as get_mask and
    inlier_ratio_from_est compute them."""
    dist = np.asarray(dist, np.float64)
    ithd = np.asarray(inlier_thds, np.float64).reshape(-1)
    mthd = [None] if scores is None else list(np.asarray(mask_thds, np.float64).reshape(-1))
    cnt = np.zeros((len(mthd), len(ithd)), np.int64)
    num = np.zeros(len(mthd), np.int64)
    with np.errstate(all="ignore"):
        for m, mt in enumerate(mthd):
            est = dist if mt is None else dist[np.asarray(scores, np.float32).astype(np.float64) < mt]
            num[m] = est.shape[0]
            for t, th in enumerate(ithd):
                cnt[m, t] = np.sum(est < th)
        ratio = cnt.astype(np.float64) / num.astype(np.float64)[:, None]
    return cnt, num, ratio


def table_mean(ratio):
    """ratio [B,Tm,Ti] -> [Tm,Ti]: the pairs added in index order, divided by B (numpy's table.mean(axis=0) for these sizes)."""
    ratio = np.asarray(ratio, np.float64)
    s = np.zeros(ratio.shape[1:])
    with np.errstate(all="ignore"):
        for b in range(ratio.shape[0]):
            s = s + ratio[b]
        return s / np.float64(ratio.shape[0])


def inlier_table(matches=None, F=None, dist=None, scores=None, n_valid=None, inlier_thds=(1.0,), mask_thds=(1.0,)):
    """The whole call on padded arrays: matches [B,N,4] fp32 + F [B,3,3], or dist [B,N] fp32 -> dict(cnt [B,Tm,Ti], num [B,Tm],
    ratio [B,Tm,Ti], dist64 [B,N] (fp64, NaN-free zero past n_valid), dist_out [B,N] fp32, mean [Tm,Ti], num_T [Tm,B])."""
    assert (matches is None) != (dist is None)
    B, N = (matches.shape[:2] if matches is not None else dist.shape)
    n = clamp_n(n_valid, B, N)
    Tm = 1 if scores is None else len(np.reshape(mask_thds, -1))
    Ti = len(np.reshape(inlier_thds, -1))
    cnt, num, ratio = np.zeros((B, Tm, Ti), np.int64), np.zeros((B, Tm), np.int64), np.zeros((B, Tm, Ti))
    d64 = np.zeros((B, N))
    for b in range(B):
        k = int(n[b])
        d = dist3(F[b], matches[b, :k]) if matches is not None else np.asarray(dist[b, :k], np.float32).astype(np.float64)
        d64[b, :k] = d
        cnt[b], num[b], ratio[b] = pair_table(d, None if scores is None else scores[b, :k], inlier_thds, mask_thds)
    with np.errstate(all="ignore"):
        d32 = d64.astype(np.float32)
    return {"cnt": cnt, "num": num, "ratio": ratio, "dist64": d64, "dist_out": d32, "mean": table_mean(ratio), "num_T": num.T.copy()}
