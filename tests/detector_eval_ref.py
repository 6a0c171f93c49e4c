"""fp64 restatement of the front-end detector evaluation the tests hold csrc/detector_eval.hip and csrc/detector_eval_math.h to:
compute_repeatability (evaluations/detector_evaluation.py:150-279), the matching score (deepFEPE/evaluate_frontend.py:176-183)
and the average precision (evaluate_frontend.py:244-275) as include/dfepe.h specifies them.  numpy only, written from the
specification, independently of the kernels: the distances are one N1 x N2 matrix, the selection is numpy's stable argsort, the
sums are numpy's.  A 50-digit mpmath twin covers the warp (through the adjugate) and the distance.

Bounds (u = 2^-53, the unit roundoff; every bound is on |an fp64 evaluation - the exact value|, for ANY order of the operations
and with or without fused multiply-adds, so two evaluations differ by at most twice the bound: TOL = 2)
------------------------------------------------------------------------------------------------------------------------------
adjugate  Each entry is a difference of two products, three roundings at most:  dM = 2u (|p1| + |p2|)  (first order; the factor
          SLACK = 1 + 2^-20 on every final bound covers the second-order terms).  For H itself dM = 0.
warp      X = m0 x + m1 y + m2 is two products and two sums: |dX| <= 3u aX + (dM0 |x| + dM1 |y| + dM2) =: eX with aX = |m0 x| +
          |m1 y| + |m2|; Y and W alike.  wx = X / W: with rW = eW / |W| < 1 the quotient moves by at most
          (eX + |wx| eW) / (|W| (1 - rW)), and the division adds u |wx|.  rW >= 1 (W may be zero): no bound, the point is undecided.
distance  dx = ax - bx carries the two warps' errors and one rounding: gx = eax + ebx + u |dx|.  d = sqrt(dx^2 + dy^2): the sum of
          squares has relative error 2u, the root halves it and rounds once: 2u d.  Moving (dx, dy) by (gx, gy) moves the norm by
          at most gx + gy.  e_d = gx + gy + 2u d.
minimum   |min_j a_j - min_j b_j| <= max_j |a_j - b_j| over the entries j that can be the minimum in either evaluation: the bound of
          a minimum is the largest e_d among the entries of its row (column) whose interval reaches below the smallest upper end.
sum       n terms in any order: (n - 1) u sum|terms| on top of the terms' own bounds; loc_err = s1 / c + s2 / c adds two divisions
          and one sum: 3u |loc_err|.
AP        every term tp / cnt is one division of exact integers (u relative), the sum of P positive terms (P - 1) u, the division
          by P one more: (P + 1) u AP.
exact     When H is integer-valued with last row (0, 0, 1) (so is its adjugate, checked), and the coordinates are multiples of 1/2
          (all below 2^26), every product, sum and quotient above is exact: the warp bounds are 0, dx and dy are exact, 4 d^2 is an
          exact integer, and the correctly rounded root carries u d -- 0 when 4 d^2 is a perfect square.  That is what makes the lattice
          family's `<=` and inside edges exact.
Every decision -- inside or outside (each of the four comparisons of both rules), min <= thresh -- is decided when its margin
exceeds TOL times the bound, or the bound is 0.  The rank at the k-th place compares the probabilities as given (no arithmetic),
so it is decided whenever the inside decisions of its set are.  `undecided` counts the rest; the shared cases are chosen so that
it is 0.
"""
import numpy as np

U = 2.0 ** -53
SLACK = 1.0 + 2.0 ** -20
TOL = 2.0


def adjugate(H):
    """(adj(H) [3,3], dM [3,3]): the transposed cofactors and the bound on each."""
    h = np.asarray(H, np.float64).reshape(9)
    pairs = [((4, 8), (5, 7)), ((2, 7), (1, 8)), ((1, 5), (2, 4)), ((5, 6), (3, 8)), ((0, 8), (2, 6)), ((2, 3), (0, 5)),
             ((3, 7), (4, 6)), ((1, 6), (0, 7)), ((0, 4), (1, 3))]
    A = np.array([h[a] * h[b] - h[c] * h[d] for (a, b), (c, d) in pairs])
    dA = np.array([2 * U * (abs(h[a] * h[b]) + abs(h[c] * h[d])) for (a, b), (c, d) in pairs])
    if _integral(h) and _integral(A):
        dA[:] = 0.0
    return A.reshape(3, 3), dA.reshape(3, 3)


def _integral(a, unit=1.0):
    """Whether every entry is a multiple of `unit` (1, or 1/2 for coordinates) below 2^26."""
    a = np.asarray(a, np.float64) / unit
    return bool(np.isfinite(a).all() and (a == np.rint(a)).all() and (np.abs(a) < 2.0 ** 26).all())


def warp(M, dM, pts):
    """pts [n,2] -> (w [n,2], e [n,2]): the warp by M (entrywise bound dM) and the bound on each coordinate (inf: none)."""
    M = np.asarray(M, np.float64).reshape(3, 3)
    dM = np.zeros((3, 3)) if dM is None else np.asarray(dM, np.float64).reshape(3, 3)
    p = np.asarray(pts, np.float64).reshape(-1, 2)
    hom = np.concatenate([p, np.ones((len(p), 1))], 1)
    with np.errstate(all="ignore"):
        V = hom @ M.T
        w = V[:, :2] / V[:, 2:]
        if _integral(M) and (M[2] == (0, 0, 1)).all() and not dM.any() and _integral(p, 0.5):
            return w, np.zeros_like(w)
        a = np.abs(hom)
        E = 3 * U * (a @ np.abs(M).T) + a @ dM.T
        W = np.abs(V[:, 2])
        rW = E[:, 2] / W
        e = (E[:, :2] + np.abs(w) * E[:, 2:]) / (W * (1 - rW))[:, None] + U * np.abs(w)
        e = np.where((rW < 1)[:, None] & np.isfinite(w), e * SLACK, np.inf)
    return w, e


def _decided(value, edge, e):
    """Whether the comparison of value against edge is safe from a perturbation of TOL e."""
    with np.errstate(all="ignore"):
        return (e == 0) | (np.abs(value - edge) > TOL * e)


def inside(w, e, height, width, closed):
    """(mask [n], decided [n]) of 0 <= x < width, 0 <= y < height (closed: <= width - 1, <= height - 1)."""
    x, y = w[:, 0], w[:, 1]
    hx, hy = (width - 1.0, height - 1.0) if closed else (float(width), float(height))
    with np.errstate(all="ignore"):
        m = (x >= 0) & ((x <= hx) if closed else (x < hx)) & (y >= 0) & ((y <= hy) if closed else (y < hy))
    # a value that is not finite with a finite bound cannot happen; with no bound the point is undecided
    ok = np.isfinite(e).all(1) & _decided(x, 0.0, e[:, 0]) & _decided(x, hx, e[:, 0]) & _decided(y, 0.0, e[:, 1]) & _decided(y, hy, e[:, 1])
    return m, ok


def select_k_best(prob, keep_k):
    """prob [n] of the kept points -> the positions select_k_best keeps, in argsort order: the last min(keep_k, n) of a stable
    ascending argsort; numpy reads [-0:] as the whole array.  With two columns the reference selects nothing: not called."""
    order = np.argsort(np.asarray(prob, np.float64), kind="stable")
    start = min(int(keep_k), len(order))
    return order[-start:]


def _min_bound(D, eD, axis):
    """The bound of the minimum along `axis`: the largest e_d among the entries that can be the minimum, that is whose lower end
    D - TOL e_d does not exceed the smallest upper end D + TOL e_d."""
    if D.shape[axis] == 0 or D.shape[1 - axis] == 0:
        return np.zeros(D.shape[1 - axis])
    upper = (D + TOL * eD).min(axis, keepdims=True)
    return np.where(D - TOL * eD <= upper, eD, 0.0).max(axis)


def repeatability_pair(kp1, kp2, H, height, width, keep_k, thresh):
    """One pair.  kp1 [n1,C], kp2 [n2,C] float64, thresh: a sequence of T.  Returns a dict: the integer outputs (count1, count2 [T],
    kept1, kept2, n_unwarped), the continuous ones with their bounds (repeatability [T], loc_err [T], loc_err_bound [T]),
    `undecided` (the number of decisions inside TOL bounds of their edge), and the intermediate values the mpmath twin compares
    (w1, e1, w2, e2, sel1, sel2, p1, p2, D, eD, min1, min2)."""
    kp1, kp2 = np.asarray(kp1, np.float64), np.asarray(kp2, np.float64)
    assert kp1.ndim == 2 and kp2.ndim == 2, "rows (x, y[, prob]); an empty set is [0,C]"
    C = kp1.shape[1] if len(kp1) else (kp2.shape[1] if len(kp2) else 2)
    Hm = np.asarray(H, np.float64).reshape(3, 3)
    A, dA = adjugate(Hm)
    undecided = 0
    w2, e2 = warp(A, dA, kp2[:, :2])
    keep2, ok2 = inside(w2, e2, height, width, False)
    unw, oku = inside(w2, e2, height, width, True)
    w1, e1 = warp(Hm, None, kp1[:, :2])
    keep1, ok1 = inside(w1, e1, height, width, False)
    undecided += int((~ok1).sum() + (~ok2).sum() + (~oku).sum())
    i1, i2 = np.flatnonzero(keep1), np.flatnonzero(keep2)
    if C > 2:
        i1 = i1[select_k_best(kp1[i1, 2], keep_k)]
        i2 = i2[select_k_best(kp2[i2, 2], keep_k)]
    i1, i2 = np.sort(i1), np.sort(i2)
    p1, q1 = w1[i1], e1[i1]                                   # image 1: the warped points
    p2, q2 = kp2[i2, :2], np.zeros((len(i2), 2))              # image 2: the points themselves
    k1, k2 = len(i1), len(i2)
    d = p1[:, None, :] - p2[None, :, :]
    D = np.sqrt((d * d).sum(2))
    exact = (not q1.any()) and _integral(p1, 0.5) and _integral(p2, 0.5)
    if exact:
        d2 = (d * d).sum(2)
        eD = np.where(np.rint(2 * D) ** 2 == 4 * d2, 0.0, U * D)  # 4 d^2 is an exact integer
    else:
        g = q1[:, None, :] + q2[None, :, :] + U * np.abs(d)
        eD = (g.sum(2) + 2 * U * D) * SLACK
    T = len(thresh)
    out = {"kept1": k1, "kept2": k2, "n_unwarped": int(unw.sum()), "count1": np.zeros(T, np.int64), "count2": np.zeros(T, np.int64),
           "repeatability": np.zeros(T), "loc_err": np.full(T, -1.0), "loc_err_bound": np.zeros(T),
           "w1": w1, "e1": e1, "w2": w2, "e2": e2, "sel1": i1, "sel2": i2, "p1": p1, "p2": p2, "D": D, "eD": eD}
    min1 = D.min(1) if k2 else np.zeros(0)
    min2 = D.min(0) if k1 else np.zeros(0)
    b1 = _min_bound(D, eD, 1) if k2 else np.zeros(0)
    b2 = _min_bound(D, eD, 0) if k1 else np.zeros(0)
    out["min1"], out["min2"] = min1, min2
    for t, th in enumerate(thresh):
        c1m, c2m = min1 <= th, min2 <= th
        undecided += int((~_decided(min1, th, b1)).sum() + (~_decided(min2, th, b2)).sum())
        c1, c2 = int(c1m.sum()), int(c2m.sum())
        out["count1"][t], out["count2"][t] = c1, c2
        c = c1 + c2
        if c > 0:
            s1, s2 = min1[c1m].sum(), min2[c2m].sum()
            out["repeatability"][t] = c / (k1 + k2)
            out["loc_err"][t] = s1 / c + s2 / c
            es = b1[c1m].sum() + b2[c2m].sum() + U * (max(c1 - 1, 0) * s1 + max(c2 - 1, 0) * s2)
            out["loc_err_bound"][t] = (es / c + 3 * U * out["loc_err"][t]) * SLACK
    out["undecided"] = undecided
    return out


def average_precision(labels, scores):
    """labels [n] (non-zero: positive), scores [n] float64 -> dict(ap, ap_bound, n_pos, tp_at [n], cnt_at [n]):
    AP = (1/P) sum over positives of TP(s_i) / CNT(s_i); 0 without an entry or a positive."""
    lab = np.asarray(labels).reshape(-1) != 0
    s = np.asarray(scores, np.float64).reshape(-1)
    with np.errstate(invalid="ignore"):
        ge = s[None, :] >= s[:, None]          # ge[i, j]: score_j >= score_i
    cnt = ge.sum(1).astype(np.int64)
    tp = (ge & lab[None, :]).sum(1).astype(np.int64)
    P = int(lab.sum())
    ap = 0.0
    if P > 0:
        with np.errstate(all="ignore"):
            ap = float((tp[lab] / cnt[lab]).sum() / P)
    return {"ap": ap, "ap_bound": (P + 1) * U * abs(ap) * SLACK, "n_pos": P, "tp_at": tp, "cnt_at": cnt}


def matching_score(n_inliers, n_kp1, n_unwarped):
    """One exact integer product and one division: held exactly."""
    with np.errstate(all="ignore"):
        return np.float64(2 * int(n_inliers)) / np.float64(int(n_kp1) + int(n_unwarped))


# ---- the 50-digit twin ---------------------------------------------------------------------------------------------------------
def mp_warp(H, pts, inverse):
    """pts [n,2] warped by H (inverse: by adj(H)) at 50 digits from the fp64 entries -> list of (x, y) mpf, None where w = 0."""
    import mpmath as mp

    mp.mp.dps = 50
    h = [mp.mpf(float(v)) for v in np.asarray(H, np.float64).reshape(9)]
    if inverse:
        h = [h[4] * h[8] - h[5] * h[7], h[2] * h[7] - h[1] * h[8], h[1] * h[5] - h[2] * h[4],
             h[5] * h[6] - h[3] * h[8], h[0] * h[8] - h[2] * h[6], h[2] * h[3] - h[0] * h[5],
             h[3] * h[7] - h[4] * h[6], h[1] * h[6] - h[0] * h[7], h[0] * h[4] - h[1] * h[3]]
    out = []
    for x, y in np.asarray(pts, np.float64).reshape(-1, 2):
        x, y = mp.mpf(float(x)), mp.mpf(float(y))
        W = h[6] * x + h[7] * y + h[8]
        out.append(None if W == 0 else ((h[0] * x + h[1] * y + h[2]) / W, (h[3] * x + h[4] * y + h[5]) / W))
    return out


def mp_dist(a, b):
    import mpmath as mp

    return mp.sqrt((a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2)
