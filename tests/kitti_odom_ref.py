"""The fp64 yardstick of the KITTI odometry table (dfepe_trajectory_align, dfepe_kitti_odometry_errors): a restatement in numpy of
the published KITTI devkit / kitti-odom-eval algorithm, and the bounds the tests hold the kernels (and the host build of
csrc/trajectory_math.h) to.  tests/test_kitti_odom_ref_cpu.py checks this file against the data the reference ships for the stage
(tests/golden/kitti_odom.npz): its segment rows and its five published numbers per sequence.

The algorithm, for est [m,3,4] and gt [n,3,4] absolute poses, m <= n:
    1 re-base     est_i <- inv(est_0) est_i,  gt_i <- inv(gt_0) gt_i                                     (general affine inverse)
    2 align       x = est translations, y = gt translations over the m common frames; MODES below
    3 segments    dist = cumulative path length of gt; for first = 0, step, ... < n and len in 100 .. 800: last = the first i >= first
                  with dist[i] > dist[first] + len; skipped without one, or with last >= m or first >= m;
                  E = inv(inv(est_first) est_last) (inv(gt_first) gt_last); r = arccos(clamp((tr E_R - 1) / 2)), t = |E_t|;
                  row = [first, r / len, t / len, len, len / (0.1 (last - first + 1))]
                  t_rel = 100 mean(t / len), r_rel = mean(r / len) 180 / pi 100, both 0 without segments
    4 ATE         sqrt(mean_i |gt_xyz,i - est_xyz,i|^2) over the m frames
    5 RPE         i < m - 1: E = inv(inv(gt_i) gt_{i+1}) (inv(est_i) est_{i+1}); mean |E_t| and mean angle in degrees; NaN for m = 1

Two legitimate evaluation orders.  Every sum (the means, sigma_x^2 and C of Umeyama, the segment means, the ATE and RPE sums)
is taken either strictly left to right ("seq") or as a balanced pairwise tree ("tree"), and every affine inverse either in closed
form (adjugate over determinant, as csrc/odometry_math.h) or with numpy.linalg.inv on the 4x4 ("linalg").  evaluate(...,
order="seq", inverse="closed") is the yardstick; its distance from evaluate(..., order="tree", inverse="linalg") on the same
inputs is the restatement's OWN spread, and the unit of the bounds:

    bound = 4 spread + k 2^-52 max|entry|                                   (the rule of tests/odometry_ref.py's chain_bound)

with k the number of frames the quantity was reduced over plus 64 for the per-item arithmetic (four inverses and three products
of 3x4 maps are fewer than 64 roundings per entry), and max|entry| the largest entry of the re-based trajectories for lengths,
1 for the entries of a rotation.  Angles are never given a flat tolerance: the bound is put on the arccos argument (tr E_R - 1) / 2
and carried through arccos itself, angle_tol below, which is delta / sin(theta) away from zero and sqrt(2 delta) at zero.

Segment ends are a discrete decision.  dist_bound is what two summation orders of the n step lengths can differ by, n 2^-52
dist[-1] (each of the n partial sums rounds once, relative to at most dist[-1]; doubled for the two sides); a (first, len) pair whose
margin min_i |dist[i] - (dist[first] + len)| is below twice that is undecided.  The tests allow no undecided pair at all.
"""
import numpy as np

import odometry_ref as R

U = R.U
MODES = ("none", "scale", "scale_7dof", "7dof", "6dof")
LENGTHS = (100.0, 200.0, 300.0, 400.0, 500.0, 600.0, 700.0, 800.0)


# ---- sums and inverses in the two orders ---------------------------------------------------------------------------------------
def tsum(a, order):
    """sum over axis 0: "seq" strictly left to right, "tree" a balanced pairwise tree; the empty sum is 0"""
    a = np.asarray(a, np.float64)
    if len(a) == 0:
        return np.zeros(a.shape[1:])
    if order == "seq":
        return np.cumsum(a, axis=0)[-1]
    while len(a) > 1:
        if len(a) % 2:
            a = np.concatenate([a, np.zeros_like(a[:1])])
        a = a[0::2] + a[1::2]
    return a[0]


def _p44(P):
    out = np.tile(np.eye(4), (len(P), 1, 1))
    out[:, :3] = np.asarray(P, np.float64).reshape(-1, 3, 4)
    return out


def inv(P, inverse):
    """[k,12] -> [k,12]"""
    P = np.asarray(P, np.float64).reshape(-1, 12)
    if len(P) == 0:
        return P.copy()
    if inverse == "closed":
        return R._rows(R.inv12(R._cols(P)))
    with np.errstate(all="ignore"):
        try:
            return np.linalg.inv(_p44(P))[:, :3].reshape(-1, 12)
        except np.linalg.LinAlgError:  # one singular matrix fails the whole batch: one by one, NaN for the singular ones
            return np.stack([_safe_inv(M) for M in _p44(P)])[:, :3].reshape(-1, 12)


def _safe_inv(M):
    try:
        return np.linalg.inv(M)
    except np.linalg.LinAlgError:
        return np.full((4, 4), np.nan)


def mul(A, B):
    """[k,12] . [k,12] (or one [12] against many), in the association of odo::affine_mul"""
    A, B = np.asarray(A, np.float64).reshape(-1, 12), np.asarray(B, np.float64).reshape(-1, 12)
    k = max(len(A), len(B))
    if k == 0 or min(len(A), len(B)) == 0:
        return np.zeros((0, 12))
    A, B = np.broadcast_to(A, (k, 12)), np.broadcast_to(B, (k, 12))
    with np.errstate(all="ignore"):
        return R._rows(R.mul12(R._cols(A), R._cols(B)))


def xyz(P):
    return np.asarray(P, np.float64).reshape(-1, 12)[:, [3, 7, 11]]


# ---- steps 1 and 2 -----------------------------------------------------------------------------------------------------------------
def rebase(P, inverse="closed"):
    P = np.asarray(P, np.float64).reshape(-1, 12)
    if len(P) == 0:
        return P.copy()
    return mul(inv(P[:1], inverse), P)


def umeyama(x, y, with_scale=True, order="seq"):
    """x, y [m,3] -> r [3,3], t [3], c with y ~ c r x + t.  sigma_x^2 = 0 gives the IEEE result of the formula; nothing is trapped."""
    m = len(x)
    with np.errstate(all="ignore"):
        mx, my = tsum(x, order) / m, tsum(y, order) / m
        dx, dy = x - mx, y - my
        sx = tsum((dx * dx).reshape(m, 3), order)
        sx = ((sx[0] + sx[1]) + sx[2]) / m
        C = tsum((dy[:, :, None] * dx[:, None, :]).reshape(m, 9), order).reshape(3, 3) / m
        umeyama.last = {"mx": mx, "my": my, "sx": sx, "C": C}  # what the closed form was given (for the per-item tests)
        if not np.isfinite(C).all():
            return np.full((3, 3), np.nan), np.full(3, np.nan), np.nan
        Um, D, Vt = np.linalg.svd(C)
        S = np.eye(3)
        if np.linalg.det(Um) * np.linalg.det(Vt) < 0:
            S[2, 2] = -1.0
        r = Um @ S @ Vt
        c = np.trace(np.diag(D) @ S) / sx if with_scale else 1.0
        t = my - c * (r @ mx)
    return r, t, c


def align(est, gt, mode, order="seq", inverse="closed"):
    """est [m,12], gt [n,12] absolute -> dict est [m,12] (re-based, aligned), gt [n,12] (re-based), r, t, c"""
    assert mode in MODES
    e, g = rebase(est, inverse), rebase(gt, inverse)
    m = len(e)
    r, t, c = np.eye(3), np.zeros(3), 1.0
    if m > 0:
        x, y = xyz(e), xyz(g)[:m]
        with np.errstate(all="ignore"):
            if mode == "scale":
                c = tsum((x * y).reshape(-1), order) / tsum((x * x).reshape(-1), order)
            elif mode != "none":
                r, t, c = umeyama(x, y, mode != "6dof", order)
            e = e.copy()
            e[:, [3, 7, 11]] = e[:, [3, 7, 11]] * c
            if mode in ("7dof", "6dof"):
                e = mul(np.concatenate([r, t[:, None]], axis=1).reshape(1, 12), e)  # scale_7dof keeps only the scale
    out = {"est": e, "gt": g, "r": np.asarray(r, np.float64), "t": np.asarray(t, np.float64), "c": float(c)}
    if m > 0 and mode in ("scale_7dof", "7dof", "6dof"):
        out["sums"] = umeyama.last
    return out


# ---- steps 3 to 5 ------------------------------------------------------------------------------------------------------------------
def distances(gt, order="seq"):
    """cumulative path length [n]; "tree": a Hillis-Steele scan of the step lengths"""
    p = xyz(gt)
    if len(p) == 0:
        return np.zeros(0)
    d = p[1:] - p[:-1]
    step = np.concatenate([[0.0], np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])])
    if order == "seq":
        return np.cumsum(step)
    k = 1
    while k < len(step):
        step = np.concatenate([step[:k], step[k:] + step[:-k]])
        k *= 2
    return step


def dist_bound(dist):
    return 2.0 * len(dist) * U * (dist[-1] if len(dist) else 0.0)


def rel_error(Ea, Eb, Ga, Gb, inverse, est_first=True):
    """the relative-motion error of frames a -> b: [k,12] each.  -> cos argument (clamped), angle, |E_t|.
    est_first: E = inv(d_est) d_gt (segments); otherwise E = inv(d_gt) d_est (RPE)."""
    dG, dE = mul(inv(Ga, inverse), Gb), mul(inv(Ea, inverse), Eb)
    E = mul(inv(dE, inverse), dG) if est_first else mul(inv(dG, inverse), dE)
    if len(E) == 0:
        return np.zeros(0), np.zeros(0), np.zeros(0)
    with np.errstate(all="ignore"):
        a = (((E[:, 0] + E[:, 5]) + E[:, 10]) - 1.0) / 2.0
        a = np.where(np.isnan(a), a, np.clip(a, -1.0, 1.0))
        ang = np.arccos(a)
        t = np.sqrt((E[:, 3] * E[:, 3] + E[:, 7] * E[:, 7]) + E[:, 11] * E[:, 11])
    return a, ang, t


def segments(est, gt, step=10, order="seq", inverse="closed"):
    """est [m,12] aligned, gt [n,12] re-based -> dict over ALL (first, len) pairs, first-major: first, len, last (n where there is
    none), valid, margin, cosarg, r, t (angle and length before the division by len), rows [pairs,5] (zero where not valid)"""
    m, n = len(est), len(gt)
    dist = distances(gt, order)
    firsts = np.arange(0, n, step)
    first = np.repeat(firsts, 8)
    ln = np.tile(np.array(LENGTHS), len(firsts))
    if n == 0:
        z = np.zeros(0)
        return {"first": first, "len": ln, "last": first, "valid": z.astype(bool), "margin": z, "cosarg": z, "r": z, "t": z,
                "rows": np.zeros((0, 5)), "dist": dist}
    target = dist[first] + ln
    last = np.searchsorted(dist, target, side="right")  # dist never decreases: the first i with dist[i] > target is >= first
    margin = np.abs(dist[None, :] - target[:, None]).min(axis=1)
    valid = (last < n) & (last < m) & (first < m)
    a, ang, t = np.zeros(len(first)), np.zeros(len(first)), np.zeros(len(first))
    v = np.nonzero(valid)[0]
    a[v], ang[v], t[v] = rel_error(est[first[v]], est[last[v]], gt[first[v]], gt[last[v]], inverse)
    rows = np.zeros((len(first), 5))
    rows[v] = np.stack([first[v].astype(np.float64), ang[v] / ln[v], t[v] / ln[v], ln[v], ln[v] / (0.1 * (last[v] - first[v] + 1))], axis=1)
    return {"first": first, "len": ln, "last": last, "valid": valid, "margin": margin, "cosarg": a, "r": ang, "t": t, "rows": rows,
            "dist": dist}


def evaluate(est, gt, mode="scale_7dof", step=10, order="seq", inverse="closed"):
    """The whole table for one sequence: est [m,3,4] / [m,12], gt [n,3,4] / [n,12] absolute poses, m <= n."""
    est, gt = np.asarray(est, np.float64).reshape(-1, 12), np.asarray(gt, np.float64).reshape(-1, 12)
    assert len(est) <= len(gt)
    al = align(est, gt, mode, order, inverse)
    e, g, m = al["est"], al["gt"], len(est)
    seg = segments(e, g, step, order, inverse)
    v = seg["valid"]
    cnt = int(v.sum())
    with np.errstate(all="ignore"):
        t_rel = 100.0 * (tsum(seg["rows"][v, 2], order) / cnt) if cnt else 0.0
        r_rel = (tsum(seg["rows"][v, 1], order) / cnt) * 180.0 / np.pi * 100.0 if cnt else 0.0
        d = xyz(g)[:m] - xyz(e)
        sq = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        ate = np.sqrt(tsum(sq, order) / m) if m else np.nan
        k = max(m - 1, 0)
        a, ang, t = rel_error(e[:k], e[1:k + 1], g[:k], g[1:k + 1], inverse, est_first=False)
        rpe_t = tsum(t, order) / k if k else np.nan
        rpe_r = (tsum(ang, order) / k) * 180.0 / np.pi if k else np.nan
    return {"align": al, "seg": seg, "count": cnt, "summary": np.array([t_rel, r_rel, ate, rpe_t, rpe_r], np.float64),
            "ate_sq": sq, "rpe_cosarg": a, "rpe_r": ang, "rpe_t": t}


# ---- bounds --------------------------------------------------------------------------------------------------------------------
def angle_tol(cosarg, delta):
    """How far arccos moves when its argument moves by at most delta (and stays clamped to [-1, 1]): evaluated through arccos
    itself, which is delta / sin(theta) away from 0 and pi and at most sqrt(2 delta) there; plus four spacings of the angle for
    the two arccos evaluations."""
    a = np.asarray(cosarg, np.float64)
    th = np.arccos(a)
    lo, hi = np.arccos(np.clip(a + delta, -1.0, 1.0)), np.arccos(np.clip(a - delta, -1.0, 1.0))
    return np.maximum(th - lo, hi - th) + 4.0 * U * np.maximum(th, 1.0)


def spread(a, b):
    with np.errstate(all="ignore"):
        d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return np.where(np.isnan(d), 0.0, d)


def bounds(ref, alt):
    """ref, alt: evaluate() of the same inputs in the two orders -> dict of bounds in ref's layout:
    est, gt (aligned / re-based poses, per entry), rtc [13] (r, t, c), seg_t, seg_r (per pair, before / len), ate_sq, rpe_t, rpe_r
    (per frame), summary [5], and the scalars they were made of: big (max |entry| of the trajectories), frames."""
    m, n = len(ref["align"]["est"]), len(ref["align"]["gt"])
    k = 64.0 + max(m, n)
    fin = lambda a: np.abs(a[np.isfinite(a)]).max() if np.isfinite(a).any() else 0.0
    big = max(fin(ref["align"]["est"]), fin(ref["align"]["gt"]), 1.0)
    ent = np.ones(12)
    ent[[3, 7, 11]] = big
    out = {"big": big, "frames": max(m, n)}
    out["est"] = 4.0 * spread(ref["align"]["est"], alt["align"]["est"]) + k * U * ent
    out["gt"] = 4.0 * spread(ref["align"]["gt"], alt["align"]["gt"]) + 64.0 * U * ent
    rtc = lambda e: np.concatenate([e["align"]["r"].reshape(9), e["align"]["t"], [e["align"]["c"]]])
    a, b = rtc(ref), rtc(alt)
    scale = np.concatenate([np.ones(9), np.full(3, big), [max(abs(a[12]), 1.0) if np.isfinite(a[12]) else 1.0]])
    out["rtc"] = 4.0 * spread(a, b) + k * U * scale
    s, s2 = ref["seg"], alt["seg"]
    out["seg_t"] = 4.0 * spread(s["t"], s2["t"]) + k * U * big
    out["seg_r"] = angle_tol(s["cosarg"], 4.0 * spread(s["cosarg"], s2["cosarg"]) + k * U)
    out["ate_sq"] = 4.0 * spread(ref["ate_sq"], alt["ate_sq"]) + k * U * big * big
    out["rpe_t"] = 4.0 * spread(ref["rpe_t"], alt["rpe_t"]) + k * U * big
    out["rpe_r"] = angle_tol(ref["rpe_cosarg"], 4.0 * spread(ref["rpe_cosarg"], alt["rpe_cosarg"]) + k * U)
    # the five numbers: the mean of the per-item bounds, plus the summation of `terms` numbers in another order, plus the spread
    sm, v = np.zeros(5), s["valid"]
    cnt = max(int(v.sum()), 1)
    mean_tol = lambda items, terms: (items.mean() if len(items) else 0.0) + terms * U * (np.abs(items).max() if len(items) else 0.0)
    sm[0] = 100.0 * (mean_tol(out["seg_t"][v] / s["len"][v], cnt) + cnt * U * fin(s["rows"][:, 2]))
    sm[1] = 180.0 / np.pi * 100.0 * (mean_tol(out["seg_r"][v] / s["len"][v], cnt) + cnt * U * fin(s["rows"][:, 1]))
    # ATE = sqrt(Q) with Q the mean square, known to q: sqrt moves by at most min(q / sqrt(Q), sqrt(q))
    ate, q = ref["summary"][2], mean_tol(out["ate_sq"], m) + m * U * fin(ref["ate_sq"])
    if np.isfinite(ate):
        sm[2] = min(q / ate, np.sqrt(q)) if ate > 0 else np.sqrt(q)
    sm[3] = mean_tol(out["rpe_t"], m) + m * U * fin(ref["rpe_t"])
    sm[4] = 180.0 / np.pi * (mean_tol(out["rpe_r"], m) + m * U * fin(ref["rpe_r"]))
    out["summary"] = 4.0 * spread(ref["summary"], alt["summary"]) + sm
    return out


def reference(est, gt, mode="scale_7dof", step=10):
    """the yardstick, the other order, and the bounds, for one sequence"""
    ref = evaluate(est, gt, mode, step, "seq", "closed")
    alt = evaluate(est, gt, mode, step, "tree", "linalg")
    return ref, alt, bounds(ref, alt)


def undecided(seg):
    """the (first, len) pairs whose end frame two summation orders of dist could place differently"""
    return np.nonzero(seg["margin"] < 2.0 * dist_bound(seg["dist"]))[0] if len(seg["margin"]) else np.zeros(0, int)
