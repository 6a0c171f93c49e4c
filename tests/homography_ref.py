"""fp64 restatement of the RANSAC homography estimator the tests hold csrc/homography.hip and csrc/homography_math.h to:
OpenCV 3.4's findHomography(RANSAC) as include/dfepe.h (dfepe_ransac_homography) specifies it -- sampler with checkSubset,
4-point solve, error, RANSACUpdateNumIters and the selection rule, the refit over the inliers, the Levenberg-Marquardt
refinement -- and the two evaluation measures (transfer distance, mean corner error).  numpy only, written from the
specification, independently of the kernels: the null space comes from numpy's QR or SVD (two routes, run against each other),
the eigen decompositions from numpy.linalg.eigh, every sum from numpy.  The stream is tests/ransac_ref.py's.  A 50-digit mpmath
twin covers the 4-point solve, the refit and one LM residual / Jacobian evaluation.

Bands (the derived bounds next to every decision, as tests/lmeds_ref.py puts one next to every median)
--------------------------------------------------------------------------------------------------------
A hypothesis H comes from a null vector of an 8x9 system A with singular values s1 >= .. >= s8 > s9 = 0.  Rounding perturbs A by
|dA| <= c1 eps s1, and the null vector then turns by at most |dA| / s8 (Wedin), so every entry of the normalised H0 carries an
error of at most c1 eps kappa with kappa = s1 / s8.  The transfer of a correspondence is a ratio of two affine forms of H0's
entries in normalised coordinates of size O(1), mapped back to pixels by the target scale 1 / s_dst <= L (L: the largest |pixel
coordinate| of the pair, at least 1), and divided by |w_n|, the normalised denominator; so the transferred point moves by at
most dd = c kappa eps L / min(1, |w|) pixels, and err = d^2 by at most 2 d dd + dd^2.  Around the decision err <= t^2 that is the
relative band   rel(i) = 2 dd / t + (dd / t)^2   with c = 512 (c1 = 8 for the 72 products and sums of a Householder QR of this
size, times 64 for the two 3x3 products of the de-normalisation, whose entries reach L, and the evaluation itself), never less
than 64 eps for the evaluation alone.  c L is above four times the measured yardstick of tests/homography_cases.py, so a result
inside its tolerance decides every correspondence outside the band alike.
A correspondence whose |err / t^2 - 1| <= rel(i) may be counted either way: counts are intervals [lo, hi].  The LM gain ratio R
is a ratio of two differences of sums over n inliers; a relative band around 0.25 and 0.75
(and around S_d < S) marks an iteration whose branch rounding may choose: lm_band below derives it.
"""
import math

import numpy as np

import ransac_ref as rr

FLT_EPSILON = rr.FLT_EPSILON
DBL_EPSILON = rr.DBL_EPSILON
DBL_MIN = rr.DBL_MIN
NO_MODEL, NO_SAMPLE = -1, -2
ALL_POINTS, NO_REFINE = 1, 2
BAND_C = 512.0
LM_ITERS = 10


def update_num_iters4(p, ep, niters):
    """OpenCV's RANSACUpdateNumIters(p, ep, 4, niters), (1 - ep)^4 by two squarings."""
    p = min(max(p, 0.0), 1.0)
    ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, DBL_MIN)
    q = 1.0 - ep
    q2 = q * q
    den = 1.0 - q2 * q2
    if den < DBL_MIN:
        return 0
    ln, ld = math.log(num), math.log(den)
    if ld >= 0 or -ln >= niters * (-ld):
        return niters
    return int(np.rint(ln / ld))


def _det_tri(p, a, b, c, off):
    a0, a1, b0, b1, c0, c1 = (float(p[a][off]), float(p[a][off + 1]), float(p[b][off]), float(p[b][off + 1]), float(p[c][off]),
                              float(p[c][off + 1]))
    return (b0 * c1 - b1 * c0) - (a0 * c1 - a1 * c0) + (a0 * b1 - a1 * b0)


def orientation_ok(p4):
    neg = sum(1 for (a, b, c) in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)) if _det_tri(p4, a, b, c, 0) * _det_tri(p4, a, b, c, 2) < 0.0)
    return neg in (0, 4)


def check_subset(p4):
    p4 = np.asarray(p4, np.float32)
    return (not rr.collinear_last(p4[:, 0], p4[:, 1])) and (not rr.collinear_last(p4[:, 2], p4[:, 3])) and orientation_ok(p4)


def draw_sample(seed, k, pts, max_attempts=1000):
    """Iteration k's 4 indices into pts [n,4] (float32 pixels), or None when every attempt failed checkSubset."""
    pts = np.asarray(pts, np.float32)
    n = pts.shape[0]
    s = rr.Stream(seed, k)
    for _ in range(max_attempts):
        idx = []
        while len(idx) < 4:
            v = s.index(n)
            if v not in idx:
                idx.append(v)
        if check_subset(pts[idx]):
            return idx
    return None


def normalisation(p):
    """(c [4], scale [4]) of runKernel, or None when a sum |x - c| is below FLT_EPSILON."""
    p = np.asarray(p, np.float64)
    c = p.mean(0)
    s = np.abs(p - c).sum(0)
    if (s < FLT_EPSILON).any():
        return None
    return c, len(p) / s


def system(p, c, sc):
    q = (np.asarray(p, np.float64) - c) * sc
    X, Y, x, y = q.T
    o, z = np.ones_like(X), np.zeros_like(X)
    Lx = np.stack([X, Y, o, z, z, z, -x * X, -x * Y, -x], 1)
    Ly = np.stack([z, z, z, X, Y, o, -y * X, -y * Y, -y], 1)
    return np.stack([Lx, Ly], 1).reshape(-1, 9)


def denormalise(h0, c, sc):
    H0 = np.asarray(h0, np.float64).reshape(3, 3)
    Ts = np.array([[sc[0], 0, -c[0] * sc[0]], [0, sc[1], -c[1] * sc[1]], [0, 0, 1.0]])
    Tdi = np.array([[1.0 / sc[2], 0, c[2]], [0, 1.0 / sc[3], c[3]], [0, 0, 1.0]])
    H = Tdi @ H0 @ Ts
    if not (abs(H[2, 2]) > 0.0) or not np.isfinite(H[2, 2]):
        return None
    H = H / H[2, 2]
    H[2, 2] = 1.0
    return H if np.isfinite(H).all() else None


def solve4(p4, route="qr"):
    """p4 [4,4] pixels -> (H [3,3] or None, kappa = s1 / s8 of the 8x9 system).  route: 'qr' (the last column of the complete Q of
    the transpose, what the kernels do with their own Householder QR) or 'svd' (the last right singular vector)."""
    nrm = normalisation(np.asarray(p4, np.float32))
    if nrm is None:
        return None, math.inf
    A = system(np.asarray(p4, np.float32), *nrm)
    sv = np.linalg.svd(A, compute_uv=False)
    kappa = sv[0] / sv[7] if sv[7] > 0 else math.inf
    if route == "qr":
        h0 = np.linalg.qr(A.T, mode="complete")[0][:, 8]
    else:
        h0 = np.linalg.svd(A)[2][8]
    return denormalise(h0, *nrm), kappa


def transfer(H, pts):
    """(X / w, Y / w, w) of the source points under H."""
    pts = np.asarray(pts, np.float64)
    H = np.asarray(H, np.float64).reshape(3, 3)
    w = H[2, 0] * pts[:, 0] + H[2, 1] * pts[:, 1] + H[2, 2]
    X = H[0, 0] * pts[:, 0] + H[0, 1] * pts[:, 1] + H[0, 2]
    Y = H[1, 0] * pts[:, 0] + H[1, 1] * pts[:, 1] + H[1, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        return X / w, Y / w, w


def errors(H, pts):
    """computeError: squared transfer distance per correspondence (inf where w = 0: never an inlier)."""
    pts = np.asarray(pts, np.float64)
    xw, yw, w = transfer(H, pts)
    e = (xw - pts[:, 2]) ** 2 + (yw - pts[:, 3]) ** 2
    return np.where(w != 0.0, e, np.inf)


def band(H, pts, t, kappa):
    """The relative band rel(i) around t^2 of every correspondence (module docstring)."""
    pts = np.asarray(pts, np.float64)
    _, _, w = transfer(H, pts)
    L = max(1.0, float(np.abs(pts).max()))
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        dd = BAND_C * kappa * DBL_EPSILON * L / np.minimum(1.0, np.abs(w))
        rel = 2.0 * dd / t + (dd / t) ** 2
    return np.maximum(np.nan_to_num(rel, nan=np.inf), 64.0 * DBL_EPSILON)


def classify(H, pts, t, kappa):
    """(sure inlier [n] bool, ambiguous [n] bool, err / t^2 [n])."""
    ratio = errors(H, pts) / (t * t)
    rel = band(H, pts, t, kappa)
    with np.errstate(invalid="ignore"):
        amb = np.abs(ratio - 1.0) <= rel
    amb &= np.isfinite(ratio)
    return (ratio <= 1.0) & ~amb, amb, ratio


def select(counts, n, confidence, max_iters):
    """The sequential rule over a count table [max_iters] -> (best count, best k, iterations consumed)."""
    best, niters, bk, k = 0, max_iters, -1, 0
    while k < niters:
        c = int(counts[k])
        if c == NO_SAMPLE:
            break
        if c > max(best, 3):
            best, bk = c, k
            niters = update_num_iters4(confidence, (n - c) / n, niters)
        k += 1
    return best, bk, k


def refit(pin, want_kappa=False):
    """runKernel over the inliers pin [m,4]: the eigenvector of the smallest eigenvalue of the 9x9 L^T L.  H or None; with
    want_kappa also the conditioning of that eigenvector, e9 / (e2 - e1) for the eigenvalues e1 <= .. <= e9 (a perturbation
    of L^T L of relative size eps turns it by that much)."""
    nrm = normalisation(pin)
    if nrm is None:
        return (None, math.inf) if want_kappa else None
    A = system(pin, *nrm)
    w, V = np.linalg.eigh(A.T @ A)
    H = denormalise(V[:, 0], *nrm)
    gap = w[1] - w[0]
    return (H, float(w[8] / gap) if gap > 0 else math.inf) if want_kappa else H


def lm_eval(h, pin):
    """Residuals r [m,2] and Jacobian J [m,2,8] of the refinement at h [8]."""
    pin = np.asarray(pin, np.float64)
    X, Y = pin[:, 0], pin[:, 1]
    w = h[6] * X + h[7] * Y + 1.0
    with np.errstate(divide="ignore"):
        wi = np.where(np.abs(w) > DBL_EPSILON, 1.0 / w, 0.0)
    xi = (h[0] * X + h[1] * Y + h[2]) * wi
    yi = (h[3] * X + h[4] * Y + h[5]) * wi
    r = np.stack([xi - pin[:, 2], yi - pin[:, 3]], 1)
    z = np.zeros_like(X)
    Jx = np.stack([X * wi, Y * wi, wi, z, z, z, -X * wi * xi, -Y * wi * xi], 1)
    Jy = np.stack([z, z, z, X * wi, Y * wi, wi, -X * wi * yi, -Y * wi * yi], 1)
    return r, np.stack([Jx, Jy], 1)


def _sym_solve(M, v):
    """(M^-1 v, diag(M^-1)) by the eigen decomposition with the zero rule |e_i| <= 2 eps sum |e_j|."""
    e, Q = np.linalg.eigh(M)
    keep = np.abs(e) > 2.0 * DBL_EPSILON * np.abs(e).sum()
    inv = np.where(keep, 1.0 / np.where(keep, e, 1.0), 0.0)
    return Q @ (inv * (Q.T @ v)), ((Q * Q) * inv).sum(1)


def lm_refine(h, pin):
    """The refinement of include/dfepe.h step 7.  Returns (h, info) with info = dict(R [iterations], S0, S1, S [per iteration],
    Sd [per iteration], iters)."""
    h = np.array(h, np.float64)

    def full(hh):
        r, J = lm_eval(hh, pin)
        Jf = J.reshape(-1, 8)
        return Jf.T @ Jf, Jf.T @ r.reshape(-1), float((r * r).sum()), float(np.abs(r).max())

    A, v, S, rmax = full(h)
    D = np.diag(A).copy()
    lam, lc = 1.0, 0.75
    info = {"R": [], "S": [], "Sd": [], "d": [], "h": [], "S0": S}
    it = 0
    while it < LM_ITERS:
        d, _ = _sym_solve(A + lam * np.diag(D) if lam > 0 else A.copy(), v)
        hd = h - d
        rd, _ = lm_eval(hd, pin)
        Sd = float((rd * rd).sum())
        dS = float(d @ (2.0 * v - A @ d))
        R = (S - Sd) / (dS if abs(dS) > DBL_EPSILON else 1.0)
        info["R"].append(R)
        info["S"].append(S)
        info["Sd"].append(Sd)
        info["d"].append(d.copy())
        info["h"].append(h.copy())
        if R > 0.75:
            lam *= 0.5
            if lam < lc:
                lam = 0.0
        elif R < 0.25:
            t = float(d @ v)
            nu = min(max((Sd - S) / (t if abs(t) > DBL_EPSILON else 1.0) + 2.0, 2.0), 10.0)
            if lam == 0.0:
                _, dinv = _sym_solve(A.copy(), v)
                lam = lc = 1.0 / max(DBL_EPSILON, float(np.abs(dinv).max()))
                nu *= 0.5
            lam *= nu
        if Sd < S:
            h = hd
            A, v, S, rmax = full(h)
        it += 1
        if float(np.abs(d).max()) < FLT_EPSILON or rmax < FLT_EPSILON:
            break
    info["S1"] = S
    info["iters"] = it
    return h, info


def lm_band(S, Sd, n, L):
    """Relative uncertainty of S - S_d.  Each residual carries an absolute rounding error of about 2 eps L (L: the largest pixel
    coordinate; the division and the subtraction of coordinates of that size), so a term r^2 moves by 4 eps L |r| and a sum of n
    of them by at most 4 eps L sqrt(n S) (Cauchy-Schwarz); the summation itself adds (n / 64 + 16) eps S for either order (64
    strided partial sums and a butterfly, or numpy's pairwise blocks).  Both sums carry it independently."""
    err = sum(4.0 * DBL_EPSILON * L * math.sqrt(n * s) + (n / 64.0 + 16.0) * DBL_EPSILON * s for s in (S, Sd))
    diff = abs(S - Sd)
    return err / diff if diff > 0 else math.inf


LM_SLACK_CAP = 1e-3  # pixels: above this the refinement is ill-posed and only the invariants are checked


def lm_ambiguous(info, n, L, pin):
    """(index i of the first LM iteration whose branch -- R against 0.25 / 0.75, S_d against S -- lies inside the band, or None;
    the slack in pixels that goes with it).  On noisy input the loop always ends this way: the step before the last is a few
    FLT_EPSILON long and the last far shorter, and neither changes S by more than its rounding error, so rounding decides whether
    they are accepted and how lambda moves.  From iteration i on the loop can do nothing but take or leave steps of the size it
    has reached: the gradient v no longer decreases measurably, every later step solves (A + lambda D) d = v for a v of that size,
    and the steps of this loop shrink at least geometrically from there (quadratically in every trace printed by
    tests/homography_cases.py).  So the results of two correct evaluations differ by at most the steps still to come, bounded
    by twice the step d_i for each remaining iteration: slack = 2 (iterations run - i) * (largest transfer difference between
    h_i and h_i - d_i over the inliers and the corners).  The comparison of H_out gets that slack on top of its tolerance; a
    slack above LM_SLACK_CAP marks the pair ambiguous."""
    its = len(info["R"])
    for i, (R, S, Sd) in enumerate(zip(info["R"], info["S"], info["Sd"])):
        rel = lm_band(S, Sd, n, L)
        if not np.isfinite(R) or rel >= 1.0 or abs(R - 0.25) <= rel * abs(R) or abs(R - 0.75) <= rel * abs(R):
            ha, hb = info["h"][i], info["h"][i] - info["d"][i]
            step = max_transfer_diff(np.append(ha, 1.0).reshape(3, 3), np.append(hb, 1.0).reshape(3, 3), pin)
            return i, 2.0 * (its - i) * step
    return None, 0.0


def hypotheses(pts, seed, max_iters, route="qr"):
    """Every iteration's (idx or None, H or None, kappa)."""
    pts = np.asarray(pts, np.float32)
    out = []
    for k in range(max_iters):
        idx = draw_sample(seed, k, pts)
        if idx is None:
            out.append((None, None, math.inf))
        else:
            H, kap = solve4(pts[idx], route)
            out.append((idx, H, kap))
    return out


def estimate(pts, n=None, threshold=3.0, confidence=0.995, max_iters=2000, seed=0, flags=0, route="qr", hyps=None):
    """One pair, stage by stage.  pts [N,4] float32; n: rows used (None: all).  Returns a dict: table / table_lo / table_hi
    [max_iters] (counts with every ambiguous correspondence out / in), kappa [max_iters], best, best_k, iters, H_model, mask,
    mask_amb, ratio (err / t^2 under H_model), H_refit, H_out, lm (info or None), ambiguous (None, or a string naming the
    correspondence or the iteration that makes the pair so)."""
    pts = np.asarray(pts, np.float32)
    N = pts.shape[0]
    n = N if n is None else min(max(int(n), 0), N)
    p = pts[:n]
    t = threshold if threshold > 0 else 3.0
    allp, norefine = bool(flags & ALL_POINTS), bool(flags & NO_REFINE)
    sampled = n > 4 and not allp
    out = {"n": n, "table": np.full(max_iters, NO_SAMPLE, np.int64), "best": 0, "best_k": -1, "iters": 0, "H_model": np.zeros((3, 3)),
           "mask": np.zeros(N, np.uint8), "mask_amb": np.zeros(N, bool), "H_refit": np.zeros((3, 3)), "H_out": np.zeros((3, 3)), "lm": None,
           "ambiguous": None, "kappa": np.full(max_iters, math.inf), "kappa_model": 1.0, "flags": flags, "lm_slack": 0.0, "kappa_refit": 1.0}
    out["table_lo"], out["table_hi"] = out["table"].copy(), out["table"].copy()
    Hm, kap_m = None, 1.0
    if sampled:
        hyps = hypotheses(p, seed, max_iters, route) if hyps is None else hyps
        out["hyps"] = hyps
        amb_of = {}
        for k, (idx, H, kap) in enumerate(hyps):
            out["kappa"][k] = kap
            if idx is None:
                continue
            if H is None:
                out["table"][k] = out["table_lo"][k] = out["table_hi"][k] = NO_MODEL
                continue
            sure, amb, ratio = classify(H, p, t, kap)
            out["table"][k] = int((ratio <= 1.0).sum())
            out["table_lo"][k] = int(sure.sum())
            out["table_hi"][k] = int(sure.sum() + amb.sum())
            if amb.any():
                amb_of[k] = int(np.flatnonzero(amb)[0])
        best, bk, iters = select(out["table"], n, confidence, max_iters)
        # a band correspondence matters only when it can change what the rule does: try the two extreme tables
        for tab in (out["table_lo"], out["table_hi"]):
            if select(tab, n, confidence, max_iters) != (int(tab[bk]) if bk >= 0 else 0, bk, iters) and out["ambiguous"] is None:
                ks = [k for k in amb_of if k <= max(iters, bk)]
                out["ambiguous"] = f"correspondence {amb_of[ks[0]]} of iteration {ks[0]} lies in the band" if ks else "band"
        out["best"], out["best_k"], out["iters"] = best, bk, iters
        if bk >= 0:
            Hm, kap_m = hyps[bk][1], hyps[bk][2]
    elif n == 4:
        Hm, kap_m = solve4(p, route)
        out["best"] = 4 if Hm is not None else 0
    elif n > 4 and allp:
        out["best"] = n
    if out["best"] == 0:
        return out
    out["kappa_model"] = kap_m
    if n == 4 or allp:
        out["mask"][:n] = 1
    else:
        sure, amb, ratio = classify(Hm, p, t, kap_m)
        out["mask"][:n] = ratio <= 1.0
        out["mask_amb"][:n] = amb
        out["ratio"] = ratio
        if amb.any() and out["ambiguous"] is None:
            out["ambiguous"] = f"correspondence {int(np.flatnonzero(amb)[0])} of the winner lies in the band"
    if Hm is not None:
        out["H_model"] = Hm
    out["H_refit"] = out["H_out"] = out["H_model"]
    if n > 4:
        pin = p[out["mask"][:n] > 0]
        Hr, out["kappa_refit"] = refit(pin, True)
        if allp and Hr is None:
            out["best"] = 0
            out["mask"][:] = 0
            return out
        if Hr is not None:
            out["H_refit"] = Hr
            if allp:
                out["H_model"] = Hr
        out["H_out"] = out["H_refit"]
        if not norefine:
            h, info = lm_refine(out["H_refit"].reshape(-1)[:8], pin)
            out["lm"] = info
            out["H_out"] = np.append(h, 1.0).reshape(3, 3)
            ai, slack = lm_ambiguous(info, len(pin), max(1.0, float(np.abs(pin).max())), pin)
            out["lm_slack"] = slack
            if ai is not None and slack > LM_SLACK_CAP and out["ambiguous"] is None:
                out["ambiguous"] = f"LM iteration {ai}: the gain ratio lies in the band and the step still moves points by {slack:.1e} px"
    return out


def transfer_dist(H, pts):
    """evaluate_frontend.getInliers' distances |H x1 - x2| in fp64."""
    pts = np.asarray(pts, np.float64)
    xw, yw, _ = transfer(H, pts)
    return np.sqrt((xw - pts[:, 2]) ** 2 + (yw - pts[:, 3]) ** 2)


def corner_mean_dist(He, Hg, height, width):
    c = np.array([[0, 0, 1], [0, height - 1, 1], [width - 1, 0, 1], [width - 1, height - 1, 1]], np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = c @ np.asarray(Hg, np.float64).reshape(3, 3).T
        b = c @ np.asarray(He, np.float64).reshape(3, 3).T
        return float(np.mean(np.linalg.norm(a[:, :2] / a[:, 2:] - b[:, :2] / b[:, 2:], axis=1)))


def max_transfer_diff(Ha, Hb, pts, height=240, width=320, corners=True):
    """The yardstick distance between two homographies: the largest difference of the transferred points over the given
    correspondences and the four image corners, in pixels.  corners=False leaves the corners out: a minimal sample's H is
    compared where it is supported (its inliers); a hypothesis fitted to outliers may send a corner to infinity."""
    cs = np.array([[0, 0, 0, 0], [0, height - 1, 0, 0], [width - 1, 0, 0, 0], [width - 1, height - 1, 0, 0]], np.float64)
    q = np.concatenate([np.asarray(pts, np.float64), cs]) if corners else np.asarray(pts, np.float64)
    xa, ya, _ = transfer(Ha, q)
    xb, yb, _ = transfer(Hb, q)
    d = np.hypot(xa - xb, ya - yb)
    d = d[np.isfinite(d)]
    return float(d.max()) if len(d) else 0.0


# ---- the 50-digit twin -----------------------------------------------------------------------------------------------------
def _mp():
    import mpmath

    mpmath.mp.dps = 50
    return mpmath


def _mp_norm(p, mp):
    n = len(p)
    c = [sum(mp.mpf(float(r[a])) for r in p) / n for a in range(4)]
    s = [n / sum(abs(mp.mpf(float(r[a])) - c[a]) for r in p) for a in range(4)]
    return c, s


def _mp_system(p, c, s, mp):
    rows = []
    for r in p:
        X, Y, x, y = [(mp.mpf(float(r[a])) - c[a]) * s[a] for a in range(4)]
        rows.append([X, Y, 1, 0, 0, 0, -x * X, -x * Y, -x])
        rows.append([0, 0, 0, X, Y, 1, -y * X, -y * Y, -y])
    return mp.matrix(rows)


def _mp_denorm(h0, c, s, mp):
    H0 = mp.matrix(3, 3)
    for i in range(9):
        H0[i // 3, i % 3] = h0[i]
    Ts = mp.matrix([[s[0], 0, -c[0] * s[0]], [0, s[1], -c[1] * s[1]], [0, 0, 1]])
    Tdi = mp.matrix([[1 / s[2], 0, c[2]], [0, 1 / s[3], c[3]], [0, 0, 1]])
    H = Tdi * H0 * Ts
    return np.array([[float(H[i, j] / H[2, 2]) for j in range(3)] for i in range(3)])


def mp_solve4(p4):
    """The 4-point solve at 50 digits: the null vector by the cofactors of the 8x9 system (exact up to the working precision)."""
    mp = _mp()
    p4 = np.asarray(p4, np.float32)
    c, s = _mp_norm(p4, mp)
    A = _mp_system(p4, c, s, mp)
    h0 = []
    for j in range(9):
        cols = [k for k in range(9) if k != j]
        M = mp.matrix(8, 8)
        for r in range(8):
            for q, k in enumerate(cols):
                M[r, q] = A[r, k]
        h0.append((-1) ** j * mp.det(M))
    return _mp_denorm(h0, c, s, mp)


def mp_refit(pin):
    """The refit at 50 digits: smallest eigenvector of L^T L by mpmath's symmetric eigen solver."""
    mp = _mp()
    pin = np.asarray(pin, np.float32)
    c, s = _mp_norm(pin, mp)
    A = _mp_system(pin, c, s, mp)
    E, Q = mp.eigsy(A.T * A)
    m = min(range(9), key=lambda i: E[i])
    return _mp_denorm([Q[i, m] for i in range(9)], c, s, mp)


def mp_lm_eval(h, pin):
    """One residual / Jacobian evaluation at 50 digits -> (J^T J [8,8], J^T r [8], S) as floats."""
    mp = _mp()
    hh = [mp.mpf(float(v)) for v in h]
    A = mp.matrix(8, 8)
    v = mp.matrix(8, 1)
    S = mp.mpf(0)
    for r in np.asarray(pin, np.float32):
        X, Y, x, y = [mp.mpf(float(a)) for a in r]
        w = hh[6] * X + hh[7] * Y + 1
        wi = 1 / w if abs(w) > DBL_EPSILON else mp.mpf(0)
        xi = (hh[0] * X + hh[1] * Y + hh[2]) * wi
        yi = (hh[3] * X + hh[4] * Y + hh[5]) * wi
        rx, ry = xi - x, yi - y
        Jx = [X * wi, Y * wi, wi, 0, 0, 0, -X * wi * xi, -Y * wi * xi]
        Jy = [0, 0, 0, X * wi, Y * wi, wi, -X * wi * yi, -Y * wi * yi]
        for i in range(8):
            v[i] += Jx[i] * rx + Jy[i] * ry
            for j in range(8):
                A[i, j] += Jx[i] * Jx[j] + Jy[i] * Jy[j]
        S += rx * rx + ry * ry
    return (np.array([[float(A[i, j]) for j in range(8)] for i in range(8)]), np.array([float(v[i]) for i in range(8)]), float(S))
