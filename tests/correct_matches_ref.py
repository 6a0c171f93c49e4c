"""fp64 restatement of dfepe_correct_matches (include/dfepe.h): the Hartley-Sturm optimal correction of a correspondence onto an
epipolar geometry, step by step with plain 3x3 matrices and numpy.roots, plus the same steps at 50 digits in mpmath
(correct_one_mp: the truth the fp64 restatement is measured against), an independent route to the same minimum that does not use
the polynomial (a scan over the pencil of epipolar lines: a one-sided witness), and the reference's own lines around the
cv2.correctMatches call (deepFEPE/dsac_tools/utils_misc.py:163-230) with this restatement in cv2's place.

Convention (OpenCV's): correct(F, p, q) returns (p', q') with q'^T F p' = 0 and |p - p'|^2 + |q - q'|^2 minimal.

Roots.  The sextic is binary in (tau, ups), t = tau / ups.  numpy.roots divides by the leading coefficient, which is of order f1^4
in t: with an epipole close to infinity (f1 -> 0) the companion matrix has entries of 1 / f1^4 and the roots it returns are
noise (a pure translation with tz = 1e-12 came out 7e3 px from the minimum).  Taking |t| <= 1 from numpy.roots of the
coefficients and |t| >= 1 from numpy.roots of the reversed ones is not enough by itself: each call still divides by its own
leading coefficient, and at tz = 1e-15 and 1e-12 one point in 64 lost every finite root that way (measured).  So numpy.roots
is given the form in a ROTATED variable, (tau, ups) = (c sigma - s, s sigma + c), with the angle among eight for which the
leading coefficient -- the form's value at (c, s) -- is largest: a sextic form that is not zero cannot vanish in seven
directions, so no companion matrix is ever scaled by a vanishing number.  Each real root then goes to its chart as the contract
describes them, t = tau / ups for |tau| <= |ups| and u = ups / tau otherwise, and is polished there by Newton steps in
numpy.longdouble on that chart's coefficients (the reversed ones for u).  Candidates are carried homogeneously as (tau, ups),
ups = 0 for t = infinity."""
import numpy as np

REAL_TOL = 1e-9      # a root t of numpy.roots is real when |imag| <= REAL_TOL * max(1, |t|)
NEAR_TIE = 1e-6      # two lowest candidate costs closer than this (relative): the position may be left out of a comparison
POS_TOL = 1e-6       # px: two candidates whose corrected points agree to this in every coordinate are the same line
MP_DPS = 50


def epipoles(F):
    """e1 with F e1 = 0 and e2 with e2^T F = 0: the largest cross product of two rows / two columns."""
    def null(u, v, w):
        c = [np.cross(u, v), np.cross(u, w), np.cross(v, w)]
        return c[int(np.argmax([x @ x for x in c]))]
    return null(F[0], F[1], F[2]), null(F[:, 0], F[:, 1], F[:, 2])


def sextic(a, b, c, d, f1, f2):
    """Coefficients, highest power first, of t ((a t + b)^2 + f2^2 (c t + d)^2)^2 - (a d - b c) (1 + f1^2 t^2)^2 (a t + b) (c t + d)."""
    P = np.polyadd(np.polymul([a, b], [a, b]), f2 * f2 * np.polymul([c, d], [c, d]))
    Q = np.polymul([f1 * f1, 0.0, 1.0], [f1 * f1, 0.0, 1.0])
    g = np.polysub(np.polymul([1.0, 0.0], np.polymul(P, P)), (a * d - b * c) * np.polymul(Q, np.polymul([a, b], [c, d])))
    return np.r_[np.zeros(7 - len(g)), g]


def cost(t, a, b, c, d, f1, f2):
    if np.isinf(t):
        return 1.0 / (f1 * f1) + c * c / (a * a + f2 * f2 * c * c)
    return t * t / (1.0 + f1 * f1 * t * t) + (c * t + d) ** 2 / ((a * t + b) ** 2 + f2 * f2 * (c * t + d) ** 2)


def cost_h(tau, ups, a, b, c, d, f1, f2):
    """The cost of the pair of lines of the candidate (tau, ups), t = tau / ups."""
    A, C = a * tau + b * ups, c * tau + d * ups
    return tau * tau / (ups * ups + f1 * f1 * tau * tau) + C * C / (A * A + f2 * f2 * C * C)


def polish_longdouble(g, t):
    """Newton steps on a root of the polynomial g (highest power first) in numpy.longdouble."""
    gl = np.asarray(g, np.longdouble)
    dl = np.polyder(gl)
    x = np.longdouble(t)
    for _ in range(6):
        x = x - np.polyval(gl, x) / np.polyval(dl, x)
    return float(x)


def real_roots(g, polish=polish_longdouble):
    """The real roots of the binary sextic sum_k g[6 - k] tau^k ups^(6 - k) (g: highest power of t = tau / ups first, largest
    magnitude 1), each in its chart: -> (ts ascending with |t| <= 1, us ascending with |u| < 1, u = ups / tau).
    numpy.roots sees the form in a rotated variable, and each real root is then polished on its own chart's coefficients (g for
    t, g reversed for u); a polished root that is not finite (Newton on a multiple root can divide 0 by 0) keeps its unpolished
    value."""
    form = lambda c, s: sum(g[6 - k] * c ** k * s ** (6 - k) for k in range(7))
    c, s = max(((np.cos(k * np.pi / 8), np.sin(k * np.pi / 8)) for k in range(8)), key=lambda cs: abs(form(*cs)))
    h = np.zeros(7)
    for k in range(7):
        term = ((np.poly1d([c, -s]) ** k) * (np.poly1d([s, c]) ** (6 - k))).coeffs   # tau^k ups^(6 - k) in sigma
        h[7 - len(term):] += g[6 - k] * term
    ts, us = [], []
    with np.errstate(all="ignore"):
        r = np.roots(h)
        for x in r.real[np.abs(r.imag) <= REAL_TOL * np.maximum(1.0, np.abs(r))]:
            tau, ups = c * x - s, s * x + c
            if abs(tau) <= abs(ups):
                t = tau / ups
                pol = polish(g, t) if polish else t
                ts.append(pol if np.isfinite(pol) else t)
            else:
                u = ups / tau
                pol = polish(g[::-1], u) if polish else u
                us.append(pol if np.isfinite(pol) else u)
    return np.sort(np.array(ts, np.float64)), np.sort(np.array(us, np.float64))


def _frame(F, p, q):
    """Steps 1 and 2 of the contract: (a, b, c, d, f1, f2), (p, R1^T), (q, R2^T) -- or None for a point on an epipole."""
    e1, e2 = epipoles(F)
    T1 = np.array([[1, 0, p[0]], [0, 1, p[1]], [0, 0, 1.0]])
    T2 = np.array([[1, 0, q[0]], [0, 1, q[1]], [0, 0, 1.0]])
    e1 = np.array([e1[0] - p[0] * e1[2], e1[1] - p[1] * e1[2], e1[2]])
    e2 = np.array([e2[0] - q[0] * e2[2], e2[1] - q[1] * e2[2], e2[2]])
    n1, n2 = e1[0] ** 2 + e1[1] ** 2, e2[0] ** 2 + e2[1] ** 2
    if not (n1 > 0 and n2 > 0):
        return None
    e1, e2 = e1 / np.sqrt(n1), e2 / np.sqrt(n2)
    R1 = np.array([[e1[0], e1[1], 0], [-e1[1], e1[0], 0], [0, 0, 1.0]])
    R2 = np.array([[e2[0], e2[1], 0], [-e2[1], e2[0], 0], [0, 0, 1.0]])
    G = R2 @ (T2.T @ F @ T1) @ R1.T
    return (G[1, 1], G[1, 2], G[2, 1], G[2, 2], e1[2], e2[2]), (p, R1.T), (q, R2.T)


def _points(tau, ups, abcdff, B1, B2):
    """The corrected points [4] (p', q') of the candidate (tau, ups): T R^T x, with the translation added AFTER the division, so
    that a coordinate is rounded once at its own magnitude and not twice at |p| times the third coordinate's; evaluated in
    numpy.longdouble and rounded to fp64 at the end, so that the output's own rounding is all that this step adds."""
    L = np.longdouble
    a, b, c, d, f1, f2 = (L(x) for x in abcdff)
    tau, ups = L(tau), L(ups)
    A, C = a * tau + b * ups, c * tau + d * ups
    x1 = B1[1].astype(L) @ np.array([tau * tau * f1, tau * ups, tau * tau * f1 * f1 + ups * ups])
    x2 = B2[1].astype(L) @ np.array([f2 * C * C, -A * C, f2 * f2 * C * C + A * A])
    return np.r_[B1[0].astype(L) + x1[:2] / x1[2], B2[0].astype(L) + x2[:2] / x2[2]].astype(np.float64)


def correct_one(F, p, q, polish=polish_longdouble):
    """One correspondence.  Returns dict(p, q: the corrected points (NaN on a degenerate lane), cost, roots: the finite real roots
    t = tau / ups of both charts, ascending, cands [n,2]: every candidate (tau, ups), the last one t = infinity = (1, 0), costs: the
    candidates' costs in ascending order, near_tie: a candidate that is another pair of lines than the winner (its corrected points
    differ from the winner's by more than POS_TOL in some coordinate) costs within NEAR_TIE relative of it).  polish: a function
    (coefficients, root) -> root applied to every real root in its chart, or None for numpy.roots' own values."""
    F = np.asarray(F, np.float64)
    with np.errstate(all="ignore"):
        F = F / np.abs(F).max()
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    nan = dict(p=np.full(2, np.nan), q=np.full(2, np.nan), cost=np.nan, roots=np.zeros(0), cands=np.zeros((0, 2)), costs=np.zeros(0),
               near_tie=False)
    if not np.isfinite(F).all():
        return nan
    fr = _frame(F, p, q)
    if fr is None:
        return nan
    abcdff, B1, B2 = fr
    g = sextic(*abcdff)
    if not (np.abs(g).max() > 0):
        return nan
    g = g / np.abs(g).max()
    ts, us = real_roots(g, polish)                             # |t| <= 1 and |u| < 1, u = 1 / t
    us = us[us != 0.0]                                         # u = 0 is t = infinity, listed below
    cands = np.array([(t, 1.0) for t in ts] + [(1.0, u) for u in us] + [(1.0, 0.0)])
    with np.errstate(all="ignore"):
        costs = np.array([cost_h(tau, ups, *abcdff) for tau, ups in cands])
        costs[np.isnan(costs)] = np.inf
        k = int(np.argmin(costs))
        pts = np.array([_points(tau, ups, abcdff, B1, B2) for tau, ups in cands])
        tie = bool((np.isfinite(costs) & (costs - costs[k] <= NEAR_TIE * costs) & (np.abs(pts - pts[k]).max(1) > POS_TOL)).any())
    out = dict(p=pts[k, :2], q=pts[k, 2:], cost=costs[k], roots=np.sort(np.r_[ts, 1.0 / us]), cands=cands, costs=np.sort(costs),
               near_tie=tie)
    if not (np.isfinite(pts[k]).all() and np.isfinite(out["cost"])):
        return nan
    return out


def correct_matches(F, P, Q, polish=polish_longdouble):
    """P, Q [M,2] under one F -> dict(p [M,2], q [M,2], cost [M], near_tie [M] bool, roots: list of M arrays)."""
    res = [correct_one(F, p, q, polish) for p, q in zip(np.asarray(P), np.asarray(Q))]
    return dict(p=np.array([r["p"] for r in res]), q=np.array([r["q"] for r in res]), cost=np.array([r["cost"] for r in res]),
                near_tie=np.array([r["near_tie"] for r in res], bool), roots=[r["roots"] for r in res])


def correct_one_mp(F, p, q):
    """The same steps, the epipole rule included, at MP_DPS digits with mpmath.polyroots on both charts.  F, p, q are taken as the
    exact values of their fp64 / fp32 numbers.  Returns dict(p [2], q [2], cost: fp64 roundings of the result (NaN on a degenerate
    lane), roots_t, roots_u: every complex root of the two charts' polynomials at full precision (for multiplicity counts))."""
    import mpmath as mp
    with mp.workdps(MP_DPS):
        nan = dict(p=np.full(2, np.nan), q=np.full(2, np.nan), cost=np.nan, roots_t=[], roots_u=[])
        F = [[mp.mpf(float(x)) for x in row] for row in np.asarray(F, np.float64)]
        m = max(abs(x) for row in F for x in row)
        if not (m > 0) or not all(mp.isfinite(x) for row in F for x in row):
            return nan
        F = [[x / m for x in row] for row in F]
        px, py, qx, qy = (mp.mpf(float(x)) for x in (p[0], p[1], q[0], q[1]))
        cross = lambda u, v: [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]

        def null(u, v, w):
            c = [cross(u, v), cross(u, w), cross(v, w)]
            n = [sum(x * x for x in y) for y in c]
            return c[0] if n[0] >= n[1] and n[0] >= n[2] else (c[1] if n[1] >= n[2] else c[2])
        e1 = null(F[0], F[1], F[2])
        e2 = null(*[[F[0][j], F[1][j], F[2][j]] for j in range(3)])
        ex1, ey1, ex2, ey2 = e1[0] - px * e1[2], e1[1] - py * e1[2], e2[0] - qx * e2[2], e2[1] - qy * e2[2]
        n1, n2 = ex1 * ex1 + ey1 * ey1, ex2 * ex2 + ey2 * ey2
        if not (n1 > 0 and n2 > 0):
            return nan
        r1, r2 = 1 / mp.sqrt(n1), 1 / mp.sqrt(n2)
        ex1, ey1, ex2, ey2, f1, f2 = ex1 * r1, ey1 * r1, ex2 * r2, ey2 * r2, e1[2] * r1, e2[2] * r2
        # F' = T2^T F T1, G = R2 F' R1^T: its lower right 2x2
        Fp = [[F[0][0], F[0][1], F[0][0] * px + F[0][1] * py + F[0][2]], [F[1][0], F[1][1], F[1][0] * px + F[1][1] * py + F[1][2]]]
        Fp.append([qx * Fp[0][j] + qy * Fp[1][j] + (F[2][j] if j < 2 else F[2][0] * px + F[2][1] * py + F[2][2]) for j in range(3)])
        H = [[ex1 * Fp[i][0] + ey1 * Fp[i][1], -ey1 * Fp[i][0] + ex1 * Fp[i][1], Fp[i][2]] for i in range(3)]   # F' R1^T
        a, b = -ey2 * H[0][1] + ex2 * H[1][1], -ey2 * H[0][2] + ex2 * H[1][2]
        c, d = H[2][1], H[2][2]
        # the sextic, lowest power first
        f1s, f2s, det = f1 * f1, f2 * f2, a * d - b * c
        p0, p1, p2 = b * b + f2s * d * d, 2 * (a * b + f2s * c * d), a * a + f2s * c * c
        s0, s1, s2 = b * d, a * d + b * c, a * c
        g = [-det * s0, p0 * p0 - det * s1, 2 * p0 * p1 - det * (s2 + 2 * f1s * s0), 2 * p0 * p2 + p1 * p1 - det * 2 * f1s * s1,
             2 * p1 * p2 - det * (2 * f1s * s2 + f1s * f1s * s0), p2 * p2 - det * f1s * f1s * s1, -det * f1s * f1s * s2]
        gm = max(abs(x) for x in g)
        if not (gm > 0):
            return nan
        g = [x / gm for x in g]

        def roots_of(hi_first):
            """Every complex root; exact zeros at either end are split off (roots at infinity, which no chart wants, and at 0).
            numpy.roots of the rounded coefficients only STARTS the iteration: polyroots returns what it has converged to."""
            while hi_first and hi_first[0] == 0:
                hi_first = hi_first[1:]
            zeros = []
            while hi_first and hi_first[-1] == 0:
                hi_first, zeros = hi_first[:-1], zeros + [mp.mpc(0)]
            if len(hi_first) < 2:
                return zeros
            with np.errstate(all="ignore"):
                init = np.roots([float(x) for x in hi_first])
            init = [mp.mpc(complex(z)) * (1 + mp.mpf(k + 1) / 10 ** 9) for k, z in enumerate(init)] \
                if len(init) == len(hi_first) - 1 and np.isfinite(init).all() else None
            for start, steps, extra in ((init, 100, 200), (None, 500, 1000), (None, 4000, 8000)):
                try:
                    return zeros + mp.polyroots(hi_first, maxsteps=steps, extraprec=extra, roots_init=start)
                except mp.libmp.NoConvergence:
                    continue
            raise RuntimeError("mpmath.polyroots did not converge")
        rt, ru = roots_of(g[::-1]), roots_of(g)
        real = lambda r: [z.real for z in r if abs(z.imag) <= mp.mpf(10) ** -20 * max(1, abs(z)) and abs(z) <= 1]
        cands = [(t, mp.mpf(1)) for t in real(rt)] + [(mp.mpf(1), u) for u in real(ru)] + [(mp.mpf(1), mp.mpf(0))]

        def s_of(tau, ups):
            A, C = a * tau + b * ups, c * tau + d * ups
            n, k = ups * ups + f1s * tau * tau, A * A + f2s * C * C
            return tau * tau / n + C * C / k if n != 0 and k != 0 else mp.inf
        costs = [s_of(*tu) for tu in cands]
        k = min(range(len(cands)), key=lambda i: costs[i])
        tau, ups = cands[k]
        A, C = a * tau + b * ups, c * tau + d * ups
        X1, Y1, W1 = tau * tau * f1, tau * ups, tau * tau * f1s + ups * ups
        X2, Y2, W2 = f2 * C * C, -A * C, f2s * C * C + A * A
        if W1 == 0 or W2 == 0 or not mp.isfinite(costs[k]):
            return nan
        out = [px + (ex1 * X1 - ey1 * Y1) / W1, py + (ey1 * X1 + ex1 * Y1) / W1, qx + (ex2 * X2 - ey2 * Y2) / W2,
               qy + (ey2 * X2 + ex2 * Y2) / W2]
        return dict(p=np.array([float(out[0]), float(out[1])]), q=np.array([float(out[2]), float(out[3])]), cost=float(costs[k]),
                    roots_t=rt, roots_u=ru)


def line_distance(F, P, Q):
    """Distance of q to the epipolar line F p [M], in pixels.  Evaluated in numpy.longdouble: next to the first image's epipole
    F p cancels (at 0.04 px from an epipole at 874 px by a factor of 2e4), and with q 800 px from its own epipole the fp64
    evaluation of q^T F p alone is 5e-9 px of noise -- more than the 1e-9 px that the tests hold this distance to."""
    L = np.longdouble
    l = np.c_[P, np.ones(len(P))].astype(L) @ np.asarray(F, np.float64).astype(L).T
    return (np.abs((l * np.c_[Q, np.ones(len(Q))].astype(L)).sum(1)) / np.hypot(l[:, 0], l[:, 1])).astype(np.float64)


def pencil_min_cost(F, P, Q, scan=8192, iters=80):
    """An upper bound of the same minimum without the polynomial: every pair of corresponding epipolar lines is l1 = e1 x w,
    l2 = F w for a point w = cos th u + sin th v, th in [0, pi), where (u, v) is an orthonormal basis of the complement of the
    normalised e1 (so w is never e1, and the pencil is the one through e1 wherever e1 lies, at infinity included); the cost of a
    pair of lines is dist(p, l1)^2 + dist(q, l2)^2.  A dense scan over th, then a golden-section search in the two cells around the
    best sample.  Returns a cost [M] that some pair of corresponding lines attains.

    ONE-SIDED: the scan can miss the basin of the global minimum (at 4096 samples and rotations of ~1 rad it returned 1.03e6 px^2
    where the minimum is 5.47e5), so nothing may be ABOVE what it returns, and being below it proves nothing wrong."""
    F = np.asarray(F, np.float64)
    F = F / np.abs(F).max()
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    e1, _ = epipoles(F)
    e1 = e1 / np.sqrt(e1 @ e1)
    u, v = np.linalg.svd(e1[None])[2][1:]
    ph, qh = np.c_[P, np.ones(len(P))], np.c_[Q, np.ones(len(Q))]

    def cost_of(th, a, b):  # th [m] or [m, n] angles, a, b [m,3] the points -> cost, shaped as th
        w = np.cos(th)[..., None] * u + np.sin(th)[..., None] * v
        l1 = np.cross(e1, w)
        l2 = w @ F.T
        sh = (slice(None),) + (None,) * (th.ndim - 1)
        with np.errstate(all="ignore"):
            d1 = (l1 * a[sh]).sum(-1) ** 2 / (l1[..., 0] ** 2 + l1[..., 1] ** 2)
            d2 = (l2 * b[sh]).sum(-1) ** 2 / (l2[..., 0] ** 2 + l2[..., 1] ** 2)
        s = d1 + d2
        return np.where(np.isnan(s), np.inf, s)   # the line at infinity is no candidate

    h = np.pi / scan
    best = np.empty(len(P))
    for s in range(0, len(P), 64):  # chunks keep the scan's table small
        sl = slice(s, min(s + 64, len(P)))
        f = lambda th: cost_of(th, ph[sl], qh[sl])
        th = np.broadcast_to(np.arange(scan) * h, (len(ph[sl]), scan))
        k = np.argmin(f(th), 1)
        lo, hi = (k - 1) * h, (k + 1) * h
        gr = (np.sqrt(5.0) - 1) / 2
        x1, x2 = hi - gr * (hi - lo), lo + gr * (hi - lo)
        f1, f2 = f(x1), f(x2)
        for _ in range(iters):
            left = f1 < f2
            hi = np.where(left, x2, hi)
            lo = np.where(left, lo, x1)
            nx1, nx2 = hi - gr * (hi - lo), lo + gr * (hi - lo)
            x1, x2 = nx1, nx2
            f1, f2 = f(x1), f(x2)
        best[sl] = np.minimum(f1, f2)
    return best


def grid(im_shape):
    """utils_misc.get_virt_x1x2_grid (:163-171): 10 x 10 positions, the same in both images, float32."""
    xx, yy = np.meshgrid(np.arange(0, 1, 0.1), np.arange(0, 1, 0.1))
    g = np.float32(np.vstack((im_shape[1] * xx.flatten(), im_shape[0] * yy.flatten())).T)
    return g, g.copy()


def virt_through_the_reference_lines(F_gt, K, pts1_virt_b, pts2_virt_b):
    """utils_misc.get_virt_x1x2_np (:173-199) with the restatement for cv2.correctMatches: the call's swapped arguments, NaN to
    0, homogeneous, inv(K), and pts2_virt_normalized computed from pts1_virt.  Everything stays fp64 except the rounding of the
    corrected points to float32 that cv2 does for float32 input."""
    r = correct_matches(F_gt, pts2_virt_b, pts1_virt_b)   # correctMatches(F_gt, pts2_virt_b, pts1_virt_b)
    pts1_virt, pts2_virt = np.float32(r["p"]), np.float32(r["q"])
    pts1_virt[np.isnan(pts1_virt)] = 0.0
    pts2_virt[np.isnan(pts2_virt)] = 0.0
    pts1_virt = np.hstack((pts1_virt, np.ones((len(pts1_virt), 1), np.float32)))
    pts2_virt = np.hstack((pts2_virt, np.ones((len(pts2_virt), 1), np.float32)))
    pts1_virt_normalized = (np.linalg.inv(K) @ pts1_virt.T).T
    pts2_virt_normalized = (np.linalg.inv(K) @ pts1_virt.T).T
    return pts1_virt_normalized, pts2_virt_normalized, pts1_virt, pts2_virt
