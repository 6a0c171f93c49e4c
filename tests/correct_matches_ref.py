"""fp64 restatement of dfepe_correct_matches (include/dfepe.h): the Hartley-Sturm optimal correction of a correspondence onto an
epipolar geometry, step by step with plain 3x3 matrices and numpy.roots, plus an independent route to the same minimum that
does not use the polynomial (a scan over the pencil of epipolar lines), and the reference's own lines around the
cv2.correctMatches call (deepFEPE/dsac_tools/utils_misc.py:163-230) with this restatement in cv2's place.

Convention (OpenCV's): correct(F, p, q) returns (p', q') with q'^T F p' = 0 and |p - p'|^2 + |q - q'|^2 minimal."""
import numpy as np

REAL_TOL = 1e-9      # a root t of numpy.roots is real when |imag| <= REAL_TOL * max(1, |t|)
NEAR_TIE = 1e-6      # two lowest candidate costs closer than this (relative): the position may be left out of a comparison


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


def correct_one(F, p, q, polish=None):
    """One correspondence.  Returns dict(p, q: the corrected points (NaN on a degenerate lane), cost, roots: the real roots of
    numpy.roots, costs: the candidates' costs in ascending order).  polish: a function (coefficients, root) -> root applied to
    every real root before it is used (the tests polish in numpy.longdouble to measure the restatement's own error)."""
    F = np.asarray(F, np.float64)
    F = F / np.abs(F).max()
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    nan = dict(p=np.full(2, np.nan), q=np.full(2, np.nan), cost=np.nan, roots=np.zeros(0), costs=np.zeros(0))
    e1, e2 = epipoles(F)
    T1 = np.array([[1, 0, p[0]], [0, 1, p[1]], [0, 0, 1.0]])
    T2 = np.array([[1, 0, q[0]], [0, 1, q[1]], [0, 0, 1.0]])
    e1 = np.array([e1[0] - p[0] * e1[2], e1[1] - p[1] * e1[2], e1[2]])
    e2 = np.array([e2[0] - q[0] * e2[2], e2[1] - q[1] * e2[2], e2[2]])
    n1, n2 = e1[0] ** 2 + e1[1] ** 2, e2[0] ** 2 + e2[1] ** 2
    if not (n1 > 0 and n2 > 0):
        return nan
    e1, e2 = e1 / np.sqrt(n1), e2 / np.sqrt(n2)
    R1 = np.array([[e1[0], e1[1], 0], [-e1[1], e1[0], 0], [0, 0, 1.0]])
    R2 = np.array([[e2[0], e2[1], 0], [-e2[1], e2[0], 0], [0, 0, 1.0]])
    G = R2 @ (T2.T @ F @ T1) @ R1.T
    a, b, c, d, f1, f2 = G[1, 1], G[1, 2], G[2, 1], G[2, 2], e1[2], e2[2]
    g = sextic(a, b, c, d, f1, f2)
    g = g / np.abs(g).max()
    r = np.roots(g)
    real = np.sort(r.real[np.abs(r.imag) <= REAL_TOL * np.maximum(1.0, np.abs(r))])
    if polish is not None:
        real = np.array([polish(g, t) for t in real])
    cands = list(real) + [np.inf]
    with np.errstate(all="ignore"):
        costs = np.array([cost(t, a, b, c, d, f1, f2) for t in cands])
    costs[np.isnan(costs)] = np.inf
    k = int(np.argmin(costs))
    t = cands[k]
    if np.isinf(t):
        x1 = np.array([f1, 0.0, f1 * f1])
        x2 = np.array([f2 * c * c, -a * c, f2 * f2 * c * c + a * a])
    else:
        x1 = np.array([t * t * f1, t, t * t * f1 * f1 + 1.0])
        x2 = np.array([f2 * (c * t + d) ** 2, -(a * t + b) * (c * t + d), f2 * f2 * (c * t + d) ** 2 + (a * t + b) ** 2])
    with np.errstate(all="ignore"):
        x1, x2 = T1 @ R1.T @ x1, T2 @ R2.T @ x2
        out = dict(p=x1[:2] / x1[2], q=x2[:2] / x2[2], cost=costs[k], roots=real, costs=np.sort(costs))
    if not (np.isfinite(out["p"]).all() and np.isfinite(out["q"]).all() and np.isfinite(out["cost"])):
        return nan
    return out


def correct_matches(F, P, Q, polish=None):
    """P, Q [M,2] under one F -> dict(p [M,2], q [M,2], cost [M], near_tie [M] bool, roots: list of M arrays)."""
    res = [correct_one(F, p, q, polish) for p, q in zip(np.asarray(P), np.asarray(Q))]
    tie = np.array([len(r["costs"]) > 1 and r["costs"][1] - r["costs"][0] <= NEAR_TIE * r["costs"][1] for r in res])
    return dict(p=np.array([r["p"] for r in res]), q=np.array([r["q"] for r in res]), cost=np.array([r["cost"] for r in res]),
                near_tie=tie, roots=[r["roots"] for r in res])


def polish_longdouble(g, t):
    """Newton steps on a root of the polynomial g (highest power first) in numpy.longdouble."""
    gl = np.asarray(g, np.longdouble)
    dl = np.polyder(gl)
    x = np.longdouble(t)
    for _ in range(6):
        x = x - np.polyval(gl, x) / np.polyval(dl, x)
    return float(x)


def line_distance(F, P, Q):
    """Distance of q to the epipolar line F p [M], in pixels."""
    l = np.c_[P, np.ones(len(P))] @ np.asarray(F, np.float64).T
    return np.abs((l * np.c_[Q, np.ones(len(Q))]).sum(1)) / np.hypot(l[:, 0], l[:, 1])


def pencil_min_cost(F, P, Q, scan=8192, iters=80):
    """The same minimum without the polynomial: every pair of corresponding epipolar lines is l1 = e1 x w, l2 = F w for a
    direction w = (cos th, sin th, 0), th in [0, pi); the cost of a pair of lines is dist(p, l1)^2 + dist(q, l2)^2.  A dense
    scan over th, then a golden-section search in the two cells around the best sample.  Returns the minimal cost [M]."""
    F = np.asarray(F, np.float64)
    F = F / np.abs(F).max()
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    e1, _ = epipoles(F)
    ph, qh = np.c_[P, np.ones(len(P))], np.c_[Q, np.ones(len(Q))]

    def cost_of(th, a, b):  # th [m] or [m, n] angles, a, b [m,3] the points -> cost, shaped as th
        w = np.stack((np.cos(th), np.sin(th), np.zeros_like(th)), -1)
        l1 = np.cross(e1, w)
        l2 = w @ F.T
        sh = (slice(None),) + (None,) * (th.ndim - 1)
        d1 = (l1 * a[sh]).sum(-1) ** 2 / (l1[..., 0] ** 2 + l1[..., 1] ** 2)
        d2 = (l2 * b[sh]).sum(-1) ** 2 / (l2[..., 0] ** 2 + l2[..., 1] ** 2)
        return d1 + d2

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
