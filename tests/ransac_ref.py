"""fp64 restatement of the RANSAC fundamental-matrix estimator the tests hold csrc/ransac.hip and csrc/ransac_math.h to:
OpenCV 3.4's findFundamentalMat(FM_RANSAC) algorithm as include/dfepe.h (dfepe_ransac_fundamental) specifies it -- sampler,
collinearity rejection, 7-point solve, error, RANSACUpdateNumIters and the sequential selection rule.  numpy only; written from
the published algorithm, independently of the kernels (the null space comes from numpy's SVD, not from a QR)."""
import math

import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
FLT_EPSILON = float(np.finfo(np.float32).eps)
DBL_EPSILON = float(np.finfo(np.float64).eps)
DBL_MIN = float(np.finfo(np.float64).tiny)
NO_ROOT, NO_SAMPLE = -1, -2


def splitmix64(x):
    x = (x + GOLDEN) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


class Stream:
    """Draw c of iteration k: splitmix64(key + c * GOLDEN), key = splitmix64(seed ^ splitmix64(k)); index = (hi32 * N) >> 32."""

    def __init__(self, seed, k):
        self.key = splitmix64((seed & M64) ^ splitmix64(k))
        self.ctr = 0

    def index(self, N):
        x = splitmix64((self.key + self.ctr * GOLDEN) & M64)
        self.ctr += 1
        return ((x >> 32) * N) >> 32


def collinear_last(x, y):
    """haveCollinearPoints for the last of 7 points: differences of the float32 coordinates in float32, the test in float64."""
    x = np.asarray(x, np.float32)
    y = np.asarray(y, np.float32)
    i = len(x) - 1
    for j in range(i):
        dx1, dy1 = float(x[j] - x[i]), float(y[j] - y[i])
        for k in range(j):
            dx2, dy2 = float(x[k] - x[i]), float(y[k] - y[i])
            if abs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (abs(dx1) + abs(dy1) + abs(dx2) + abs(dy2)):
                return True
    return False


def draw_sample(seed, k, pts, max_attempts=1000):
    """Iteration k's 7 indices into pts [N,4] (float32 pixels), or None when every attempt was collinear."""
    pts = np.asarray(pts, np.float32)
    N = pts.shape[0]
    s = Stream(seed, k)
    for _ in range(max_attempts):
        idx = []
        while len(idx) < 7:
            v = s.index(N)
            if v not in idx:
                idx.append(v)
        p = pts[idx]
        if not collinear_last(p[:, 0], p[:, 1]) and not collinear_last(p[:, 2], p[:, 3]):
            return idx
    return None


def solve_cubic(c3, c2, c1, c0):
    """Real roots (one or three) of c3 l^3 + c2 l^2 + c1 l + c0, two Newton steps each, ascending."""
    if c3 == 0.0:
        if c2 == 0.0:
            return [] if c1 == 0.0 else [-c0 / c1]
        d = c1 * c1 - 4.0 * c2 * c0
        if d < 0.0:
            return []
        q = -0.5 * (c1 + math.copysign(math.sqrt(d), c1 if c1 != 0.0 else 1.0))
        r = [q / c2, c0 / q if q != 0.0 else q / c2]
    else:
        a, b, c = c2 / c3, c1 / c3, c0 / c3
        Q = (a * a - 3.0 * b) / 9.0
        R = (2.0 * a ** 3 - 9.0 * a * b + 27.0 * c) / 54.0
        d = Q ** 3 - R * R
        if d >= 0.0:
            th = math.acos(min(max(R / math.sqrt(Q ** 3), -1.0), 1.0)) if Q > 0 else 0.0
            sq = -2.0 * math.sqrt(max(Q, 0.0))
            r = [sq * math.cos((th + o) / 3.0) - a / 3.0 for o in (0.0, 2 * math.pi, -2 * math.pi)]
        else:
            e = (math.sqrt(-d) + abs(R)) ** (1.0 / 3.0)
            if R > 0:
                e = -e
            r = [(e + Q / e) - a / 3.0]
    out = []
    for x in r:
        for _ in range(2):
            f = ((c3 * x + c2) * x + c1) * x + c0
            df = (3.0 * c3 * x + 2.0 * c2) * x + c1
            if df != 0.0:
                x -= f / df
        out.append(x)
    return sorted(out)


def _hartley(px, py):
    px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
    cx, cy = px.mean(), py.mean()
    ss = ((px - cx) ** 2 + (py - cy) ** 2).sum()
    s = math.sqrt(2.0 * len(px) / ss) if ss > 0 else 1.0
    return np.array([[s, 0, -s * cx], [0, s, -s * cy], [0, 0, 1.0]])


def seven_point(p7):
    """p7 [7,4] pixels -> list of F (pixels, F22 = 1 where |F22| > DBL_EPSILON) for the real roots of det(l F1 + (1 - l) F2)
    in ascending l, {F1, F2} the right singular vectors of the two smallest singular values (normalised coordinates)."""
    p7 = np.asarray(p7, np.float64)
    T1, T2 = _hartley(p7[:, 0], p7[:, 1]), _hartley(p7[:, 2], p7[:, 3])
    h1 = np.c_[p7[:, :2], np.ones(7)] @ T1.T
    h2 = np.c_[p7[:, 2:], np.ones(7)] @ T2.T
    A = np.stack([h2[:, 0] * h1[:, 0], h2[:, 0] * h1[:, 1], h2[:, 0], h2[:, 1] * h1[:, 0], h2[:, 1] * h1[:, 1], h2[:, 1],
                  h1[:, 0], h1[:, 1], np.ones(7)], 1)
    V = np.linalg.svd(A)[2]
    F1, F2 = V[7].reshape(3, 3), V[8].reshape(3, 3)
    D = F1 - F2
    # det(F2 + l D) sampled at four points -> exact cubic coefficients
    ls = np.array([0.0, 1.0, -1.0, 2.0])
    vals = [np.linalg.det(F2 + l * D) for l in ls]
    c3, c2, c1, c0 = np.linalg.solve(np.vander(ls, 4), vals)
    Fs = []
    for lam in solve_cubic(c3, c2, c1, c0):
        F = T2.T @ (F2 + lam * D) @ T1
        if abs(F[2, 2]) > DBL_EPSILON:
            F = F / F[2, 2]
        Fs.append(F)
    return Fs


def errors(F, pts):
    """OpenCV's FMEstimatorCallback::computeError: max(d1^2, d2^2) per correspondence, fp64."""
    pts = np.asarray(pts, np.float64)
    F = np.asarray(F, np.float64).reshape(3, 3)
    h1 = np.c_[pts[:, :2], np.ones(len(pts))]
    h2 = np.c_[pts[:, 2:], np.ones(len(pts))]
    l2 = h1 @ F.T   # lines in image 2
    l1 = h2 @ F     # lines in image 1
    r = (h2 * l2).sum(1)
    d2 = r * r / (l2[:, 0] ** 2 + l2[:, 1] ** 2)
    d1 = r * r / (l1[:, 0] ** 2 + l1[:, 1] ** 2)
    return np.maximum(d1, d2)


def update_num_iters(p, ep, niters):
    """OpenCV's RANSACUpdateNumIters(p, ep, 7, niters), (1 - ep)^7 by the same multiplications as the kernels."""
    p = min(max(p, 0.0), 1.0)
    ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, DBL_MIN)
    q = 1.0 - ep
    q2 = q * q
    q4 = q2 * q2
    den = 1.0 - q4 * q2 * q
    if den < DBL_MIN:
        return 0
    ln, ld = math.log(num), math.log(den)
    if ld >= 0 or -ln >= niters * (-ld):
        return niters
    return int(np.rint(ln / ld))


def select(counts, N, confidence, max_iters):
    """The sequential rule over a count table [max_iters, 3] -> (best count, best k, best root, iterations consumed)."""
    best, niters, bk, br, k = 0, max_iters, -1, -1, 0
    while k < niters:
        if counts[k][0] == NO_SAMPLE:
            break
        for r in range(3):
            c = int(counts[k][r])
            if c > max(best, 6):
                best, bk, br = c, k, r
                niters = update_num_iters(confidence, (N - c) / N, niters)
        k += 1
    return best, bk, br, k


def hypotheses(pts, seed, max_iters):
    """Every iteration's sample and its roots: list of (idx or None, [F, ...])."""
    out = []
    for k in range(max_iters):
        idx = draw_sample(seed, k, pts)
        out.append((idx, [] if idx is None else seven_point(np.asarray(pts, np.float32)[idx])))
    return out
