"""fp64 restatement of the cheirality-checked pose selection (utils_F._get_M2s / _E_to_M_train as oracle.cheirality_select states
them), vectorised over the correspondences of a pair, with a per-correspondence answer and an `undecided` band.

Written from the reference's statement, not from the kernel: the candidates come from numpy.linalg.svd of E in the reference's
order (R1,t), (R1,-t), (R2,t), (R2,-t); every candidate is triangulated on its own (the kernel triangulates once per rotation and
reads (R,-t) off the sign of the same vector); the null vector is the last right singular vector of the 4x4 DLT matrix A itself
(the kernel forms A^T A).  Inputs are the fp32 values the kernel sees; everything after them is fp64.

The band.  X the unit null vector, s1 >= s2 >= s3 >= s4 the singular values of A,
    eta = max(1e-8, 64 * 2^-52 * s1^2 / (s3^2 - s4^2)).
The first term is ten times the 1e-9 eigenvector error cheirality_body.h documents for its fp64 route.  The second: the kernel's
route takes the eigenvector of the fp64-ROUNDED normal matrix A^T A, whose entries carry a relative rounding error 2^-52 of
|A^T A| ~ s1^2; first-order perturbation theory moves the eigenvector of the smallest eigenvalue s4^2 by at most
|dS| / gap = 2^-52 s1^2 / (s3^2 - s4^2), times a safety factor of 64 (entries, accumulation order, the unit-trace scaling).  A
correspondence is undecided for a candidate when one of its test quantities lies within the band of its bound, with the weights
the quantities have as linear forms of X (|R3| = 1, |t3| <= 1):
    |X3| < eta, |z1n| < eta, |z2n| < 2 eta, ||z1n| - thr |X3|| < (1 + thr) eta, ||z2n| - thr |X3|| < (2 + thr) eta
(z1n = X2, z2n = R3 . X012 + t3 X3: the undivided numerators of the two depths)."""
import numpy as np

W90 = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
EPS64 = 2.0 ** -52
ETA_FLOOR = 1e-8
ETA_SAFETY = 64.0


def essential(F, pre):
    """E = pre^T F pre in fp64 from the fp32 values (the matrix the fused route decomposes, before its rounding to fp32)."""
    A = np.asarray(pre, np.float32).astype(np.float64)
    return A.T @ np.asarray(F, np.float32).astype(np.float64) @ A


def candidates(E):
    """The four scene motions (R, t) of E [3,3] in the reference's order: (R1,t), (R1,-t), (R2,t), (R2,-t); R1 = U W V^T,
    R2 = U W^T V^T with W negated when det(U W V^T) < 0, t = u3 / |u3|."""
    U, _, Vt = np.linalg.svd(np.asarray(E, np.float64))
    W = -W90 if np.linalg.det(U @ W90 @ Vt) < 0 else W90
    t = U[:, 2] / np.linalg.norm(U[:, 2])
    return [(R, s * t) for R in (U @ W @ Vt, U @ W.T @ Vt) for s in (1.0, -1.0)]


def inverse_pose(R, t):
    """Camera motion [3,4] = inverse of the scene motion [R | t] (utils_misc._inv_Rt)."""
    return np.c_[R.T, -R.T @ t]


def triangulate(P1, P2, m):
    """Batched DLT of m [n,4] (all finite): unit null vectors X [n,4] and singular values [n,4] of [x P3 - P1; y P3 - P2] over
    both views."""
    A = np.stack((m[:, 0, None] * P1[2] - P1[0], m[:, 1, None] * P1[2] - P1[1],
                  m[:, 2, None] * P2[2] - P2[0], m[:, 3, None] * P2[2] - P2[1]), 1)
    _, s, Vt = np.linalg.svd(A)
    return Vt[:, 3, :], s


def select(counts):
    """The reference's vote: the first maximum, -1 when it is 0."""
    counts = [int(c) for c in counts]
    w = int(np.argmax(counts))
    return w if counts[w] > 0 else -1


def reference(E, K, matches, depth_thres, pre=None):
    """One pair.  E [3,3] fp32 (or F with pre: then E = pre^T F pre), K [3,3] fp32, matches [N,4] fp32 (non-finite rows count
    nowhere), depth_thres as given to the kernel (rounded to fp32 here).  Returns a dict: in_front [4,N] bool, undecided [4,N]
    bool, lo / hi [4] (the interval of each candidate's count), cands (the four (R, t)), E (the fp64 matrix decomposed)."""
    E = np.asarray(E, np.float32).astype(np.float64) if pre is None else essential(E, pre)
    K = np.asarray(K, np.float32).astype(np.float64)
    m = np.asarray(matches, np.float32).astype(np.float64)
    thr = float(np.float32(depth_thres))
    N = m.shape[0]
    cands = candidates(E)
    fin = np.isfinite(m).all(1)
    mf = m[fin]
    in_front = np.zeros((4, N), bool)
    undecided = np.zeros((4, N), bool)
    P1 = K @ np.c_[np.eye(3), np.zeros(3)]
    if len(mf):
        for c, (R, t) in enumerate(cands):
            X, s = triangulate(P1, K @ np.c_[R, t], mf)
            w, z1n = X[:, 3], X[:, 2]
            z2n = X[:, :3] @ R[2] + t[2] * w
            with np.errstate(divide="ignore", invalid="ignore"):
                z1, z2 = z1n / w, z2n / w
                eta = np.maximum(ETA_FLOOR, ETA_SAFETY * EPS64 * s[:, 0] ** 2 / (s[:, 2] ** 2 - s[:, 3] ** 2))
            eta = np.where(np.isfinite(eta), eta, np.inf)
            in_front[c, fin] = (z1 > 0) & (z1 < thr) & (z2 > 0) & (z2 < thr)
            aw = thr * np.abs(w)
            undecided[c, fin] = ((np.abs(w) < eta) | (np.abs(z1n) < eta) | (np.abs(z2n) < 2 * eta) |
                                 (np.abs(np.abs(z1n) - aw) < (1 + thr) * eta) | (np.abs(np.abs(z2n) - aw) < (2 + thr) * eta))
    lo = (in_front & ~undecided).sum(1)
    return {"in_front": in_front, "undecided": undecided, "lo": lo, "hi": lo + undecided.sum(1), "cands": cands, "E": E}
