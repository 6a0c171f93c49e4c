"""fp64 restatement of the two-view structure entry points (dfepe_triangulate, dfepe_two_view_structure, dfepe_reproject), written
from their statement in include/dfepe.h, not from the kernel.  Inputs are the fp32 values the kernel sees; everything after them
is fp64.  The null vector is the last right singular vector of the 4x4 DLT matrix A itself (numpy.linalg.svd), not of A^T A.

The band is the project's own (tests/cheirality_ref.py): with s1 >= .. >= s4 the singular values of A,
    eta = max(ETA_FLOOR, ETA_SAFETY * EPS64 * s1^2 / (s3^2 - s4^2)),   inf where the gap is 0.
mp_null_vector() is the same vector at 50 digits (mpmath), against which the restatement is itself pinned (within eta / 16)."""
import numpy as np

from cheirality_ref import EPS64, ETA_FLOOR, ETA_SAFETY

U24 = 2.0 ** -24  # one rounding to fp32
REPROJ_SAFETY = 32.0


def f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


def dlt_matrices(P1, P2, m):
    """A [n,4,4] of P1, P2 [3,4] and m [n,4], all fp64."""
    with np.errstate(invalid="ignore"):  # inf * 0 of a poisoned row: NaN on purpose
        return np.stack((m[:, 0, None] * P1[2] - P1[0], m[:, 1, None] * P1[2] - P1[1],
                         m[:, 2, None] * P2[2] - P2[0], m[:, 3, None] * P2[2] - P2[1]), 1)


def null_vectors(P1, P2, m):
    """P1, P2 [3,4], m [n,4] fp64 -> Xh [n,4] (unit, w >= 0; NaN rows where A is not finite or zero), eta [n] (NaN there)."""
    n = len(m)
    Xh, eta = np.full((n, 4), np.nan), np.full(n, np.nan)
    A = dlt_matrices(P1, P2, m)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(A).all((1, 2)) & (np.abs(A).sum((1, 2)) > 0)
    if ok.any():
        _, s, Vt = np.linalg.svd(A[ok])
        X = Vt[:, 3, :]
        X = np.where(X[:, 3:4] < 0, -X, X)
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.maximum(ETA_FLOOR, ETA_SAFETY * EPS64 * s[:, 0] ** 2 / (s[:, 2] ** 2 - s[:, 3] ** 2))
        Xh[ok], eta[ok] = X, np.where(np.isfinite(e), e, np.inf)
    return Xh, eta


def triangulate(P1, P2, matches):
    """One pair, P1, P2 [3,4] and matches [n,4] as the kernel sees them (fp32).  -> Xh [n,4] fp64, eta [n]."""
    return null_vectors(f64(P1), f64(P2), f64(matches))


def scene_motion(Rt, camera_motion):
    """Rt [3,4] fp32 -> (R, t) fp64 of the scene motion: Rt itself, or the inverse of a camera motion (utils_misc._inv_Rt)."""
    Rt = f64(Rt)
    R, t = Rt[:, :3], Rt[:, 3]
    return (R.T, -R.T @ t) if camera_motion else (R, t)


def cameras(Rt, K, camera_motion):
    R, t = scene_motion(Rt, camera_motion)
    K = f64(K)
    return K @ np.c_[np.eye(3), np.zeros(3)], K @ np.c_[R, t], R, t


def two_view_structure(Rt, K, matches, camera_motion=False):
    """One pair, unscaled and unclamped.  -> dict(Xh, eta, w, X [n,3], z1, z2 [n]) fp64."""
    P1, P2, R, t = cameras(Rt, K, camera_motion)
    # the cameras are fp64 here (the kernel forms them in fp64 too): no rounding to fp32 in between
    Xh, eta = null_vectors(P1, P2, f64(matches))
    with np.errstate(divide="ignore", invalid="ignore"):
        X3 = Xh[:, :3] / Xh[:, 3:4]
        z2 = X3 @ R[2] + t[2]
    return {"Xh": Xh, "eta": eta, "w": Xh[:, 3], "X": X3, "z1": X3[:, 2], "z2": z2}


def value_bound(v, a, w, eta, scale=1.0):
    """First-order propagation of eta through v / w plus one fp32 rounding: (a eta + |v| eta) / (|w| - eta) + 2^-24 |v|, both terms
    times |scale| (v unscaled).  Only meaningful on held points (|w| > 2 eta)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return abs(scale) * ((a * eta + np.abs(v) * eta) / (np.abs(w) - eta) + U24 * np.abs(v))


def reproject(X, Rt, K, camera_motion=False):
    """One pair.  X [m,3] fp32 -> dict(x [m,2], z [m], bound [m,2], held [m]) fp64: u = K (R X + t), x = u_01 / u_2, z = u_2;
    bound = 2^-24 |x| + 32 2^-52 (S_u + |x| S_z) / |u_2| with S the sums of the absolute values of the expanded terms
    K_ij R_jk X_k and K_ij t_j (for a camera motion t_j = -sum_k R_jk tc_k is expanded too); held: |u_2| > 32 2^-52 S_z."""
    X, Kd = f64(X), f64(K)
    R, t = scene_motion(Rt, camera_motion)
    u = (X @ R.T + t) @ Kd.T
    KR = np.abs(Kd)[:, :, None] * np.abs(R)[None, :, :]                       # |K_ij R_jk|
    S = np.einsum("ijk,mk->mi", KR, np.abs(X))
    if camera_motion:
        S = S + np.einsum("ijk,k->i", KR, np.abs(f64(Rt)[:, 3]))
    else:
        S = S + np.abs(Kd) @ np.abs(t)
    with np.errstate(divide="ignore", invalid="ignore"):
        x = u[:, :2] / u[:, 2:3]
        bound = U24 * np.abs(x) + REPROJ_SAFETY * EPS64 * (S[:, :2] + np.abs(x) * S[:, 2:3]) / np.abs(u[:, 2:3])
    return {"x": x, "z": u[:, 2], "bound": bound, "z_bound": U24 * np.abs(u[:, 2]) + REPROJ_SAFETY * EPS64 * S[:, 2], "held": np.abs(u[:, 2]) > REPROJ_SAFETY * EPS64 * S[:, 2]}


def within(x, y, xlim, ylim):
    """utils_misc.within, by its definition."""
    return (x >= 0) & (y >= 0) & (x <= xlim) & (y <= ylim)


def mp_null_vector(P1, P2, m, digits=50):
    """The unit null vector (w >= 0) of the DLT matrix of ONE correspondence at `digits` digits: P1, P2 [3,4] and m [4] fp64
    values, taken exactly.  -> [4] fp64 (rounded once at the end)."""
    import mpmath as mp

    with mp.workdps(digits):
        P1m, P2m = mp.matrix(P1.tolist()), mp.matrix(P2.tolist())
        x = [mp.mpf(float(v)) for v in m]
        A = mp.matrix(4, 4)
        for c in range(4):
            A[0, c] = x[0] * P1m[2, c] - P1m[0, c]
            A[1, c] = x[1] * P1m[2, c] - P1m[1, c]
            A[2, c] = x[2] * P2m[2, c] - P2m[0, c]
            A[3, c] = x[3] * P2m[2, c] - P2m[1, c]
        _, S, V = mp.svd_r(A)
        k = min(range(4), key=lambda i: S[i])
        v = [V[k, c] for c in range(4)]
        nrm = mp.sqrt(sum(c * c for c in v))
        sg = -1 if v[3] < 0 else 1
        return np.array([float(sg * c / nrm) for c in v])
