"""float64 restatement of the seven small pose helpers of dfepe_geo_misc (include/dfepe.h, "Small pose-geometry helpers"), one item
at a time, plain loops: what tests/test_pose_helpers_edges_gpu.py holds csrc/geom.hip's geo_misc_kernel to.  Inputs are the float32
values the kernel reads, widened to float64; nothing here runs on a GPU or imports the product.

Every function that feeds a bound also returns the reference's own conditioning term: the change of its output when the argument
of its last float64 operation moves by ULPS = 4 float64 ulps (the kernel computes in float64 and rounds once to float32, so it may
differ from this restatement by the rounding of the operations before the last one, and by nothing else)."""
import math

import numpy as np

ULPS = 4
EPS64 = 2.0 ** -52
RAD2DEG = 57.29577951308232  # the kernel's constant: float64(180 / pi)


def _w(x, shape):
    a = np.asarray(x)
    assert a.dtype == np.float32, "the reference takes the float32 values the kernel is given"
    return a.astype(np.float64).reshape(shape)


def ulp32(x):
    """Spacing of float32 at |x| (x already rounded to float32)."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


# ---- kind 0 -----------------------------------------------------------------------------------------------------------------
def quat(R32):
    """Trace-method quaternion with q0 >= 0 (utils_geo._R_to_q): (q [4], branch 0..3, flipped, conditioning [4]).  The branch
    tests read m = R^T, whose diagonal is R's."""
    R = _w(R32, (3, 3))
    m = R.T
    if m[2, 2] < 0.0:
        if m[0, 0] > m[1, 1]:
            br, t = 0, 1.0 + m[0, 0] - m[1, 1] - m[2, 2]
            v = [m[1, 2] - m[2, 1], t, m[0, 1] + m[1, 0], m[2, 0] + m[0, 2]]
        else:
            br, t = 1, 1.0 - m[0, 0] + m[1, 1] - m[2, 2]
            v = [m[2, 0] - m[0, 2], m[0, 1] + m[1, 0], t, m[1, 2] + m[2, 1]]
    else:
        if m[0, 0] < -m[1, 1]:
            br, t = 2, 1.0 - m[0, 0] - m[1, 1] + m[2, 2]
            v = [m[0, 1] - m[1, 0], m[2, 0] + m[0, 2], m[1, 2] + m[2, 1], t]
        else:
            br, t = 3, 1.0 + m[0, 0] + m[1, 1] + m[2, 2]
            v = [t, m[1, 2] - m[2, 1], m[2, 0] - m[0, 2], m[0, 1] - m[1, 0]]
    sc = 0.5 / math.sqrt(t)
    flip = v[0] * sc < 0.0
    if flip:
        sc = -sc
    q = np.array([sc * x for x in v])
    return q, br, flip, ULPS * EPS64 * np.abs(q)  # the last operation is the product sc * v[k]


# ---- kind 1 -----------------------------------------------------------------------------------------------------------------
def _rotation_sc(R0, R1, dtype=np.float64):
    """|axis part| and tr - 1 of R0 R1^T, in plain loops."""
    D = np.zeros((3, 3), dtype)
    for r in range(3):
        for c in range(3):
            D[r, c] = R0[r, 0] * R1[c, 0] + R0[r, 1] * R1[c, 1] + R0[r, 2] * R1[c, 2]
    ax, ay, az = D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]
    return np.sqrt(ax * ax + ay * ay + az * az), D[0, 0] + D[1, 1] + D[2, 2] - dtype(1.0)


def rotation_angle(R0_32, R1_32):
    """atan2(|axis|, tr - 1) of R0 R1^T in degrees (oracle.rotation_angle_deg): (angle, conditioning)."""
    s, c = (float(x) for x in _rotation_sc(_w(R0_32, (3, 3)), _w(R1_32, (3, 3))))
    a = math.atan2(s, c) * RAD2DEG
    ds, dc = ULPS * np.spacing(abs(s)), ULPS * np.spacing(abs(c))
    cond = max(abs(math.atan2(max(s + i * ds, 0.0), c + j * dc) * RAD2DEG - a) for i in (-1, 1) for j in (-1, 1))
    return a, cond


def rotation_angle_longdouble(R0_32, R1_32):
    """The same formula on the same float32 inputs in np.longdouble (the CPU test's yardstick for the float64 restatement)."""
    L = np.longdouble
    s, c = _rotation_sc(np.asarray(R0_32).astype(L).reshape(3, 3), np.asarray(R1_32).astype(L).reshape(3, 3), L)
    return float(np.arctan2(s, c) * (L(180.0) / np.arctan2(L(0.0), L(-1.0))))


# ---- kind 2 -----------------------------------------------------------------------------------------------------------------
def vector_angle(v1_32, v2_32):
    """acos(clip(v1.v2 / ((|v1| + 1e-10)(|v2| + 1e-10) + 1e-10))) in degrees (oracle.vector_angle_deg): (angle, conditioning)."""
    a, b = _w(v1_32, (3,)), _w(v2_32, (3,))
    dot = n1 = n2 = 0.0
    for k in range(3):
        dot += float(a[k] * b[k])
        n1 += float(a[k] * a[k])
        n2 += float(b[k] * b[k])
    x = dot / ((math.sqrt(n1) + 1e-10) * (math.sqrt(n2) + 1e-10) + 1e-10)
    f = lambda z: math.acos(min(max(z, -1.0), 1.0)) * RAD2DEG
    ang = f(x)
    d = ULPS * np.spacing(abs(x))
    return ang, max(abs(f(x - d) - ang), abs(f(x + d) - ang))


# ---- kind 3 -----------------------------------------------------------------------------------------------------------------
def singular_values(E32):
    return np.linalg.svd(_w(E32, (3, 3)), compute_uv=False)


def relative_gap(E32):
    """(s2 - s3) / s1: what the smallest singular triplet, hence the projection, is conditioned by (0 for the zero matrix)."""
    s = singular_values(E32)
    return float((s[1] - s[2]) / s[0]) if s[0] > 0.0 else 0.0


def project(E32):
    """U diag(1, 1, 0) V^T from np.linalg.svd."""
    U, _, Vt = np.linalg.svd(_w(E32, (3, 3)))
    return U @ np.diag([1.0, 1.0, 0.0]) @ Vt


# ---- kind 4 -----------------------------------------------------------------------------------------------------------------
W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])


def decompose(E32):
    """oracle.get_M2s (utils_F._get_M2s): R1 = U W V^T, R2 = U W^T V^T with W negated when det(U W V^T) < 0; t = u3 / |u3|."""
    U, _, Vt = np.linalg.svd(_w(E32, (3, 3)))
    w = -W if np.linalg.det(U @ W @ Vt) < 0.0 else W
    return U @ w @ Vt, U @ w.T @ Vt, U[:, 2] / np.linalg.norm(U[:, 2])


# ---- kind 5 -----------------------------------------------------------------------------------------------------------------
def congruence(F32, A32):
    """A^T F A: (result [3,3], conditioning [3,3] = ULPS ulps on every product the last sums add up)."""
    F, A = _w(F32, (3, 3)), _w(A32, (3, 3))
    return A.T @ F @ A, ULPS * EPS64 * (np.abs(A).T @ np.abs(F) @ np.abs(A))


# ---- kind 6 -----------------------------------------------------------------------------------------------------------------
def camera_rotation(delta32):
    """np.linalg.inv(delta)[:3, :3]: (result [3,3], conditioning = cond2(delta) 2^-52 |result|_2, per entry).  The relative term
    cond2(delta) 2^-52 is scaled by the 2-norm of the 3x3 block that is compared, and by nothing larger: 1 for a rigid motion however
    far it translates, up to several hundred for the ill-conditioned general ones, whose entries are that large -- there
    np.linalg.inv itself is 13 times cond2 2^-52 away from a np.longdouble inverse (tests/test_pose_helper_ref_cpu.py)."""
    d = _w(delta32, (4, 4))
    r = np.linalg.inv(d)[:3, :3]
    return r, float(np.linalg.cond(d) * EPS64 * np.linalg.norm(r, 2))


def inverse_longdouble(delta32):
    """Gauss-Jordan with partial pivoting in np.longdouble, plain loops: the CPU test's yardstick for np.linalg.inv."""
    L = np.longdouble
    a = np.concatenate((np.asarray(delta32).astype(L).reshape(4, 4), np.eye(4, dtype=L)), 1)
    for c in range(4):
        p = c + int(np.argmax(np.abs(a[c:, c])))
        a[[c, p]] = a[[p, c]]
        a[c] = a[c] / a[c, c]
        for r in range(4):
            if r != c:
                a[r] = a[r] - a[r, c] * a[c]
    return a[:, 4:]
