"""The fp64 yardstick of the odometry evaluation (dfepe_pose_chain, dfepe_snippet_errors): a restatement in Python / numpy of
what the reference does on the host,

    relative_pose_cam_to_body   Train_model_pipeline.py:1098-1108    inv(C) @ M @ C
    get_abs_poses               deepFEPE/utils/eval_tools.py:268-284 last = pose @ last; abs.append(inv(last)[:3])
    compensate_poses            eval_tools.py:252-265
    compute_pose_error          eval_tools.py:309-331
    pose_seq_ate                eval_tools.py:334-375

and the bounds the tests hold the kernels (and the host build of csrc/odometry_math.h) to.  tests/test_odometry_ref_cpu.py
checks this file against the reference's own output (tests/golden/odometry.npz).

How the arithmetic is written.  Every product, sum and quotient below is one correctly rounded IEEE operation on Python floats
or numpy float64 arrays (neither fuses a multiply with an add), in the association csrc/odometry_math.h spells out:
r_ij = (a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j (+ a_i3), the inverse as adjugate / determinant with one division per entry, sums
over a snippet pose by pose and x, y, z within a pose.  The reference itself uses `@` and numpy.linalg.inv, whose orders are the
BLAS's and LAPACK's business; the difference is rounding and is bounded in golden_*_tol below.

The chain comes in two association orders of the same product P_k ... P_1:
    chain_sequential   the reference's loop, strictly left to right;
    chain_tree         a Hillis-Steele scan, every prefix a balanced tree of pairwise products.
Their per-pose distance (chain_spread) is the reference's OWN sensitivity to re-association on the given inputs, and it is the
unit the kernel is measured in: chain_bound = 4 spread_k + k 2^-52 max|entry_k| (any valid re-association is one more rounding
pattern of the same family; the floor keeps the bound from collapsing where two orders happen to agree to the last bit, which
they do for k <= 2 always).  Seen on the CPU with n = 1591, rotations up to pi: spread up to 2.0e-13 at entries of size 63.
"""
import numpy as np

U = 2.0 ** -52  # spacing of doubles in [1, 2)
IDENT = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


# ---- the arithmetic of csrc/odometry_math.h: a pose is a sequence of 12 entries (floats, or arrays of one shape) --------------
def mul12(a, b):
    r = [None] * 12
    for i in range(3):
        for j in range(4):
            v = (a[4 * i] * b[j] + a[4 * i + 1] * b[4 + j]) + a[4 * i + 2] * b[8 + j]
            if j == 3:
                v = v + a[4 * i + 3]
            r[4 * i + j] = v
    return r


def inv9(a):
    c00, c01, c02 = a[4] * a[8] - a[5] * a[7], a[2] * a[7] - a[1] * a[8], a[1] * a[5] - a[2] * a[4]
    c10, c11, c12 = a[5] * a[6] - a[3] * a[8], a[0] * a[8] - a[2] * a[6], a[2] * a[3] - a[0] * a[5]
    c20, c21, c22 = a[3] * a[7] - a[4] * a[6], a[1] * a[6] - a[0] * a[7], a[0] * a[4] - a[1] * a[3]
    det = (a[0] * c00 + a[1] * c10) + a[2] * c20
    return [c00 / det, c01 / det, c02 / det, c10 / det, c11 / det, c12 / det, c20 / det, c21 / det, c22 / det]


def rot9(a):
    return [a[0], a[1], a[2], a[4], a[5], a[6], a[8], a[9], a[10]]


def inv12(a, rigid=False):
    """rigid=True is the WRONG inverse (the transpose), kept for the test that check() notices it."""
    r = rot9(a)
    ai = [r[0], r[3], r[6], r[1], r[4], r[7], r[2], r[5], r[8]] if rigid else inv9(r)
    out = [None] * 12
    for i in range(3):
        out[4 * i:4 * i + 3] = ai[3 * i:3 * i + 3]
        out[4 * i + 3] = -((ai[3 * i] * a[3] + ai[3 * i + 1] * a[7]) + ai[3 * i + 2] * a[11])
    return out


def conj12(m, c):
    return mul12(mul12(inv12(c), m), c)


def _cols(x):
    """[n,12] -> list of 12 arrays [n]"""
    x = np.asarray(x, np.float64).reshape(-1, 12)
    return [np.ascontiguousarray(x[:, k]) for k in range(12)]


def _rows(c):
    return np.stack([np.asarray(v, np.float64) for v in c], axis=-1)


def body_poses(rel, cam2body=None):
    """relative_pose_cam_to_body for every pose: rel [n,12]; cam2body None, [12] (one for the sequence) or [n,12]."""
    rel = np.asarray(rel, np.float64).reshape(-1, 12)
    if cam2body is None or len(rel) == 0:
        return rel.copy()
    c = np.broadcast_to(np.asarray(cam2body, np.float64).reshape(-1, 12), rel.shape)
    return _rows(conj12(_cols(rel), _cols(c)))


def _finish(prefix, rigid=False):
    """prefix [n,12] (P_k ... P_1) -> abs [n+1,12] with the identity first"""
    out = np.empty((len(prefix) + 1, 12))
    out[0] = IDENT
    if len(prefix):
        out[1:] = _rows(inv12(_cols(prefix), rigid=rigid))
    return out


def chain_sequential(rel, cam2body=None, swapped=False, rigid=False, drop=None):
    """get_abs_poses, strictly in order.  The three switches make the WRONG results check() has to notice: swapped composes
    last @ pose, rigid inverts by transposing, drop = j leaves pose j out of every product that should hold it."""
    P = body_poses(rel, cam2body).tolist()
    last, prefix = list(IDENT), []
    for j, p in enumerate(P):
        if j != drop:
            last = mul12(last, p) if swapped else mul12(p, last)
        prefix.append(last)
    return _finish(np.array(prefix, np.float64).reshape(-1, 12), rigid=rigid)


def chain_tree(rel, cam2body=None):
    """The same products, every prefix as a balanced tree (Hillis-Steele: X[k] <- X[k] . X[k - d], d = 1, 2, 4, ...)."""
    X = body_poses(rel, cam2body)
    d = 1
    while d < len(X):
        X = np.concatenate([X[:d], _rows(mul12(_cols(X[d:]), _cols(X[:-d])))])
        d *= 2
    return _finish(X)


def chain_spread(seq, tree):
    """per pose k = 0..n: max-norm distance of the two association orders"""
    return np.abs(seq - tree).max(axis=1)


def chain_bound(seq, tree):
    """per pose k: what any valid association order may differ from the sequential one (module docstring)"""
    k = np.arange(len(seq), dtype=np.float64)
    return 4.0 * chain_spread(seq, tree) + k * U * np.abs(seq).max(axis=1)


def golden_chain_tol(abs_poses):
    """The restatement against the reference's own get_abs_poses (`@` and numpy.linalg.inv): both are backward-stable
    evaluations of the same product of k near-rotations and of one inverse, each step adding at most 4 roundings per entry
    relative to the largest entry (three products, three sums, condition ~1), the inverse at most 8: (4 k + 8) 2^-53 max|entry_k|,
    doubled because both sides carry it."""
    k = np.arange(len(abs_poses), dtype=np.float64)
    return (4.0 * k + 8.0) * U * np.abs(abs_poses).reshape(len(abs_poses), -1).max(axis=1)


# ---- snippets --------------------------------------------------------------------------------------------------------------
def compensate(P):
    """compensate_poses for windows: P = list of 12 arrays [nw, L] -> the same layout"""
    Rinv = inv9([v[:, :1] for v in rot9(P)])
    t0 = [P[3][:, :1], P[7][:, :1], P[11][:, :1]]
    out = [None] * 12

    def col(q):
        return [(Rinv[3 * i] * q[0] + Rinv[3 * i + 1] * q[1]) + Rinv[3 * i + 2] * q[2] for i in range(3)]

    for j in range(3):
        out[j], out[4 + j], out[8 + j] = col([P[j], P[4 + j], P[8 + j]])
    out[3], out[7], out[11] = col([P[3] - t0[0], P[7] - t0[1], P[11] - t0[2]])
    return out


def snippet_errors(est, gt, nw, L, compensated=True, documented_roles=False):
    """pose_seq_ate's loop body for windows 0 .. nw-1 of est, gt [m,12] (window w = poses w .. w+L-1).
    -> dict: errors64 [nw,2] (ATE, RE before the float32 rounding), errors [nw,2] float32, scale [nw], aligned [nw,12],
    compensated [nw,L,12] (the estimate's), kappa [nw] = sum|est_t gt_t| / |sum est_t gt_t|, den [nw] = sum gt_t^2, degenerate [nw] bool (all
    ground-truth translations of the window exactly zero after compensation).
    documented_roles=True scores compute_pose_error(gt, pred) as its parameter NAMES suggest (gt = ground truth): WRONG, the
    reference passes (est_snip, gt_snip); kept for the test that check() notices it."""
    est, gt = np.asarray(est, np.float64).reshape(-1, 12), np.asarray(gt, np.float64).reshape(-1, 12)
    idx = np.arange(nw)[:, None] + np.arange(L)[None, :]
    E = [est[idx, k] for k in range(12)]
    G = [gt[idx, k] for k in range(12)]
    if compensated:
        E, G = compensate(E), compensate(G)
    comp = np.stack(E, axis=-1)
    a, b = (G, E) if documented_roles else (E, G)  # a: the function's "gt", b: its "pred"
    num, den, re, absnum = np.zeros(nw), np.zeros(nw), np.zeros(nw), np.zeros(nw)
    for i in range(L):
        for c in (3, 7, 11):
            num = num + a[c][:, i] * b[c][:, i]
            den = den + b[c][:, i] * b[c][:, i]
            absnum = absnum + np.abs(a[c][:, i] * b[c][:, i])
        bi = inv9([v[:, i] for v in rot9(b)])
        ar = [v[:, i] for v in rot9(a)]
        R = [(ar[3 * r] * bi[c] + ar[3 * r + 1] * bi[3 + c]) + ar[3 * r + 2] * bi[6 + c] for r in range(3) for c in range(3)]
        s0, s1, s2 = R[1] - R[3], R[5] - R[7], R[2] - R[6]
        s = np.sqrt((s0 * s0 + s1 * s1) + s2 * s2)
        cc = ((R[0] + R[4]) + R[8]) - 1.0
        re = re + np.arctan2(s, cc)
    with np.errstate(all="ignore"):
        scale = num / den
        sq = np.zeros(nw)
        for i in range(L):
            for c in (3, 7, 11):
                d = a[c][:, i] - scale * b[c][:, i]
                sq = sq + d * d
        ate = np.sqrt(sq) / float(L)
        kappa = absnum / np.abs(num)
    re = re / float(L)
    aligned = est[:nw].copy()
    with np.errstate(all="ignore"):
        for c in (3, 7, 11):
            aligned[:, c] = aligned[:, c] * scale
    e64 = np.stack([ate, re], axis=1)
    with np.errstate(all="ignore"):
        e32 = e64.astype(np.float32)
    return {"errors64": e64, "errors": e32, "scale": scale, "aligned": aligned, "compensated": comp, "kappa": kappa,
            "den": den, "degenerate": den == 0.0}


def stats(errors32):
    """(ATE mean, ATE std, RE mean, RE std) of float32 errors [nw,2]: the fp64 two-pass mean and population std; NaN for nw = 0"""
    x = np.asarray(errors32, np.float32).astype(np.float64).reshape(-1, 2)
    if len(x) == 0:
        return np.full(4, np.nan)
    with np.errstate(all="ignore"):
        m = x.sum(0) / len(x)
        sd = np.sqrt(((x - m) ** 2).sum(0) / len(x))
    return np.array([m[0], sd[0], m[1], sd[1]])


def stats_tol(errors32):
    """Two fp64 summations of the same nw numbers in different orders differ by at most nw 2^-53 sum|x| <= nw^2 2^-53 max|x|
    before the division by nw: nw 2^-53 max|x| on the mean.  The deviations inherit that shift and add their own summation:
    the std moves by at most the shift of the mean plus nw 2^-53 max|x| again, taken four times over for the square root's
    conditioning at a spread that is not small against the values (asserted where this is used: std >= max|x| / 1e3 or std == 0)."""
    x = np.abs(np.asarray(errors32, np.float64).reshape(-1, 2))
    if len(x) == 0:
        return np.zeros(4)
    t = len(x) * (U / 2) * x.max(0)
    return np.array([t[0], 8 * t[0], t[1], 8 * t[1]])


def spacing32(x):
    """the float32 spacing at |x|"""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


# RE near zero.  atan2(s, c) at c ~ 2 (a residual rotation near the identity) moves by ds / 2 for an error ds of s, and s is the
# norm of three differences of entries of R = est_R inv(gt_R).  An entry of R carries two 3x3 inverses and two 3x3 products (the
# compensation and the residual) on entries of size <= 1: at most 32 roundings of 2^-53; two entries per difference, the norm
# of three differences sqrt 3 times one: ds <= 2 sqrt(3) 32 2^-53, halved by atan2, and both sides of a comparison carry it:
# 2 sqrt(3) 32 2^-53 < 128 2^-53.  The mean over the L poses of a window has the same bound.
RE_FLOOR = 128 * 2.0 ** -53


def error_tol(errors32_ref):
    """[nw,2]: one float32 spacing of the value, plus RE_FLOOR on RE"""
    t = spacing32(errors32_ref)
    t[:, 1] += RE_FLOOR
    return t


def scale_tol(kappa):
    """relative: kappa 2^-52"""
    return kappa * U


def golden_scale_tol(kappa, L):
    """The restatement against the reference's numpy.sum / `@`: 3 L terms summed in another order, (3 L - 1) 2^-53 sum|terms|, and
    terms that carry the compensation's own rounding in another order, at most 8 roundings each on either factor:
    (3 L + 16) kappa 2^-52 relative, counting both the numerator and the (well-conditioned) denominator."""
    return (3 * L + 16) * kappa * U


def perturbed_input_tol(delta, L):
    """How far a window's compensated translations (as a vector of 3 L numbers) move when every entry of every pose of the
    estimate moves by at most delta -- for comparing results whose INPUT trajectories differ by a known rounding bound.  A
    compensated translation is Rinv (t_i - t_0): the difference moves by 2 delta per component, and Rinv (entries <= ~1, itself
    moved by ~3 delta per entry through the adjugate) multiplies a vector of 1-norm <= 3 L units of travel: per component
    3 (2 delta) + 3 delta 3 L, i.e. (9 L + 6) delta, times sqrt(3 L) for the norm of the vector.  ATE moves by that / L, the
    scale by that / |gt_t|, and RE (three differences of entries of est_R inv(gt_R), each moved by <= 18 delta) by less."""
    return (9 * L + 6) * delta * np.sqrt(3.0 * L)
