"""Case table of the seven small pose helpers (dfepe_geo_misc, csrc/geom.hip: geo_misc_kernel), shared by the host test of the
reference (tests/test_pose_helper_ref_cpu.py) and the GPU edge suite (tests/test_pose_helpers_edges_gpu.py).  Deterministic: every
family is drawn from numpy.random.default_rng(SEED + its own offset) and rounded to float32 once, here; the float64 restatement of
tests/pose_helper_ref.py is computed once per process per kind and shared (pool() / expected()).

Bounds ("Pose helpers and the validation summary held to fp64"):
  kinds 0, 1, 2, 5, 6   |got - float32(ref)| <= 1 float32 ulp of float32(ref) + the reference's own conditioning term
  kind 3                |got - ref| <= 4 * 2^-24 + 4 K_SVD3 2^-52 s1 / (s2 - s3) per entry; singular values (1, 1, 0) within 1e-6
  kind 4                R1, R2 in SO(3) and |t| = 1 within 1e-6; {R1, R2} and +-t against the reference to the bound of kind 3
K_SVD3 is the largest distance, in units of 2^-52 s1 / (s2 - s3), that the HOST build of svd3_closed (tests/emu/emu_svd3.cpp) was seen
at from np.linalg.svd over every family below; the factor 4 covers the device's reciprocal / square-root seeds differing from the
host emulation's."""
import functools

import numpy as np

import pose_branch_cases as pbc
import pose_helper_ref as ref

SEED = 7100
LAUNCH_SIZES = (0, 1, 63, 64, 255, 256, 257, 1000)  # the grid is (n + 255) / 256 workgroups of 256 lanes
ANGLES_DEG = (0.0, 1e-4, 1e-2, 1.0, 90.0, 179.0, 180.0 - 1e-2, 180.0 - 1e-4, 180.0)
SCALES = {"2^-20": 2.0 ** -20, "1e-6": 1e-6, "1e+6": 1e6}
K_SVD3 = 8.1e4     # measured on the host: 80654.8 (small_gap; at most 3.5 in every other family): tests/test_pose_helper_ref_cpu.py prints it
SVD3_MARGIN = 4.0  # device seeds against the host emulation's
SV_TOL = 1e-6      # singular values of a projection / orthonormality of a decomposition (float32 output of unit matrices)
DEGENERATE = ("rank1", "zero")  # no projection is defined: invariants only
OUT_WIDTH = {0: 4, 1: 1, 2: 1, 3: 9, 4: 21, 5: 9, 6: 9}


def rodrigues(axis, angle):
    """Rotation by `angle` radians about `axis` (any length), float64."""
    k = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    Kx = skew(k)
    return np.eye(3) + np.sin(angle) * Kx + (1.0 - np.cos(angle)) * (Kx @ Kx)


def skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def _rng(k):
    return np.random.default_rng(SEED + k)


def _f32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(np.float32))


def _random_rotation(g):
    return rodrigues(g.standard_normal(3), g.uniform(0.1, 3.0))


# ---- rotations (kind 0) ---------------------------------------------------------------------------------------------------------
EXACT_ROTATIONS = {  # every entry 0 or +-1: the branch predicates M22 < 0, M00 > M11, M00 < -M11 are decided by exact ties
    "identity": np.eye(3),
    "x180": np.diag([1.0, -1.0, -1.0]), "y180": np.diag([-1.0, 1.0, -1.0]), "z180": np.diag([-1.0, -1.0, 1.0]),
    "x90": np.array([[1.0, 0, 0], [0, 0, -1], [0, 1, 0]]), "x-90": np.array([[1.0, 0, 0], [0, 0, 1], [0, -1, 0]]),    # M22 == 0
    "y90": np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]]), "y-90": np.array([[0.0, 0, -1], [0, 1, 0], [1, 0, 0]]),    # M22 == 0
    "z90": np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]]), "z-90": np.array([[0.0, 1, 0], [-1, 0, 0], [0, 0, 1]]),    # M00 == -M11 == 0
    "xy180": np.array([[0.0, 1, 0], [1, 0, 0], [0, 0, -1]]),   # 180 degrees about (1, 1, 0): M22 < 0 and M00 == M11
    "xz180": np.array([[0.0, 0, 1], [0, -1, 0], [1, 0, 0]]),   # about (1, 0, 1): M22 == 0, M00 == 0 < -M11 == 1
    "yz180": np.array([[-1.0, 0, 0], [0, 0, 1], [0, 1, 0]]),   # about (0, 1, 1): M22 == 0, M00 == -1 < -M11 == 0
    "cyc": np.array([[0.0, 0, 1], [1, 0, 0], [0, 1, 0]]), "cyc'": np.array([[0.0, 1, 0], [0, 0, 1], [1, 0, 0]]),     # 120 degrees, zero diagonal
}
# what the trace method gives for them, written out (s = sqrt(1/2))
_S = np.sqrt(0.5)
EXACT_QUATERNIONS = {
    "identity": (1, 0, 0, 0), "x180": (0, 1, 0, 0), "y180": (0, 0, 1, 0), "z180": (0, 0, 0, 1),
    "x90": (_S, _S, 0, 0), "x-90": (_S, -_S, 0, 0), "y90": (_S, 0, _S, 0), "y-90": (_S, 0, -_S, 0), "z90": (_S, 0, 0, _S), "z-90": (_S, 0, 0, -_S),
    "xy180": (0, _S, _S, 0), "xz180": (0, _S, 0, _S), "yz180": (0, 0, _S, _S), "cyc": (0.5, 0.5, 0.5, 0.5), "cyc'": (0.5, -0.5, -0.5, -0.5),
}


@functools.lru_cache(maxsize=None)
def rotations():
    """name -> [n,3,3] float32.  branch0..2: 100..170 degrees about +-(e_x, e_y, e_z) + 0.15 N(0, I), the sign alternating (both states
    of the q0 >= 0 flip); branch3: 1..60 degrees about random axes; exact: EXACT_ROTATIONS; rounded: random rotations, which after the
    float32 rounding are orthonormal to ~1e-7 only; pose_branch: the 42 ground-truth rotations of tests/pose_branch_cases.py."""
    g = _rng(0)
    fam = {}
    for ax in range(3):
        Rs, sign = [], 1.0
        for deg in (100.0, 130.0, 150.0, 170.0):
            for _ in range(3):
                Rs.append(rodrigues(sign * np.eye(3)[ax] + 0.15 * g.standard_normal(3), np.radians(deg)))
                sign = -sign
        fam[f"branch{ax}"] = _f32(Rs)
    fam["branch3"] = _f32([rodrigues(g.standard_normal(3), np.radians(g.uniform(1.0, 60.0))) for _ in range(12)])
    fam["exact"] = _f32(list(EXACT_ROTATIONS.values()))
    fam["rounded"] = _f32([_random_rotation(g) for _ in range(24)])
    fam["pose_branch"] = np.ascontiguousarray(pbc.make_cases().R_gt.numpy().reshape(-1, 3, 3))
    return fam


# ---- rotation pairs (kind 1) ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def angle_pairs():
    """(R0 [n,3,3], R1 [n,3,3] float32, generating angle [n] in degrees): R0 = R(axis, angle) Rb, R1 = Rb for three random axes and
    bases Rb per angle of ANGLES_DEG, both rounded to float32 (at 0 degrees R0 is R1 bit for bit); last, the identity against itself."""
    g = _rng(1)
    R0, R1, deg = [], [], []
    for a in ANGLES_DEG:
        for _ in range(3):
            Rb = _random_rotation(g)
            R0.append(rodrigues(g.standard_normal(3), np.radians(a)) @ Rb)
            R1.append(Rb)
            deg.append(a)
    R0.append(np.eye(3)); R1.append(np.eye(3)); deg.append(0.0)
    return _f32(R0), _f32(R1), np.array(deg)


# ---- vector pairs (kind 2) ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def vector_pairs():
    """[(name, v1 [3] float32, v2 [3] float32, exact float32 result or None)].  The exact results are what the formula gives: a zero
    vector makes the cosine 0; at norm 1e12 the 1e-10 terms are absorbed and the cosine of equal / opposite vectors is +-1 exactly.
    At norm 1 they are not absorbed: equal unit vectors have the cosine 1 / (1 + 3e-10) and the reference's 1.4e-3 degrees."""
    g = _rng(2)
    out = []
    big = np.float32(1e12)
    for k in range(3):
        e = np.eye(3, dtype=np.float32)[k]
        out += [(f"equal_1e12[{k}]", big * e, big * e, 0.0), (f"opposite_1e12[{k}]", big * e, -big * e, 180.0),
                (f"orthogonal_axes[{k}]", e, np.eye(3, dtype=np.float32)[(k + 1) % 3], 90.0)]
    for k in range(4):
        v = _f32(g.standard_normal(3))
        u = _f32(np.cross(v.astype(np.float64), g.standard_normal(3)))
        z = np.zeros(3, np.float32)
        out += [(f"equal[{k}]", v, v.copy(), None), (f"opposite[{k}]", v, -v, None), (f"orthogonal[{k}]", v, u, None),
                (f"zero_first[{k}]", z, v, 90.0), (f"zero_second[{k}]", v, z, 90.0),
                (f"tiny[{k}]", _f32(1e-12 * v.astype(np.float64)), u, None), (f"tiny_both[{k}]", _f32(1e-12 * v.astype(np.float64)), _f32(1e-12 * u.astype(np.float64)), None),
                (f"huge[{k}]", _f32(1e12 * v.astype(np.float64)), u, None), (f"huge_both[{k}]", _f32(1e12 * v.astype(np.float64)), _f32(-1e12 * v.astype(np.float64) + 1e11 * u), None),
                (f"tiny_huge[{k}]", _f32(1e-12 * v.astype(np.float64)), _f32(1e12 * v.astype(np.float64)), None)]
        for deg, name in ((1e-3, "near_parallel"), (180.0 - 1e-3, "near_antiparallel")):
            w = rodrigues(u.astype(np.float64), np.radians(deg)) @ v.astype(np.float64)
            out.append((f"{name}[{k}]", v, _f32(w), None))
        out.append((f"generic[{k}]", v, _f32(g.standard_normal(3)), None))
    out.append(("zero_both", np.zeros(3, np.float32), np.zeros(3, np.float32), 90.0))
    return out


# ---- essential-like matrices (kinds 3, 4) ---------------------------------------------------------------------------------------
N_POSES = 12


@functools.lru_cache(maxsize=None)
def poses():
    """The generating (R [n,3,3], t [n,3] unit) of the txR families, float64."""
    g = _rng(3)
    R = np.stack([_random_rotation(g) for _ in range(N_POSES)])
    t = g.standard_normal((N_POSES, 3))
    return R, t / np.linalg.norm(t, axis=1, keepdims=True)


def _with_singular_values(g, s):
    U, _, Vt = np.linalg.svd(g.standard_normal((3, 3)))
    return U @ np.diag(s) @ Vt


@functools.lru_cache(maxsize=None)
def essentials():
    """name -> [n,3,3] float32.
      txR                [t]x R of poses(), rounded to float32: s1 == s2 to ~1e-7, s3 ~ 1e-8
      txR*2^-20, *1e-6, *1e+6   the same in float64 times the factor, then rounded (the power of two is exact)
      axis               [e_k]x and [-e_k]x with R = I: entries 0 and +-1, every tie of the closed form's selects is exact
      generic            full rank, singular values (1, u, v) with (u - v) >= 1e-2 drawn at random, |E| scaled by 10^U(-2, 2)
      small_gap          singular values (1, 0.5 + 0.5e-6, 0.5 - 0.5e-6): (s2 - s3) / s1 = 1e-6
      rank1              outer products a b^T (random, and e_j e_k^T)
      zero               the zero matrix"""
    g = _rng(4)
    R, t = poses()
    E = np.stack([skew(t[k]) @ R[k] for k in range(N_POSES)])
    fam = {"txR": _f32(E)}
    for name, s in SCALES.items():
        fam[f"txR*{name}"] = _f32(E * s)
    fam["axis"] = _f32([sg * skew(np.eye(3)[k]) for k in range(3) for sg in (1.0, -1.0)])
    gen = []
    while len(gen) < 16:
        u, v = sorted(g.uniform(0.02, 1.0, 2), reverse=True)
        if u - v >= 2e-2:
            gen.append(_with_singular_values(g, [1.0, u, v]) * 10.0 ** g.uniform(-2.0, 2.0))
    fam["generic"] = _f32(gen)
    fam["small_gap"] = _f32([_with_singular_values(g, [1.0, 0.5 + 0.5e-6, 0.5 - 0.5e-6]) for _ in range(8)])
    r1 = [np.outer(g.standard_normal(3), g.standard_normal(3)) for _ in range(6)]
    r1 += [np.outer(np.eye(3)[j], np.eye(3)[k]) for j, k in ((0, 0), (1, 2), (2, 1))] + [1e-3 * np.outer(r1[0][0], r1[0][0])]
    fam["rank1"] = _f32(r1)
    fam["zero"] = np.zeros((1, 3, 3), np.float32)
    return fam


# ---- 4x4 motions (kind 6) -------------------------------------------------------------------------------------------------------
MAX_COND = 1e3


@functools.lru_cache(maxsize=None)
def motions():
    """name -> [n,4,4] float32: rigid (|t| ~ 1), rigid_far (|t| = 1e3), general (I + 0.5 N(0, 1) on all 16 entries, so the last row is
    not (0, 0, 0, 1); redrawn until the 2-norm condition number of the float32 matrix is <= MAX_COND: up to 45), general_ill (random
    orthogonal factors around singular values from 1 down to 1 / c, c log-uniform in [1e2, 0.9e3]: the upper decade of what is allowed)."""
    g = _rng(5)

    def rigid(scale):
        m = np.eye(4)
        m[:3, :3] = _random_rotation(g)
        v = g.standard_normal(3)
        m[:3, 3] = scale * v / np.linalg.norm(v)
        return m

    fam = {"rigid": _f32([rigid(1.0) for _ in range(12)]), "rigid_far": _f32([rigid(1e3) for _ in range(12)])}
    gen = []
    while len(gen) < 12:
        m = _f32(np.eye(4) + 0.5 * g.standard_normal((4, 4)))
        if np.linalg.cond(m.astype(np.float64)) <= MAX_COND:
            gen.append(m)
    fam["general"] = np.stack(gen)
    ill = []
    for _ in range(8):
        c = 10.0 ** g.uniform(2.0, np.log10(900.0))
        U, _, Vt = np.linalg.svd(g.standard_normal((4, 4)))
        ill.append(U @ np.diag(np.geomspace(1.0, 1.0 / c, 4)) @ Vt)
    fam["general_ill"] = _f32(ill)
    return fam


# ---- congruences (kind 5) -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def congruences():
    """(F [n,3,3], A [n,3,3]) float32: unit-Frobenius F with A = T K of a 1241 x 376 image (entries from 1e-3 to 7e2, the call the
    pipeline makes), then random F and A, then A = I and F = 0."""
    g = _rng(6)
    F, A = [], []
    T = np.array([[2.0 / 1241, 0, -1], [0, 2.0 / 376, -1], [0, 0, 1]])
    for _ in range(8):
        f = g.standard_normal((3, 3))
        K = np.array([[718.0 + g.uniform(-20, 20), 0, 607.0 + g.uniform(-5, 5)], [0, 718.0 + g.uniform(-20, 20), 185.0 + g.uniform(-5, 5)], [0, 0, 1]])
        F.append(f / np.linalg.norm(f)); A.append(T @ K)
    for _ in range(8):
        F.append(g.standard_normal((3, 3))); A.append(g.standard_normal((3, 3)))
    F += [g.standard_normal((3, 3)), np.zeros((3, 3))]
    A += [np.eye(3), g.standard_normal((3, 3))]
    return _f32(F), _f32(A)


# ---- one pool of items per kind, and its restatement, computed once -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pool(kind):
    """(in0 [n,w0] float32, in1 [n,w1] float32 or None, family name of every item)."""
    cat = lambda fam, w: (np.concatenate([v.reshape(-1, w) for v in fam.values()]), [k for k, v in fam.items() for _ in range(len(v))])
    if kind == 0:
        x, names = cat(rotations(), 9)
        return x, None, names
    if kind == 1:
        R0, R1, _ = angle_pairs()
        return R0.reshape(-1, 9), R1.reshape(-1, 9), ["angle_pairs"] * len(R0)
    if kind == 2:
        vp = vector_pairs()
        return np.stack([v[1] for v in vp]), np.stack([v[2] for v in vp]), [v[0] for v in vp]
    if kind in (3, 4):
        x, names = cat(essentials(), 9)
        return x, None, names
    if kind == 5:
        F, A = congruences()
        return F.reshape(-1, 9), A.reshape(-1, 9), ["congruences"] * len(F)
    x, names = cat(motions(), 16)
    return x, None, names


def family_slice(kind, name):
    names = pool(kind)[2]
    idx = [i for i, n in enumerate(names) if n == name]
    assert idx and idx == list(range(idx[0], idx[-1] + 1))
    return slice(idx[0], idx[-1] + 1)


def projection_tolerance(E32, margin=SVD3_MARGIN):
    """Per-entry bound of kind 3 (and 4) for one float32 matrix; inf where no projection is defined."""
    gap = ref.relative_gap(E32)
    return 4.0 * 2.0 ** -24 + margin * K_SVD3 * ref.EPS64 / gap if gap > 0.0 else np.inf


@functools.lru_cache(maxsize=None)
def expected(kind):
    """The restatement of every item of pool(kind): dict of arrays, leading dimension n.
      kinds 0, 1, 2, 5, 6   want [n,w] float64, cond [n,w]
      kind 3                want [n,9], tol [n]
      kind 4                R1, R2 [n,9], t [n,3], tol [n]"""
    in0, in1, names = pool(kind)
    n = len(in0)
    if kind == 0:
        r = [ref.quat(x) for x in in0]
        return {"want": np.stack([q for q, _, _, _ in r]), "cond": np.stack([c for _, _, _, c in r]), "branch": np.array([b for _, b, _, _ in r]),
                "flip": np.array([f for _, _, f, _ in r])}
    if kind in (1, 2):
        f = ref.rotation_angle if kind == 1 else ref.vector_angle
        r = np.array([f(in0[i], in1[i]) for i in range(n)])
        return {"want": r[:, :1], "cond": r[:, 1:]}
    if kind == 3:
        return {"want": np.stack([ref.project(x).reshape(9) for x in in0]), "tol": np.array([projection_tolerance(x) for x in in0])}
    if kind == 4:
        r = [ref.decompose(x) for x in in0]
        return {"R1": np.stack([a.reshape(9) for a, _, _ in r]), "R2": np.stack([b.reshape(9) for _, b, _ in r]), "t": np.stack([t for _, _, t in r]),
                "tol": np.array([projection_tolerance(x) for x in in0])}
    if kind == 5:
        r = [ref.congruence(in0[i], in1[i]) for i in range(n)]
        return {"want": np.stack([a.reshape(9) for a, _ in r]), "cond": np.stack([c.reshape(9) for _, c in r])}
    r = [ref.camera_rotation(x) for x in in0]
    return {"want": np.stack([a.reshape(9) for a, _ in r]), "cond": np.stack([np.full(9, c) for _, c in r])}


def rounded_bound(want, cond):
    """float32(want) and the bound 1 float32 ulp of it + cond."""
    w32 = np.asarray(want, dtype=np.float64).astype(np.float32)
    return w32, ref.ulp32(w32) + cond


def check_so3(R, tag):
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    assert np.abs(R @ R.T - np.eye(3)).max() <= SV_TOL and abs(np.linalg.det(R) - 1.0) <= SV_TOL, tag


def check(kind, got, idx, tag=""):
    """got [m,w]: what the device (or the host build) returned for the items idx of pool(kind).  Returns the largest error in units
    of its bound (the invariants of kinds 3 and 4 are asserted on the way)."""
    got = np.asarray(got)
    idx = np.arange(len(pool(kind)[0]))[idx] if isinstance(idx, slice) else np.asarray(idx)
    assert got.dtype == np.float32 and got.shape == (len(idx), OUT_WIDTH[kind]), (tag, got.shape)
    ex, names = expected(kind), pool(kind)[2]
    worst = 0.0
    if kind in (0, 1, 2, 5, 6):
        w32, bound = rounded_bound(ex["want"][idx], ex["cond"][idx])
        err = np.abs(got.astype(np.float64) - w32.astype(np.float64))
        bad = ~(err <= bound)  # a NaN fails
        assert not bad.any(), f"{tag} kind {kind}: item {names[idx[np.argwhere(bad)[0][0]]]} off by {err[bad].max():.3e}, bound {bound[bad].min():.3e}"
        return float((err / bound).max()) if len(idx) else 0.0
    for j, i in enumerate(idx):
        g = got[j].astype(np.float64)
        what = f"{tag} kind {kind}: item {i} ({names[i]})"
        assert np.isfinite(g).all(), what
        degenerate = names[i] in DEGENERATE
        if kind == 3:
            assert np.abs(np.linalg.svd(g.reshape(3, 3), compute_uv=False) - [1.0, 1.0, 0.0]).max() <= SV_TOL, what
            if not degenerate:
                e = np.abs(g - ex["want"][i]).max()
                assert e <= ex["tol"][i], f"{what}: {e:.3e} > {ex['tol'][i]:.3e}"
                worst = max(worst, e / ex["tol"][i])
        else:
            check_so3(g[0:9], what + " R1")
            check_so3(g[9:18], what + " R2")
            assert abs(np.linalg.norm(g[18:21]) - 1.0) <= SV_TOL, what
            if not degenerate:
                direct = max(np.abs(g[0:9] - ex["R1"][i]).max(), np.abs(g[9:18] - ex["R2"][i]).max())
                swapped = max(np.abs(g[0:9] - ex["R2"][i]).max(), np.abs(g[9:18] - ex["R1"][i]).max())
                te = min(np.abs(g[18:21] - ex["t"][i]).max(), np.abs(g[18:21] + ex["t"][i]).max())
                e = max(min(direct, swapped), te)
                assert e <= ex["tol"][i], f"{what}: {e:.3e} > {ex['tol'][i]:.3e}"
                worst = max(worst, e / ex["tol"][i])
    return worst


def batch(kind, n, offset=0):
    """n items of pool(kind), cyclically from `offset`: (in0, in1, idx)."""
    in0, in1, _ = pool(kind)
    idx = (np.arange(n) + offset) % len(in0)
    return in0[idx], (None if in1 is None else in1[idx]), idx
