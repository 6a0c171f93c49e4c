"""Shared case families of the eight-point adjoint (dfepe_eight_point_bwd) and the one check() that the host build
(tests/test_eight_point_adjoint_ref_cpu.py) and the kernel (tests/test_eight_point_adjoint_gpu.py) both go through.  A case is a dict
of float32 numpy arrays, exactly what the C ABI is given: X, Y [B,N,2], w [S,B,N] or None, F_out, g_F [S,B,3,3], plus essential
(DFEPE_W8PT_FORCE_110), normalize (not DFEPE_W8PT_NO_HARTLEY), S, B, N, family.
Families:
  scene     a synthetic two-view scene per pair (pinhole camera f = 718, rotation ~ 0.1 rad, a general translation, depths 5 .. 35),
            0.5 .. 1 px of Gaussian noise on the pixels, then K^-1 points rounded to float32.  N in NS, sets in {1, 3}, the four flag
            combinations, weights none / uniform in [0.2, 1.2] / the same with some exact zeros (N >= 10, so that nine rows stay).
            F_out is the float32 of the restatement's forward in the fit kernel's gauge (largest-magnitude entry positive), negated
            for every other problem so that the orientation step is exercised; g_F is standard normal.
            A pair is drawn again (next attempt of its own generator) until, for every weight set,
            (lam_8 - lam_9) / lam_1 >= 1e-6 and, without FORCE_110, (s2 - s3) / s1 >= 1e-3: the condition under which the bound holds.
  exact     the same scene without noise, FORCE_110 | NO_HARTLEY: an essential matrix up to the float32 rounding of the points,
            s1 = s2 to about 1e-7, where svd_backward divides by s1^2 - s2^2.  No condition; held to the 50-digit twin (g_X, g_Y at the
            bound below; g_w, which is the fit's residual there, with the interior term exact_interior() derives).
  nonfinite scene, B = 3, one NaN coordinate in pair 1 only: for the locality rule.
The bound of check(): per problem and per output tensor |g - g_ref| <= 2^-22 max |g_ref|.  Inputs are identical float32, the output
is rounded once (2^-24 relative to its own size, at most that of the largest entry), the interior fp64 arithmetic stays below
1e-9 max |g_ref| under the condition above (asserted against the twin); the rest is margin."""
import functools
import zlib

import numpy as np

import eight_point_adjoint_ref as er

F32 = np.float32
NS = (8, 9, 10, 16, 63, 64, 65, 129)
FLAG_COMBOS = ((False, True), (False, False), (True, True), (True, False))  # (essential, normalize)
BATCHES = (1, 3, 5, 70)
MIN_GAP_LAM, MIN_GAP_S = 1e-6, 1e-3
BOUND = 2.0 ** -22
TWIN_BOUND = 1e-9
K = np.array([[718.0, 0.0, 607.0], [0.0, 718.0, 185.0], [0.0, 0.0, 1.0]])


def scene_pair(N, rng, noise):
    """One pair's K^-1 points [N,2] x 2, float32."""
    Ki = np.linalg.inv(K)
    uv = np.stack((rng.uniform(0, 1241, N), rng.uniform(0, 376, N), np.ones(N)), 1)
    P1 = (uv @ Ki.T) * rng.uniform(5, 35, (N, 1))
    om = 0.1 * rng.standard_normal(3)
    th = np.linalg.norm(om)
    k = om / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    t = rng.standard_normal(3) * np.array([1.0, 0.5, 1.0])
    P2 = P1 @ R.T + t

    def pixels(Q):
        x = Q @ K.T
        return x[:, :2] / x[:, 2:] + noise * rng.uniform(0.5, 1.0) * rng.standard_normal((N, 2))

    def normalised(x):
        return ((np.concatenate((x, np.ones((N, 1))), 1) @ Ki.T)[:, :2]).astype(F32)

    return normalised(pixels(P1)), normalised(pixels(P2))


def _weights(S, N, wfam, rng):
    if wfam == "none":
        return None
    w = rng.uniform(0.2, 1.2, (S, N)).astype(F32)
    if wfam == "zeros":
        for s in range(S):
            w[s, rng.choice(N, max(1, min(N - 9, N // 8)), replace=False)] = 0.0
    return w


def make(N, S, essential, normalize, wfam, B, family="scene"):
    assert wfam in ("none", "range", "zeros") and (wfam != "zeros" or N >= 10) and (wfam != "none" or S == 1)
    X, Y = np.empty((B, N, 2), F32), np.empty((B, N, 2), F32)
    w = None if wfam == "none" else np.empty((S, B, N), F32)
    tag = zlib.crc32(f"{N}-{S}-{int(essential)}{int(normalize)}-{wfam}-{family}".encode())
    for b in range(B):
        for attempt in range(200):
            rng = np.random.default_rng([tag, b, attempt])
            X[b], Y[b] = scene_pair(N, rng, 0.0 if family == "exact" else 1.0)
            wb = _weights(S, N, wfam, rng)
            if family == "exact":
                break
            gaps = [er.problem(X[b], Y[b], None if wb is None else wb[s], essential, normalize, None, None) for s in range(S)]
            if all(g.gap_lam >= MIN_GAP_LAM and (essential or g.gap_s >= MIN_GAP_S) for g in gaps):
                break
        else:
            raise AssertionError(f"no conditioned pair in 200 attempts: N={N} S={S} {wfam}")
        if w is not None:
            w[:, b] = wb
    out, _, _ = er.forward(X, Y, w, essential, normalize)
    flat = out.reshape(S, B, 9)
    top = np.take_along_axis(flat, np.abs(flat).argmax(-1)[..., None], -1)[..., None]
    out = out * np.sign(top)                                   # the fit kernel's gauge
    out[(np.arange(S)[:, None] + np.arange(B)[None, :]) % 2 == 1] *= -1.0
    g_F = np.random.default_rng([tag, 7]).standard_normal((S, B, 3, 3)).astype(F32)
    case = {"family": family, "X": X, "Y": Y, "w": w, "F_out": np.ascontiguousarray(out, F32), "g_F": g_F, "essential": essential,
            "normalize": normalize, "S": S, "B": B, "N": N, "wfam": wfam}
    if family == "nonfinite":
        case["X"][1, N // 2, 0] = np.nan
    return case


def flags_of(case):
    return 4 | 8 | (16 if case["essential"] else 0) | (0 if case["normalize"] else 32)


def name_of(case):
    return (f"{case['family']}-N{case['N']}-S{case['S']}-B{case['B']}-{'E' if case['essential'] else 'F'}"
            f"{'h' if case['normalize'] else 'n'}-{case['wfam']}")


@functools.lru_cache(maxsize=None)
def scene_cases():
    """Every N x flag combination once, the sets, the weight family and the batch size cycling, plus four cases that pair the batch
    sizes with the other number of sets."""
    out = []
    for iN, N in enumerate(NS):
        for iF, (essential, normalize) in enumerate(FLAG_COMBOS):
            S = (1, 3)[(iN + iF) % 2]
            fams = ("none", "range", "zeros") if S == 1 else ("range", "zeros")
            wfam = fams[(iN // 2 + iF) % len(fams)]
            if wfam == "zeros" and N < 10:
                wfam = "range"
            out.append(make(N, S, essential, normalize, wfam, BATCHES[(3 * iN + iF) % 4]))
    out.append(make(10, 3, True, True, "zeros", 1))
    out.append(make(16, 1, False, True, "none", 3))
    out.append(make(65, 3, True, False, "range", 5))
    out.append(make(64, 1, True, True, "zeros", 70))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def exact_cases():
    return (make(16, 1, True, False, "none", 2, family="exact"), make(65, 1, True, False, "range", 2, family="exact"))


@functools.lru_cache(maxsize=None)
def nonfinite_case():
    return make(65, 3, True, True, "range", 3, family="nonfinite")


def golden_cases():
    """The inputs of tests/golden/eight_point_adjoint.npz: pair 0 of scene cases, N in {9, 10, 16, 65} (N = 9 is the smallest N at
    which the reference's some=True SVD still has a ninth right singular vector), both solvers, `normalize` both ways, W None and
    torch.diag(ws).  Each: X, Y [N,2], ws [N] or None, essential, normalize, g [3,3] (the fixed upstream matrix)."""
    out = []
    for N in (9, 10, 16, 65):
        for essential in (False, True):
            for normalize in (True, False):
                for wfam in ("none", "range"):
                    c = make(N, 1, essential, normalize, wfam, 1)
                    out.append({"X": c["X"][0], "Y": c["Y"][0], "ws": None if c["w"] is None else c["w"][0, 0], "essential": essential,
                                "normalize": normalize, "g": c["g_F"][0, 0], "N": N})
    return out


def reference(case):
    """The restatement of the case (cached on it); for the exact family the 50-digit twin, problem by problem (S = 1)."""
    if "_ref" not in case:
        with np.errstate(all="ignore"):
            r = er.adjoint(case["X"], case["Y"], case["w"], case["essential"], case["normalize"], case["F_out"], case["g_F"])
        if case["family"] == "exact":
            assert case["S"] == 1
            for b in range(case["B"]):
                r.gX[b], r.gY[b], r.gw[0, b] = er.twin(case["X"][b], case["Y"][b], None if case["w"] is None else case["w"][0, b],
                                                       case["essential"], case["normalize"], case["F_out"][0, b], case["g_F"][0, b])
        case["_ref"] = r
    return case["_ref"]


def _within(name, what, got, ref, skip, interior=None):
    """|got - ref| <= 2^-22 max |ref| (+ interior[at], the exact family's g_w only) per leading index (a problem, or a pair for the
    summed point gradients)."""
    got = np.asarray(got)
    assert got.dtype == F32 and got.shape == ref.shape, (name, what, got.dtype, got.shape)
    lead = ref.shape[:-2] if what != "g_w" else ref.shape[:-1]
    for at in np.ndindex(*lead):
        if at[-1] in skip:
            continue
        top = np.abs(ref[at]).max()
        err = np.abs(got[at].astype(np.float64) - ref[at]).max()
        extra = 0.0 if interior is None else interior[at]
        assert extra <= MAX_INTERIOR * top, (name, what, at, "interior term / max", float(extra / top))
        assert np.isfinite(top) and err <= BOUND * top + extra, (name, what, at, float(err), float(top), float(extra))


JACOBI_ROUNDINGS = 8 * 8 * 6  # see exact_interior()
MAX_INTERIOR = 2.0 ** -15     # of max |g_w|: an interior term above it would hold nothing, and fails


def exact_interior(case, r):
    """The exact family's g_w = 2 w (a . f)(a . u) is the residual a . f of a noise-free fit, about 1e-8 (the float32 rounding of the
    points), times a . u, so an ABSOLUTE error df of the unit vector f is magnified by |a| / |a . f|, about 1e8, where elsewhere it
    is not: the 2^-22 of the bound leaves room for 2^-22 / 1e8 = 2e-15 of f, twenty units of fp64.  What fp64 Jacobi delivers for a
    unit eigenvector, whatever the gap: a column of the accumulated rotations is touched by 8 rotations per sweep, a 9x9 converges
    in about 8 sweeps, and one rotation of an element is two products, a sum and the rounded (c, s), 6 roundings of at most 2^-53
    of a number below 1: |df| <= 8 * 8 * 6 * 2^-53 = 4.3e-14, added up linearly.  To first order |d g_w,i| <= 2 w_i |a_i| |a_i . u|
    |df| (restatement: gw_df).  [S,B].  On the cases this is 5e-6 .. 2.3e-5 of max |g_w| (asserted below 2^-15 of it, so that it can
    never hold nothing); the host build's error is 9e-8 .. 1.1e-6 there.
    Not included: the rounding of M9 = A^T A itself, which Davis-Kahan lets through as N 2^-53 lam_1 / (lam_8 - lam_9), 0.005 .. 0.85
    of max |g_w| here: six orders above anything that occurs, so as a term of a test it would hold nothing.  An evaluation in which
    that worst case materialised would fail this check."""
    return JACOBI_ROUNDINGS * 2.0 ** -53 * r.gw_df.max(-1)


def check(case, got):
    """got: dict with any of g_X, g_Y [B,N,2], g_w [S,B,N] (float32; None or absent: not checked)."""
    r = reference(case)
    skip = {1} if case["family"] == "nonfinite" else set()
    name = name_of(case)
    if got.get("g_X") is not None:
        _within(name, "g_X", got["g_X"], r.gX, skip)
    if got.get("g_Y") is not None:
        _within(name, "g_Y", got["g_Y"], r.gY, skip)
    if got.get("g_w") is not None:
        _within(name, "g_w", got["g_w"], r.gw, skip, exact_interior(case, r) if case["family"] == "exact" else None)
    return r
