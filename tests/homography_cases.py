"""Shared inputs of the homography tests and the one check() both the CPU tests (host build of csrc/homography_math.h) and the GPU
tests (csrc/homography.hip) go through.  Every pair is generated from a seed; the restatement's answer (tests/homography_ref.py)
is computed once per (pair, settings) and cached for the session, and nothing mutates it.

Tolerances (measured by `python tests/homography_cases.py`, recorded in profiles/homography.md)
-------------------------------------------------------------------------------------------------
The yardstick is the fp64 restatement's own distance from its 50-digit twin on these case families, taken as the largest
difference of the transferred points over the pair's correspondences and the four image corners, in pixels
(homography_ref.max_transfer_diff).  The code under test is fp64 too, with another order of operations, and gets four times the
yardstick (the margin of tests/test_refcfg_gpu.py for "same precision, different operation order").
"""
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import homography_ref as hr  # noqa: E402
import ransac_ref as rr  # noqa: E402

HEIGHT, WIDTH = 240, 320
EPS = hr.DBL_EPSILON

# ---- measured yardsticks (restatement against its mpmath twin; `python tests/homography_cases.py` prints them) -------------
# 4-point solve: the distance grows with the sample's conditioning kappa = s1 / s8.  Over the 360 samples of the first 24
# iterations of every family below, compared at the hypothesis' own inliers, the largest dist / (kappa * eps) was 27533.5 px
# (a coordinate of ~320 px, the scales of the two normalisations and the division by w all multiply kappa * eps).
Y_SOLVE_PER_KAPPA_EPS = 27533.5
# refit over the inliers: the distance grows with the conditioning of the eigenvector, kappa_refit = e9 / (e2 - e1) of L^T L
# (homography_ref.refit).  Measured on well-supported winners (24 iterations), on the first model whatever it is (1 iteration:
# four to thirteen inliers, kappa_refit up to 2.5e5, corners sent far away) and on least squares over all points: the largest
# dist / (kappa_refit * eps) was 328232.2 px (the duplicates pair after one iteration); a well-supported winner with
# kappa_refit = 13 is thereby held to 4 * 328232.2 * 13 * eps = 3.8e-9 px.
Y_REFIT_PER_KAPPA_EPS = 328232.2
# refinement: no twin runs the loop; the yardstick is the restatement's own loop started from the twin's refit instead of its
# own: the largest distance beyond the slack of the iterations whose gain rounding decides (homography_ref.lm_ambiguous;
# ref(...)["lm_slack"] is added to the tolerance) was 328020.9 kappa_refit * eps px.
Y_REFINE_PER_KAPPA_EPS = 328020.9
MARGIN = 4.0


def tol_refit(kappa_refit):
    return MARGIN * Y_REFIT_PER_KAPPA_EPS * kappa_refit * EPS


def tol_refine(kappa_refit):
    return MARGIN * Y_REFINE_PER_KAPPA_EPS * kappa_refit * EPS


# transfer distances are rounded to fp32: half an ulp of the value on top of the fp64 evaluation
DIST_RTOL = 2.0 ** -23


def tol_solve(kappa):
    return MARGIN * Y_SOLVE_PER_KAPPA_EPS * kappa * EPS


# ---- pairs -----------------------------------------------------------------------------------------------------------------
def random_h(rng, persp=2e-4):
    a = rng.uniform(-0.25, 0.25)
    s = rng.uniform(0.8, 1.2)
    H = np.array([[s * math.cos(a), -s * math.sin(a), rng.uniform(-20, 20)], [s * math.sin(a), s * math.cos(a), rng.uniform(-20, 20)],
                  [rng.uniform(-persp, persp), rng.uniform(-persp, persp), 1.0]])
    H[0, 1] += rng.uniform(-0.05, 0.05)
    return H


def warp(H, xy):
    q = np.c_[xy, np.ones(len(xy))] @ np.asarray(H).T
    return q[:, :2] / q[:, 2:]


def synth(seed, N, outliers=0.0, noise=0.0, H=None):
    """[N,4] float32 matches of a 240 x 320 image under H (random when None), a share of outliers with a uniform target."""
    rng = np.random.default_rng(seed)
    H = random_h(rng) if H is None else np.asarray(H, np.float64)
    src = np.c_[rng.uniform(0, WIDTH - 1, N), rng.uniform(0, HEIGHT - 1, N)]
    dst = warp(H, src) + noise * rng.standard_normal((N, 2))
    k = int(round(outliers * N))
    if k:
        bad = rng.permutation(N)[:k]
        dst[bad] = np.c_[rng.uniform(0, WIDTH - 1, k), rng.uniform(0, HEIGHT - 1, k)]
    return np.c_[src, dst].astype(np.float32), H


def noise_pair(seed, N):
    rng = np.random.default_rng(seed)
    return rng.uniform(0, HEIGHT - 1, (N, 4)).astype(np.float32)


def collinear_pair(seed, N):
    """Every point on one line in both images: no sample passes checkSubset, no model."""
    rng = np.random.default_rng(seed)
    t = rng.permutation(N).astype(np.float64)
    return np.c_[2 * t + 1, t + 3, t + 5, 3 * t + 2].astype(np.float32)


def duplicate_pair(seed, N):
    m, _ = synth(seed, N, 0.3, 0.5)
    rng = np.random.default_rng(seed + 1)
    idx = rng.integers(0, N // 4, N)  # every row one of N/4 distinct correspondences
    return m[idx]


def sampler_stop_pair(seed, N):
    """A model at iteration 0, no sample at iteration 1: the four draws of iteration 0's first attempt are a good quadrilateral;
    every other row is one and the same correspondence, an outlier of that model.  Any later sample holds two copies of it (zero
    differences: collinear) unless it draws three of the four, which 1000 attempts at N = 200 do with probability 1 %."""
    s = rr.Stream(seed, 0)
    idx = []
    while len(idx) < 4:
        v = s.index(N)
        if v not in idx:
            idx.append(v)
    m = np.tile(np.array([[100.0, 100.0, 30.0, 200.0]], np.float32), (N, 1))
    quad = np.array([[10, 10], [300, 20], [290, 220], [20, 200]], np.float64)
    m[idx, :2] = quad
    m[idx, 2:] = quad + [5.0, -3.0]
    return m


def w_zero_pair(seed, N):
    """A strongly projective H whose line w = 0 (x = 128) crosses the image; row 0 lies on it, the others keep |w| >= 0.2."""
    H = np.array([[1.0, 0.02, 3.0], [-0.01, 1.0, -2.0], [-1.0 / 128.0, 0.0, 1.0]])
    rng = np.random.default_rng(seed)
    x = np.where(rng.random(N) < 0.7, rng.uniform(0, 100, N), rng.uniform(160, 319, N))
    src = np.c_[x, rng.uniform(0, HEIGHT - 1, N)]
    src[0] = [128.0, 77.0]
    dst = warp(H, np.where(src[:, :1] == 128.0, src + [1.0, 0.0], src))
    dst[0] = [50.0, 60.0]
    return np.c_[src, dst].astype(np.float32)


H_TRANSLATION = np.array([[1, 0, 12.5], [0, 1, -7.25], [0, 0, 1.0]])
H_AFFINE = np.array([[1.05, 0.08, 4.0], [-0.06, 0.97, 9.0], [1e-7, -2e-7, 1.0]])
H_PROJECTIVE = np.array([[0.9, 0.1, 10.0], [-0.05, 1.1, 5.0], [1.5e-3, -1.0e-3, 1.0]])

N_DEFAULT = 100


@functools.lru_cache(maxsize=None)
def pair(name, N=N_DEFAULT):
    """The named pair as a read-only [N,4] float32 array."""
    if name.startswith("synth"):  # synth_<outlier %>_<noise px * 10>_<seed>
        _, o, s, sd = name.split("_")
        m = synth(1000 + int(sd), N, int(o) / 100.0, int(s) / 10.0)[0]
    elif name == "noise":
        m = noise_pair(7, N)
    elif name == "translation":
        m = synth(11, N, 0.2, 0.5, H_TRANSLATION)[0]
    elif name == "affine":
        m = synth(12, N, 0.2, 0.5, H_AFFINE)[0]
    elif name == "projective":
        m = synth(13, N, 0.2, 0.5, H_PROJECTIVE)[0]
    elif name == "collinear":
        m = collinear_pair(14, N)
    elif name == "duplicates":
        m = duplicate_pair(15, N)
    elif name == "sampler_stop":
        m = sampler_stop_pair(0, N)
    elif name == "w_zero":
        m = w_zero_pair(16, N)
    else:
        raise KeyError(name)
    m.setflags(write=False)
    return m


SYNTH = tuple(f"synth_{o}_{s}_{i}" for i, (o, s) in enumerate((o, s) for o in (0, 30, 60) for s in (0, 5, 20)))
SPECIAL = ("noise", "translation", "affine", "projective", "duplicates", "w_zero")
FAMILIES = SYNTH + SPECIAL
SLOW_SAMPLER = ("collinear", "sampler_stop")  # 1000 attempts per iteration in the restatement: keep max_iters small
N_VALID = (0, 3, 4, 5, None)
# cv2's method = 0 is a plain least-squares fit.  With gross outliers among its points the restatement itself moves by up to
# 1e4 px between two starts 1e-9 px apart (measure() prints it), so there is nothing to hold a kernel to: it is compared on the
# outlier-free families.
ALL_POINTS_FAMILIES = SYNTH[:3]
# the settings every family is run at, on the host build and on the GPU alike: (threshold, confidence, max_iters, seed, flags)
SETTINGS = ((3.0, 0.995, 64, 0, 0), (1.0, 0.995, 64, 0, 0), (5.0, 0.5, 64, 3, 0), (-1.0, 1.0, 65, (1 << 64) - 1, hr.NO_REFINE))


def jobs():
    """(name, N, n, threshold, confidence, max_iters, seed, flags) of every pair both builds are held to."""
    out = [(name, N_DEFAULT, None, *s) for name in FAMILIES for s in SETTINGS]
    out += [(name, N_DEFAULT, None, 3.0, 0.995, 1, 0, f) for name in ALL_POINTS_FAMILIES for f in (hr.ALL_POINTS, hr.ALL_POINTS | hr.NO_REFINE)]
    out += [("synth_0_5_1", N_DEFAULT, n, 3.0, 0.995, 16, 0, f) for n in N_VALID for f in (0, hr.ALL_POINTS, hr.NO_REFINE)]
    out += [("collinear", 50, None, 3.0, 0.995, 3, 0, 0), ("sampler_stop", 200, None, 3.0, 0.995, 3, 0, 0)]
    return out


@functools.lru_cache(maxsize=None)
def hyps(name, N, n, seed, max_iters, route="qr"):
    m = pair(name, N)
    n = N if n is None else n
    return tuple(hr.hypotheses(m[:n], seed, max_iters, route)) if n > 4 else ()


@functools.lru_cache(maxsize=None)
def ref(name, N=N_DEFAULT, n=None, threshold=3.0, confidence=0.995, max_iters=64, seed=0, flags=0, route="qr"):
    """The restatement's answer for one pair and one setting (cached; the hypotheses are shared between thresholds, confidences
    and shorter runs of the same stream)."""
    h = None
    nn = N if n is None else n
    if nn > 4 and not flags & hr.ALL_POINTS:
        h = list(hyps(name, N, n, seed, max_iters, route))
    return hr.estimate(pair(name, N), n, threshold, confidence, max_iters, seed, flags, route, hyps=h)


# ---- the one check ---------------------------------------------------------------------------------------------------------
def _h(x):
    return np.asarray(x, np.float64).reshape(3, 3)


def check(got, r, m, threshold, confidence=0.995, what=""):
    """got: dict of one pair's outputs from the code under test -- table (or None), best, best_k, iters, H_model, mask, and where
    the run has them H_refit (a NO_REFINE run's H_out), H_out, S0, S1; r: ref(...) of the same pair and settings; m: the pair.
    Prints each figure before it asserts.  Returns 'exact' or 'ambiguous'."""
    n = r["n"]
    t = threshold if threshold > 0 else 3.0
    p = np.asarray(m[:n], np.float32)
    Hm = _h(got["H_model"])
    mask = np.asarray(got["mask"]).reshape(-1)
    assert not mask[n:].any(), f"{what}: rows past n_valid are set"
    sampled = n > 4 and not r["flags"] & hr.ALL_POINTS
    if r["ambiguous"] is None:
        if got.get("table") is not None and sampled:
            np.testing.assert_array_equal(np.asarray(got["table"]), r["table"], err_msg=f"{what}: count table")
        assert (int(got["best"]), int(got["best_k"]), int(got["iters"])) == (r["best"], r["best_k"], r["iters"]), what
        np.testing.assert_array_equal(mask, r["mask"], err_msg=f"{what}: mask")
        if r["best"] == 0:
            assert not Hm.any(), f"{what}: no model must give a zero H_model"
            for key in ("H_refit", "H_out"):
                assert got.get(key) is None or not np.asarray(got[key]).any(), f"{what}: no model must give a zero {key}"
            return "exact"
        pin = p[r["mask"][:n] > 0]
        minimal = n == 4 or sampled  # H_model is a 4-point solve; with ALL_POINTS it is the refit
        tol_m = tol_solve(r["kappa_model"]) if minimal else tol_refit(r["kappa_refit"])
        d = hr.max_transfer_diff(Hm, r["H_model"], pin, HEIGHT, WIDTH, corners=not minimal)
        print(f"{what}: H_model {d:.3e} px (tolerance {tol_m:.3e}, kappa {r['kappa_model']:.3e})")
        assert d <= tol_m, f"{what}: H_model off by {d} px > {tol_m}"
        for key, tolk in (("H_refit", tol_refit(r["kappa_refit"])), ("H_out", tol_refine(r["kappa_refit"]) + r["lm_slack"])):
            if got.get(key) is None:
                continue
            if n == 4:
                tolk = tol_m  # no refit, no refinement: the same 4-point solve
            d = hr.max_transfer_diff(_h(got[key]), r[key], pin, HEIGHT, WIDTH, corners=n > 4)
            print(f"{what}: {key} {d:.3e} px (tolerance {tolk:.3e})")
            assert d <= tolk, f"{what}: {key} off by {d} px > {tolk}"
    else:  # only the invariants
        print(f"{what}: ambiguous -- {r['ambiguous']}")
        if got.get("table") is not None and sampled:
            tab = np.asarray(got["table"])
            assert ((tab >= r["table_lo"]) & (tab <= r["table_hi"])).all(), f"{what}: a count leaves its band interval"
            assert (int(got["best"]), int(got["best_k"]), int(got["iters"])) == hr.select(tab, n, confidence, len(tab)), \
                f"{what}: the rule on the reported table"
        if int(got["best"]) > 0 and sampled:
            sure, amb, _ = hr.classify(Hm, p, t, r["kappa"][int(got["best_k"])])
            bad = (mask[:n].astype(bool) != sure) & ~amb
            assert not bad.any(), f"{what}: mask inconsistent with the reported H_model at {np.flatnonzero(bad)[:4]}"
            assert int(mask.sum()) == int(got["best"]), f"{what}: mask and count differ"
    if got.get("S0") is not None:
        print(f"{what}: S {got['S0']:.6e} -> {got['S1']:.6e}")
        assert got["S1"] <= got["S0"], f"{what}: the refinement increased S"
    return "exact" if r["ambiguous"] is None else "ambiguous"


def cost(H, m, mask):
    """S = |r|^2 of the refinement's residuals at H over the masked rows (for the 'S is not increased' invariant)."""
    pin = np.asarray(m, np.float32)[np.asarray(mask).reshape(-1)[:len(m)] > 0]
    r, _ = hr.lm_eval(_h(H).reshape(-1)[:8], pin)
    return float((r * r).sum())


# ---- the tolerance record --------------------------------------------------------------------------------------------------
def measure():
    """Restatement against its twin on every family: prints what the constants above were taken from."""
    ys, nsamples = 0.0, 0
    yr = yl = yrk = ylk = 0.0
    for name in FAMILIES:
        m = pair(name)
        for idx, H, kap in hyps(name, N_DEFAULT, None, 0, 24):
            if H is None:
                continue
            sure, _, _ = hr.classify(H, m, 3.0, kap)
            sure[idx] = True
            ys = max(ys, hr.max_transfer_diff(H, hr.mp_solve4(m[idx]), m[sure], HEIGHT, WIDTH, corners=False) / (kap * EPS))
            nsamples += 1
        # well-supported winners (24 iterations), the first model whatever it is (1 iteration), least squares over all points
        for (iters, flags) in ((24, 0), (1, 0), (1, hr.ALL_POINTS)):
            if flags and name not in ALL_POINTS_FAMILIES:
                continue
            r = ref(name, max_iters=iters, flags=flags)
            if r["best"] == 0:
                continue
            pin = m[r["mask"] > 0]
            Ht = hr.mp_refit(pin)
            d = hr.max_transfer_diff(r["H_refit"], Ht, pin, HEIGHT, WIDTH)
            h2, _ = hr.lm_refine(Ht.reshape(-1)[:8], pin)
            dl = max(0.0, hr.max_transfer_diff(r["H_out"], np.append(h2, 1.0).reshape(3, 3), pin, HEIGHT, WIDTH) - r["lm_slack"])
            k = r["kappa_refit"] * EPS
            if r["ambiguous"] is None:
                yr, yl, yrk, ylk = max(yr, d), max(yl, dl), max(yrk, d / k), max(ylk, dl / k)
            print(f"{name:16s} iters {iters:2d} flags {flags} inliers {r['best']:4d} kappa_refit {r['kappa_refit']:.2e} refit {d:.3e} px "
                  f"({d / k:.2f} kappa eps)  refine {dl:.3e} px beyond the slack {r['lm_slack']:.1e} ({dl / k:.2f} kappa eps)  ambiguous: {r['ambiguous']}")
    print(f"{nsamples} samples: Y_SOLVE_PER_KAPPA_EPS {ys:.3f}   Y_REFIT {yr:.3e} = {yrk:.3f} kappa eps   Y_REFINE {yl:.3e} = {ylk:.3f} kappa eps")


if __name__ == "__main__":
    measure()
