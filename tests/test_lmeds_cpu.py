"""The LMedS estimators' per-lane arithmetic (csrc/lmeds_math.h), compiled for the HOST with g++ through tests/emu/emu_lmeds.cpp,
against numpy and the fp64 restatement in tests/lmeds_ref.py: the bit-by-bit selection of the median (64 emulated lanes x R
registers, the layout and the rung the device takes) against numpy.sort, the two error functions within the restatement's derived
bound, the iteration count, sigma and the inlier bound exactly, and the strict-minimum rule.  Also the C ABI's argument checks
(no launch) and the ctypes table.  Runs without a GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lmeds_ref as ref  # noqa: E402
import ransac5_ref as ref5  # noqa: E402
import ransac_ref as ref7  # noqa: E402

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EMU_DIR = os.path.join(REPO, "tests", "emu")
CSRC = os.path.join(REPO, "pytorch-deepfepe_amd", "csrc")
KITTI_K = np.array([[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1.0]])


@pytest.fixture(scope="module")
def emu():
    out = os.path.join(EMU_DIR, "_build")
    os.makedirs(out, exist_ok=True)
    lib = os.path.join(out, "libemu_lmeds.so")
    srcs = [os.path.join(EMU_DIR, "emu_lmeds.cpp")] + [os.path.join(CSRC, h) for h in ("lmeds_math.h", "ransac5_math.h", "ransac_math.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", f"-I{CSRC}", srcs[0], "-o", lib], check=True)
    L = ctypes.CDLL(lib)
    P, I, D, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_float
    L.emu_lmeds_regs_for.argtypes, L.emu_lmeds_regs_for.restype = [I], I
    L.emu_lmeds_median.argtypes, L.emu_lmeds_median.restype = [P, I, I], F
    L.emu_lmeds_f_errors.argtypes, L.emu_lmeds_f_errors.restype = [P, P, I, P], None
    L.emu_lmeds_e_errors.argtypes, L.emu_lmeds_e_errors.restype = [P, P, I, P], None
    L.emu_lmeds_sigma.argtypes, L.emu_lmeds_sigma.restype = [D, I, I, P], D
    L.emu_lmeds_num_iters.argtypes, L.emu_lmeds_num_iters.restype = [I, D, I], I
    L.emu_lmeds_select.argtypes, L.emu_lmeds_select.restype = [P, I, I, P], None
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def emu_median(L, e32, force=0):
    e32 = np.ascontiguousarray(e32, np.float32)
    return np.float32(L.emu_lmeds_median(_p(e32.view(np.uint32)), len(e32), force))


def same_float(a, b):
    return np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32)


# ---- the selection --------------------------------------------------------------------------------------------------------
SIZES = [1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 1000, 1001, 4095, 4096]  # both parities at every lane and register tail
TINY = np.float32(1e-45)  # the smallest denormal


def _value_sets(N, g):
    """Named fp32 error vectors of length N: what the median's selection has to get right."""
    base = (g.lognormal(0.0, 4.0, N)).astype(np.float32)
    sets = {"lognormal": base, "all_equal": np.full(N, np.float32(0.37)), "all_zero": np.zeros(N, np.float32),
            "all_inf": np.full(N, np.inf, np.float32)}
    run = np.sort(base)
    lo, hi = max(0, N // 2 - 3), min(N, N // 2 + 3)
    run[lo:hi] = run[N // 2]  # a run of duplicates across the median
    sets["run_across_median"] = g.permutation(run)
    half = np.sort(base)
    half[N // 2:] = half[N // 2]  # the run starts exactly at rank N/2: the lower neighbour is a different value
    sets["run_from_median_up"] = g.permutation(half)
    low = np.sort(base)
    low[:N // 2] = low[0]  # ... and ends exactly below it
    sets["run_below_median"] = g.permutation(low)
    mixed = base.copy()
    mixed[g.random(N) < 0.3] = 0.0
    mixed[g.random(N) < 0.2] = TINY * np.float32(g.integers(1, 9))
    mixed[g.random(N) < 0.3] = np.inf
    sets["zeros_denormals_inf"] = mixed
    two = np.where(g.random(N) < 0.5, np.float32(1.0), np.float32(np.inf)).astype(np.float32)
    sets["finite_or_inf"] = two
    sets["adjacent_patterns"] = (np.uint32(0x3F800000) + g.integers(0, 4, N).astype(np.uint32)).view(np.float32)
    sets["huge"] = np.full(N, np.finfo(np.float32).max, np.float32)  # the sum of the two middle values overflows in fp32
    return sets


@pytest.mark.parametrize("N", SIZES)
def test_selection_agrees_with_numpy_sort(emu, N):
    g = np.random.default_rng(N)
    assert emu.emu_lmeds_regs_for(N) * 64 >= N and (N <= 64 or emu.emu_lmeds_regs_for(N) * 32 < N)
    for name, e in _value_sets(N, g).items():
        want = ref.median32(e)
        got = emu_median(emu, e)
        assert same_float(got, want), (N, name, got, want)
        s = np.sort(e)  # and the restatement's median is numpy's sorted middle
        with np.errstate(over="ignore"):
            direct = s[N // 2] if N % 2 else np.float32(np.float32(s[N // 2 - 1] + s[N // 2]) * np.float32(0.5))
        assert same_float(want, direct), (N, name)


@pytest.mark.parametrize("N", [1, 2, 63, 64])
def test_every_rung_gives_the_same_median(emu, N):
    g = np.random.default_rng(100 + N)
    for name, e in _value_sets(N, g).items():
        want = ref.median32(e)
        for R in (1, 2, 4, 8, 16, 32, 64):
            assert same_float(emu_median(emu, e, R), want), (N, name, R)


# ---- errors, sigma, the rule ----------------------------------------------------------------------------------------------
def _points(dfepe, N, seed):
    return dfepe.synth.make_scene(1, N, seed=seed, outlier_ratio=0.3, noise_px=0.5)["matches_xy_ori"][0].numpy()


def test_fundamental_errors_within_the_derived_bound(emu, dfepe):
    pts = _points(dfepe, 500, 3)
    n_models = 0
    for k in range(40):
        idx = ref7.draw_sample(1, k, pts)
        for F in ref7.seven_point(pts[idx]):
            Fc = np.ascontiguousarray(F.ravel())
            got = np.zeros(len(pts), np.float32)
            emu.emu_lmeds_f_errors(_p(Fc), _p(np.ascontiguousarray(pts)), len(pts), _p(got))
            want = ref.to_f32(ref.f_errors(F, pts))
            bound = ref.error_bounds(F, np.zeros((3, 3)), pts, False)  # the same model on both sides: no model term
            assert (np.abs(got.astype(np.float64) - want) <= bound).all(), k
            assert bound[idx].max() < 1e-12  # the absolute term at the sample's own points stays far below any real error
            n_models += 1
    assert n_models >= 40
    # a degenerate model: zero line norms count as +inf, never NaN
    got = np.zeros(len(pts), np.float32)
    emu.emu_lmeds_f_errors(_p(np.zeros(9)), _p(np.ascontiguousarray(pts)), len(pts), _p(got))
    assert np.isinf(got).all() and np.isinf(ref.to_f32(ref.f_errors(np.zeros((3, 3)), pts))).all()


def test_essential_errors_within_the_derived_bound(emu, dfepe):
    pts = _points(dfepe, 500, 4)
    q = ref5.normalize(pts, KITTI_K)
    n_models = 0
    for k in range(20):
        for E in ref5.five_point(q[ref5.draw_sample(1, k, len(q))]):
            got = np.zeros(len(q), np.float32)
            emu.emu_lmeds_e_errors(_p(np.ascontiguousarray(E.ravel())), _p(np.ascontiguousarray(q)), len(q), _p(got))
            want = ref.to_f32(ref.e_errors(E, q))
            bound = ref.error_bounds(E, np.zeros((3, 3)), q, True)
            assert (np.abs(got.astype(np.float64) - want) <= bound).all(), k
            n_models += 1
    assert n_models >= 20
    got = np.zeros(len(q), np.float32)
    emu.emu_lmeds_e_errors(_p(np.zeros(9)), _p(np.ascontiguousarray(q)), len(q), _p(got))
    assert np.isinf(got).all()


def test_iteration_count_agrees_and_is_300_for_the_defaults(emu):
    assert emu.emu_lmeds_num_iters(7, 0.99, 1000) == 300 == ref.num_iters(7, 0.99, 1000)
    for m in (7, 5):
        for p in (0.0, 0.5, 0.9, 0.99, 0.999, 1.0):
            for it in (1, 2, 63, 64, 65, 299, 300, 301, 1000, 100000):
                assert emu.emu_lmeds_num_iters(m, p, it) == ref.num_iters(m, p, it), (m, p, it)
    assert ref.num_iters(7, 0.0, 1000) == 0 and ref.num_iters(7, 1.0, 1000) == 1000 and ref.num_iters(7, 0.99, 299) == 299
    assert ref.num_iters(5, 0.999, 1000) == emu.emu_lmeds_num_iters(5, 0.999, 1000) < 300  # exponent 5: fewer iterations


def test_sigma_and_the_inlier_bound_agree_exactly(emu):
    g = np.random.default_rng(5)
    meds = [0.0, 1e-45, 1e-30, 7.2e-8, 0.25, 1.0, 3.4e38, np.inf] + list(g.lognormal(0, 6, 200).astype(np.float32).astype(np.float64))
    for m, Ns in ((7, (8, 9, 14, 15, 64, 1000, 4096)), (5, (6, 7, 64, 4096))):
        for N in Ns:
            for med in meds:
                b = np.zeros(1, np.float32)
                s = emu.emu_lmeds_sigma(med, N, m, _p(b))
                assert s == ref.sigma_of(med, N, m), (m, N, med)
                assert same_float(b[0], ref.bound32(s)), (m, N, med)
    assert ref.sigma_of(0.0, 8, 7) == 0.001 and ref.sigma_of(1e-10, 8, 7) == 0.001  # the floor (noise-free pairs hit it)
    assert ref.sigma_of(1.0, 8, 7) == 2.5 * 1.4826 * 6.0


@pytest.mark.parametrize("roots", [3, 10])
def test_selection_rule_agrees_on_synthetic_tables(emu, roots):
    g = np.random.default_rng(roots)
    for trial in range(400):
        T = int(g.integers(1, 320))
        tab = g.lognormal(0, 3, (T, roots)).astype(np.float32).astype(np.float64)
        tab[g.random((T, roots)) < 0.5] = ref.NO_ROOT
        tab[g.random((T, roots)) < 0.05] = np.inf
        if trial % 4 == 0:
            tab = np.where(tab > 0, np.round(tab), tab)  # exact ties: the first one in (k, root) order wins
        if roots == 3 and trial % 3 == 0:
            tab[int(g.integers(0, T))] = ref.NO_SAMPLE     # the loop ends there; k = 0: no model
        if trial % 50 == 0:
            tab[tab >= 0] = np.inf                         # no finite median: no model
        tab = np.ascontiguousarray(tab)
        out = np.zeros(4)
        emu.emu_lmeds_select(_p(tab), T, roots, _p(out))
        best, bk, br, it = ref.select(tab, T)
        assert (out[0], int(out[1]), int(out[2]), int(out[3])) == (best, bk, br, it), trial
    out = np.zeros(4)
    emu.emu_lmeds_select(_p(np.zeros(0)), 0, roots, _p(out))
    assert tuple(out) == (ref.DBL_MAX, -1, -1, 0)  # niters = 0 (confidence 0): no model


def test_restatement_ambiguity_class():
    med = np.array([[1.0, 2.0, ref.NO_ROOT], [0.5, ref.NO_ROOT, ref.NO_ROOT], [ref.NO_SAMPLE] * 3, [0.1, 0.1, 0.1]])
    bnd = np.full(med.shape, 1e-6)
    assert ref.select(med, 4) == (0.5, 1, 0, 2) and not ref.is_ambiguous(med, bnd, 4)
    med2 = med.copy()
    med2[0, 0] = 0.5 + 1.5e-6
    assert ref.is_ambiguous(med2, bnd, 4)          # a second median within the summed bounds of the minimum
    bnd2 = bnd.copy()
    bnd2[1, 0] = np.inf
    assert ref.is_ambiguous(med, bnd2, 4)          # the minimum itself is not comparable


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_cabi_argument_checks_without_launching(dfepe):
    L = dfepe._lib.lib()
    nul = [None] * 11
    f = lambda B, N, p=0.99, it=1000: L.dfepe_lmeds_fundamental(None, B, N, p, it, 0, *nul)
    e = lambda B, N, p=0.999, it=1000: L.dfepe_lmeds_essential(None, None, B, N, p, it, 0, *nul)
    assert f(0, 100) == 0 and e(0, 100) == 0                          # empty batch
    assert f(4, 7) == -3 and f(4, 4097) == -3 and f(65536, 100) == -3  # N = 7: OpenCV's direct 7-point path, not built
    assert e(4, 5) == -3 and e(4, 4097) == -3 and e(65536, 100) == -3
    assert f(4, 100, it=0) == -1 and f(4, 100, p=-0.1) == -1 and f(4, 100, p=1.5) == -1 and f(-1, 100) == -1
    assert e(4, 100, it=0) == -1 and e(4, 100, p=float("nan")) == -1
    assert f(4, 8) == -1 and f(4, 4096) == -1 and e(4, 6) == -1       # in range: the null pointers are what is refused
    assert L.dfepe_lmeds_num_iters(7, 0.99, 1000) == 300 and L.dfepe_lmeds_num_iters(7, 0.99, 100) == 100
    assert L.dfepe_lmeds_num_iters(5, 0.999, 1000) == ref.num_iters(5, 0.999, 1000)
    assert L.dfepe_lmeds_num_iters(6, 0.99, 1000) == -1 and L.dfepe_lmeds_num_iters(7, 0.99, 0) == -1
    assert L.dfepe_lmeds_workspace_bytes(8, 7, 0.99, 1000) >= 8 * 300 * 3 * 8 + 8 * 9 * 8 + 8 * 4
    assert L.dfepe_lmeds_workspace_bytes(8, 5, 0.999, 1000) >= 8 * ref.num_iters(5, 0.999, 1000) * 10 * 8
    assert L.dfepe_lmeds_workspace_bytes(0, 7, 0.99, 1000) == 0 and L.dfepe_lmeds_workspace_bytes(8, 6, 0.99, 1000) == 0
    assert L.dfepe_version() == 154
    # the RANSAC entry keeps refusing what LMedS now serves
    assert L.dfepe_ransac_fundamental(None, 4, 14, 0.1, 0.99, 1000, 0, *([None] * 9)) == -3


def test_new_symbols_are_in_the_ctypes_table(dfepe):
    for name in ("dfepe_lmeds_num_iters", "dfepe_lmeds_workspace_bytes", "dfepe_lmeds_fundamental", "dfepe_lmeds_essential"):
        assert name in dfepe.EXPORTED_SYMBOLS
    assert dfepe._lib.LMEDS_MIN_N == 8 and dfepe._lib.LMEDS5_MIN_N == 6 and dfepe._lib.RANSAC_MIN_N == 15
    for fn in ("lmeds_fundamental", "lmeds_pose", "lmeds_essential", "lmeds_essential_pose"):
        assert callable(getattr(dfepe.ops, fn))
    assert callable(dfepe.compat.utils_opencv.recover_camera_lmeds)
