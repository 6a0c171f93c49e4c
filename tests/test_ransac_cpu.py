"""The RANSAC estimator's per-lane arithmetic (csrc/ransac_math.h), compiled for the HOST with g++ through tests/emu/emu_ransac.cpp,
against the fp64 restatement of OpenCV 3.4's findFundamentalMat(FM_RANSAC) algorithm in tests/ransac_ref.py: the sampler's index
streams and its collinear / duplicate rejection, the 7-point solver, RANSACUpdateNumIters and the sequential selection rule.
Also the C ABI's argument checks (no launch).  Runs without a GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_ref as ref  # noqa: E402
import rule_tables  # noqa: E402

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EMU_DIR = os.path.join(REPO, "tests", "emu")
CSRC = os.path.join(REPO, "pytorch-deepfepe_amd", "csrc")


@pytest.fixture(scope="module")
def emu():
    out = os.path.join(EMU_DIR, "_build")
    os.makedirs(out, exist_ok=True)
    lib = os.path.join(out, "libemu_ransac.so")
    srcs = [os.path.join(EMU_DIR, "emu_ransac.cpp"), os.path.join(CSRC, "ransac_math.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", f"-I{CSRC}", srcs[0], "-o", lib], check=True)
    L = ctypes.CDLL(lib)
    P, I, D, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_ulonglong
    L.emu_ransac_stream.argtypes = [U, I, I, I, P]
    L.emu_ransac_stream.restype = None
    L.emu_ransac_sample.argtypes = [U, I, I, P, P]
    L.emu_ransac_sample.restype = I
    L.emu_ransac_seven_point.argtypes = [P, P, P, P, P]
    L.emu_ransac_seven_point.restype = I
    L.emu_ransac_update_num_iters.argtypes = [D, D, I]
    L.emu_ransac_update_num_iters.restype = I
    L.emu_ransac_select.argtypes = [P, I, D, I, P]
    L.emu_ransac_select.restype = None
    L.emu_ransac_is_inlier.argtypes = [P, D, D, D, D, D]
    L.emu_ransac_is_inlier.restype = I
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def emu_sample(L, seed, k, pts):
    pts = np.ascontiguousarray(pts, np.float32)
    idx = np.zeros(7, np.int32)
    ok = L.emu_ransac_sample(seed, k, pts.shape[0], _p(pts), _p(idx))
    return list(idx) if ok else None


def emu_seven_point(L, p7):
    p7 = np.asarray(p7, np.float32)
    cols = [np.ascontiguousarray(p7[:, c]) for c in range(4)]
    F = np.zeros(27)
    n = L.emu_ransac_seven_point(*[_p(c) for c in cols], _p(F))
    return [F[9 * i:9 * i + 9].reshape(3, 3) for i in range(n)]


def unit(F):
    f = np.asarray(F, np.float64).ravel()
    f = f / np.linalg.norm(f)
    return f * np.sign(f[np.argmax(np.abs(f))])


def scene(n, seed, noise=0.0):
    """n noise-free (up to the float32 rounding of the pixels) correspondences of a random rigid motion, KITTI intrinsics."""
    rng = np.random.default_rng(seed)
    K = np.array([[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1.0]])
    X = np.c_[rng.uniform(-15, 15, n), rng.uniform(-4, 4, n), rng.uniform(5, 35, n)]
    w = rng.normal(0, 0.05, 3)
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    t = rng.normal(0, 1, 3) * np.array([0.2, 0.1, 1.0])
    x1 = X @ K.T
    x2 = (X @ R.T + t) @ K.T
    x1, x2 = x1[:, :2] / x1[:, 2:], x2[:, :2] / x2[:, 2:]
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Kinv = np.linalg.inv(K)
    F = Kinv.T @ tx @ R @ Kinv
    pts = np.c_[x1, x2] + rng.normal(0, noise, (n, 4)) if noise else np.c_[x1, x2]
    return pts.astype(np.float32), F


@pytest.mark.parametrize("seed", [0, 1, 12345, (1 << 64) - 1])
@pytest.mark.parametrize("N", [15, 100, 1000, 4096])
def test_index_streams_match_the_restatement(emu, seed, N):
    for k in (0, 1, 7, 999, 123456):
        out = np.zeros(50, np.int32)
        emu.emu_ransac_stream(seed, k, N, 50, _p(out))
        s = ref.Stream(seed, k)
        assert list(out) == [s.index(N) for _ in range(50)]
        assert out.min() >= 0 and out.max() < N
    # the stream does not depend on anything but (seed, k): iterations differ from one another
    a, b = np.zeros(20, np.int32), np.zeros(20, np.int32)
    emu.emu_ransac_stream(seed, 3, N, 20, _p(a))
    emu.emu_ransac_stream(seed, 4, N, 20, _p(b))
    assert list(a) != list(b)


@pytest.mark.parametrize("seed", [0, 7, 99])
def test_samples_with_duplicate_and_collinear_rejection_match(emu, seed):
    rng = np.random.default_rng(seed)
    # a padded pair (crop_or_pad_choice repeats rows: a repeated point is collinear with anything) with a third of its points on
    # one line in image 1 and a few on one line in image 2
    base = rng.uniform(0, 1000, (40, 4)).astype(np.float32)
    base[:13, 1] = (0.5 * base[:13, 0] + 20.0).astype(np.float32)
    base[30:36, 3] = np.float32(200.0)
    pts = np.concatenate([base, base[rng.integers(0, 40, 60)]])
    n_redrawn = 0
    for k in range(300):
        e, r = emu_sample(emu, seed, k, pts), ref.draw_sample(seed, k, pts)
        assert e == r, k
        first = ref.Stream(seed, k)
        idx0 = []
        while len(idx0) < 7:
            v = first.index(pts.shape[0])
            if v not in idx0:
                idx0.append(v)
        n_redrawn += idx0 != r
    assert n_redrawn > 20  # the rejection path was exercised


def test_a_pair_without_any_valid_sample(emu):
    pts = np.zeros((20, 4), np.float32)
    pts[:, 0] = np.arange(20)
    pts[:, 1] = 3 * np.arange(20) + 1  # every point of image 1 on one line
    pts[:, 2:] = np.random.default_rng(0).uniform(0, 500, (20, 2))
    assert emu_sample(emu, 5, 0, pts) is None
    assert ref.draw_sample(5, 0, pts) is None


def test_seven_point_recovers_the_ground_truth(emu):
    for s in range(200):
        pts, F_gt = scene(7, s)
        Fs, Fr = emu_seven_point(emu, pts), ref.seven_point(pts)
        assert len(Fs) in (1, 3) and len(Fs) == len(Fr)
        # each root agrees with the fp64 restatement's (other null-space basis: compare as sets)
        for F in Fs:
            assert min(np.linalg.norm(unit(F) - unit(G)) for G in Fr) < 1e-9
            if abs(F[2, 2]) > 1e-300:
                assert F[2, 2] == 1.0
        # the ground truth is among the roots, up to what the float32 rounding of the pixel coordinates moves it (the 1e-9 above
        # is against the exact solution set of the rounded sample)
        assert min(np.linalg.norm(unit(F) - unit(F_gt)) for F in Fs) < 1e-3


def test_seven_point_root_count_agrees_on_random_samples(emu):
    rng = np.random.default_rng(1)
    n, agree, three = 4000, 0, 0
    for _ in range(n):
        p7 = rng.uniform(0, 1241, (7, 4)).astype(np.float32)
        Fs, Fr = emu_seven_point(emu, p7), ref.seven_point(p7)
        agree += len(Fs) == len(Fr)
        three += len(Fs) == 3
        for F in Fs:  # every root is a rank-2 matrix through the 7 points
            h1, h2 = np.c_[p7[:, :2], np.ones(7)], np.c_[p7[:, 2:], np.ones(7)]
            f = F / np.linalg.norm(F)
            assert np.abs(np.linalg.svd(f, compute_uv=False)[2]) < 1e-7
            assert np.abs(((h2 @ f) * h1).sum(1)).max() < 1e-6 * np.abs(h2).max() * np.abs(h1).max()
    assert agree >= 0.999 * n
    assert three > 0.1 * n  # both branches of the cubic were exercised


def test_update_num_iters_agrees_exactly(emu):
    eps = sorted(set(np.linspace(0.0, 1.0, 201).tolist() + [1e-9, 1e-4, 0.999999, 1.0 - 1e-12, 0.5]))
    for p in (0.99, 0.999, 0.5, 1.0, 0.0):
        for niters in (1, 10, 100, 1000, 2000, 100000):
            for ep in eps:
                assert emu.emu_ransac_update_num_iters(p, ep, niters) == ref.update_num_iters(p, ep, niters), (p, ep, niters)
    assert emu.emu_ransac_update_num_iters(0.99, 0.0, 1000) == 0  # every point an inlier: stop after this iteration
    assert emu.emu_ransac_update_num_iters(0.99, 1.0, 1000) == 1000


def test_selection_rule_agrees_on_synthetic_tables(emu):
    rng = np.random.default_rng(3)
    for trial in range(500):
        N = int(rng.integers(15, 2000))
        T = int(rng.integers(1, 300))
        tab = rng.integers(0, N + 1, (T, 3)).astype(np.int32)
        tab[rng.random((T, 3)) < 0.4] = ref.NO_ROOT
        tab[:, 0] = np.where(tab[:, 0] < 0, rng.integers(0, N + 1, T), tab[:, 0])  # root 0 exists in every sampled iteration
        if trial % 5 == 0:
            tab = np.minimum(tab, rng.integers(0, 12))  # small counts: the max(best, 6) floor matters
        if trial % 7 == 0:
            cut = int(rng.integers(0, T))
            tab[cut] = ref.NO_SAMPLE  # the sampler gave up: the loop ends there
        conf = float(rng.choice([0.99, 0.999, 0.5]))
        out = np.zeros(4, np.int32)
        tab = np.ascontiguousarray(tab, dtype=np.int32)
        emu.emu_ransac_select(_p(tab), N, conf, T, _p(out))
        assert tuple(out) == ref.select(tab, N, conf, T), trial


def test_shared_rule_as_3_roots_of_7_points_on_the_edge_tables(emu):
    """rs::select_best<3, 7> on tests/rule_tables.py: several improving roots in one iteration, no sample at k = 0 and past the
    first model, ties, confidence 0 and 1 -- all four outputs against this estimator's own restatement."""
    tab, N, conf = rule_tables.climbing(3)
    assert ref.select(tab, N, conf, len(tab)) == (99, 5, 2, 6)  # every root of k = 5 was looked at, k = 6 was not
    for tab, N, conf in rule_tables.tables(3, ref.NO_SAMPLE):
        out = np.zeros(4, np.int32)
        emu.emu_ransac_select(_p(tab), N, conf, len(tab), _p(out))
        assert tuple(out) == ref.select(tab, N, conf, len(tab)), (tab.tolist(), N, conf)


def test_inlier_decision_matches_the_error_outside_the_band(emu):
    pts, F_gt = scene(2000, 5, noise=0.3)
    F = F_gt / F_gt[2, 2]
    err = ref.errors(F, pts)
    Fc = np.ascontiguousarray(F.ravel())
    for t in (0.1, 0.5, 1.0):
        t2 = t * t
        got = np.array([emu.emu_ransac_is_inlier(_p(Fc), *map(float, p), t2) for p in pts.astype(np.float64)])
        sure = np.abs(err - t2) > 1e-6 * t2
        assert ((got == 1) == (err <= t2))[sure].all()
        assert 0 < got.sum() < len(got)


def test_cabi_argument_checks_without_launching(dfepe):
    L = dfepe._lib.lib()
    call = lambda B, N, t=0.1, p=0.99, it=1000, m=None: L.dfepe_ransac_fundamental(m, B, N, t, p, it, 0, None, None, None, None, None, None,
                                                                                 None, None, None)
    assert call(0, 100) == 0                      # empty batch
    assert call(4, 14) == -3 and call(4, 5) == -3  # fewer than 15 correspondences: LMedS in OpenCV, not built
    assert call(4, 4097) == -3 and call(65536, 100) == -3
    assert call(4, 100) == -1                     # null pointers
    assert call(-1, 100) == -1 and call(4, 100, it=0) == -1 and call(4, 100, t=-1.0) == -1 and call(4, 100, p=1.5) == -1
    assert L.dfepe_ransac_workspace_bytes(8, 1000, 1000) >= 8 * 1000 * 3 * 4 + 8 * 9 * 8
    assert L.dfepe_ransac_workspace_bytes(0, 1000, 1000) == 0
    assert L.dfepe_ransac_in_front(None, None, None, 0, 100, 50.0, None, None, None) == 0
    assert L.dfepe_ransac_in_front(None, None, None, 2, 100, 50.0, None, None, None) == -1
