"""The five-point RANSAC estimator's per-lane arithmetic (csrc/ransac5_math.h), compiled for the HOST with g++ through
tests/emu/emu_ransac5.cpp, against the fp64 restatement in tests/ransac5_ref.py: the sampler, the five-point solver (validity of
every solution, the ground truth and completeness on a well-conditioned scene), RANSACUpdateNumIters with exponent 5, the
selection rule with ten slots and the Sampson decision.  Also the C ABI's argument checks (no launch).  Runs without a GPU.

Why the solver is not compared root for root everywhere: on the KITTI-like synth.make_scene pairs (small rotation, mostly
forward motion) two fp64 solves of the same sample disagree by more than 1e-7 for about one sample in eight, so only validity is
demanded there; completeness is demanded where the problem is well conditioned (the wide-baseline scene below, and uniform
noise), with a cap of 5 % of samples that may differ."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac5_ref as ref  # noqa: E402
import rule_tables  # noqa: E402

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EMU_DIR = os.path.join(REPO, "tests", "emu")
CSRC = os.path.join(REPO, "pytorch-deepfepe_amd", "csrc")
KITTI_K = np.array([[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1.0]])
KINDS = [(0.0, 0.05), (0.3, 0.5), (0.6, 0.5), "noise"]


@pytest.fixture(scope="module")
def emu():
    out = os.path.join(EMU_DIR, "_build")
    os.makedirs(out, exist_ok=True)
    lib = os.path.join(out, "libemu_ransac5.so")
    srcs = [os.path.join(EMU_DIR, "emu_ransac5.cpp"), os.path.join(CSRC, "ransac5_math.h"), os.path.join(CSRC, "ransac_math.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", f"-I{CSRC}", srcs[0], "-o", lib], check=True)
    L = ctypes.CDLL(lib)
    P, I, D, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_ulonglong
    L.emu_ransac5_sample.argtypes = [U, I, I, P]
    L.emu_ransac5_sample.restype = None
    L.emu_ransac5_normalize.argtypes = [P, P, I, D, P]
    L.emu_ransac5_normalize.restype = D
    L.emu_ransac5_five_point.argtypes = [P, P]
    L.emu_ransac5_five_point.restype = I
    L.emu_ransac5_update_num_iters.argtypes = [D, D, I]
    L.emu_ransac5_update_num_iters.restype = I
    L.emu_ransac5_select.argtypes = [P, I, D, I, P]
    L.emu_ransac5_select.restype = None
    L.emu_ransac5_is_inlier.argtypes = [P, P, I, D, P]
    L.emu_ransac5_is_inlier.restype = None
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def emu_sample(L, seed, k, N):
    idx = np.zeros(5, np.int32)
    L.emu_ransac5_sample(seed, k, N, _p(idx))
    return [int(i) for i in idx]


def emu_normalize(L, pts, K, threshold=1.0):
    pts = np.ascontiguousarray(pts, np.float32)
    Kf = np.ascontiguousarray(K, np.float32).ravel()
    q = np.zeros((pts.shape[0], 4))
    t2 = L.emu_ransac5_normalize(_p(pts), _p(Kf), pts.shape[0], threshold, _p(q))
    return q, t2


def emu_five_point(L, q5):
    q5 = np.ascontiguousarray(q5, np.float64)
    E = np.zeros(90)
    n = L.emu_ransac5_five_point(_p(q5), _p(E))
    assert 0 <= n <= 10
    return [E[9 * i:9 * i + 9].reshape(3, 3).copy() for i in range(n)]


def kind_points(dfepe, kind, N, seed):
    if kind == "noise":
        g = np.random.default_rng(seed)
        return np.c_[g.uniform(0, 1241, (N, 1)), g.uniform(0, 376, (N, 1)), g.uniform(0, 1241, (N, 1)),
                     g.uniform(0, 376, (N, 1))].astype(np.float32)
    return dfepe.synth.make_scene(1, N, seed=seed, outlier_ratio=kind[0], noise_px=kind[1])["matches_xy_ori"][0].numpy()


def wide_scene(seed, n=200):
    """A well-conditioned pair: 200 points in a box in front of the first camera, rotation vector N(0, 0.25^2) per axis, a
    mostly sideways translation.  Returns float32 pixels [n,4] and the unit-norm, sign-fixed ground-truth E."""
    rng = np.random.default_rng(seed)
    X = np.c_[rng.uniform(-4, 4, n), rng.uniform(-2, 2, n), rng.uniform(4, 12, n)]
    w = rng.normal(0, 0.25, 3)
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    t = np.array([rng.choice([-1.0, 1.0]) * rng.uniform(1, 2), rng.uniform(-.5, .5), rng.uniform(-.5, .5)])
    x1 = X @ KITTI_K.T
    x2 = (X @ R.T + t) @ KITTI_K.T
    pts = np.c_[x1[:, :2] / x1[:, 2:], x2[:, :2] / x2[:, 2:]].astype(np.float32)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    return pts, ref.unit(tx @ R)


def check_valid(E, q5):
    """The validity bounds of one solution for its sample (also used by the GPU tests)."""
    e = E.ravel()
    assert abs(np.linalg.norm(e) - 1.0) < 1e-12
    assert e[np.argmax(np.abs(e))] > 0
    h1, h2 = np.c_[q5[:, :2], np.ones(5)], np.c_[q5[:, 2:], np.ones(5)]
    assert np.abs(((h2 @ E) * h1).sum(1)).max() <= 1e-10
    c, d = ref.constraint_residuals(E)
    assert c <= 1e-6 and d <= 1e-6, (c, d)


def complete(Es, Er):
    """The device's solutions are the restatement's: same number, each restatement root within 1e-6 of a device root."""
    return len(Es) == len(Er) and all(min(np.abs(E - G).max() for E in Es) < 1e-6 for G in Er)


@pytest.mark.parametrize("seed", [0, 0xFEDCBA9876543210])
@pytest.mark.parametrize("N", [6, 64, 1000])
def test_samples_match_the_restatement(emu, seed, N):
    for k in list(range(40)) + [999, 123456]:
        idx = emu_sample(emu, seed, k, N)
        assert idx == ref.draw_sample(seed, k, N)
        assert len(set(idx)) == 5 and min(idx) >= 0 and max(idx) < N


def test_normalisation_matches_and_the_identity_leaves_the_points(emu):
    pts = np.random.default_rng(0).uniform(0, 1241, (50, 4)).astype(np.float32)
    q, t2 = emu_normalize(emu, pts, KITTI_K, 0.5)
    assert np.array_equal(q, ref.normalize(pts, KITTI_K)) and t2 == ref.threshold2(0.5, KITTI_K)
    q, t2 = emu_normalize(emu, pts, np.eye(3), 0.5)
    assert np.array_equal(q, pts.astype(np.float64)) and t2 == 0.25


@pytest.mark.parametrize("kind", KINDS, ids=str)
def test_every_solution_is_valid(emu, dfepe, kind):
    pts = kind_points(dfepe, kind, 200, 7)
    q, _ = emu_normalize(emu, pts, KITTI_K)
    n_roots = 0
    for k in range(300):
        q5 = q[ref.draw_sample(3, k, 200)]
        Es = emu_five_point(emu, q5)
        n_roots += len(Es)
        for E in Es:
            check_valid(E, q5)
    assert n_roots >= 300  # the solver finds solutions: on average at least one a sample


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_ground_truth_and_completeness_on_a_well_conditioned_scene(emu, seed):
    pts, E_gt = wide_scene(seed)
    q, _ = emu_normalize(emu, pts, KITTI_K)
    found = same = 0
    for k in range(300):
        q5 = q[ref.draw_sample(seed, k, 200)]
        Es, Er = emu_five_point(emu, q5), ref.five_point(q5)
        found += any(np.abs(E.ravel() - E_gt).max() < 1e-4 for E in Es)
        same += complete(Es, Er)
    print(f"seed {seed}: ground truth among the roots {found}/300, roots equal to the restatement's {same}/300")
    assert found >= 0.95 * 300
    assert same >= 0.95 * 300


def test_completeness_on_uniform_noise(emu, dfepe):
    pts = kind_points(dfepe, "noise", 200, 11)
    q, _ = emu_normalize(emu, pts, KITTI_K)
    same = sum(complete(emu_five_point(emu, q[idx]), ref.five_point(q[idx])) for idx in (ref.draw_sample(5, k, 200) for k in range(300)))
    print(f"noise: roots equal to the restatement's {same}/300")
    assert same >= 0.95 * 300


def test_update_num_iters_agrees_exactly(emu):
    eps = sorted(set(np.linspace(0.0, 1.0, 201).tolist() + [1e-9, 1e-4, 0.999999, 1.0 - 1e-12, 0.5]))
    for p in (0.99, 0.999, 0.5, 1.0, 0.0):
        for niters in (1, 10, 100, 1000, 2000, 100000):
            for ep in eps:
                assert emu.emu_ransac5_update_num_iters(p, ep, niters) == ref.update_num_iters(p, ep, niters), (p, ep, niters)
    assert emu.emu_ransac5_update_num_iters(0.999, 0.0, 1000) == 0  # every point an inlier: stop after this iteration
    assert emu.emu_ransac5_update_num_iters(0.999, 1.0, 1000) == 1000
    assert emu.emu_ransac5_update_num_iters(0.99, 0.5, 1000) == 145  # log(0.01) / log(1 - 0.5^5): exponent 5, not 7


def test_selection_rule_agrees_on_synthetic_tables(emu):
    rng = np.random.default_rng(3)
    for trial in range(500):
        N = int(rng.integers(6, 2000))
        T = int(rng.integers(1, 300))
        tab = rng.integers(0, N + 1, (T, 10)).astype(np.int32)
        tab[rng.random((T, 10)) < 0.6] = ref.NO_ROOT
        if trial % 5 == 0:
            tab = np.minimum(tab, rng.integers(0, 9))  # small counts: the max(best, 4) floor matters
        conf = float(rng.choice([0.99, 0.999, 0.5]))
        out = np.zeros(4, np.int32)
        tab = np.ascontiguousarray(tab, dtype=np.int32)
        emu.emu_ransac5_select(_p(tab), N, conf, T, _p(out))
        assert tuple(out) == ref.select(tab, N, conf, T), trial


def test_shared_rule_as_10_roots_of_5_points_on_the_edge_tables(emu):
    """rs::select_best<10, 5> on tests/rule_tables.py: several improving roots in one iteration, ties, confidence 0 and 1 -- all
    four outputs against this estimator's own restatement.  No iteration without a sample: this table never holds one."""
    tab, N, conf = rule_tables.climbing(10)
    assert ref.select(tab, N, conf, len(tab)) == (99, 5, 9, 6)  # every root of k = 5 was looked at, k = 6 was not
    for tab, N, conf in rule_tables.tables(10):
        out = np.zeros(4, np.int32)
        emu.emu_ransac5_select(_p(tab), N, conf, len(tab), _p(out))
        assert tuple(out) == ref.select(tab, N, conf, len(tab)), (tab.tolist(), N, conf)


def test_inlier_decision_matches_the_sampson_error_outside_the_band(emu, dfepe):
    pts = kind_points(dfepe, (0.3, 0.5), 2000, 5)
    q, _ = emu_normalize(emu, pts, KITTI_K)
    for k in range(20):
        for E in emu_five_point(emu, q[ref.draw_sample(1, k, 2000)]):
            err = ref.sampson(E, q)
            Ec = np.ascontiguousarray(E.ravel())
            for t in (0.01, 0.5, 1.0):
                t2 = ref.threshold2(t, KITTI_K)
                got = np.zeros(len(q), np.uint8)
                emu.emu_ransac5_is_inlier(_p(Ec), _p(np.ascontiguousarray(q)), len(q), t2, _p(got))
                sure = np.abs(err - t2) > 1e-6 * t2
                assert ((got == 1) == (err <= t2))[sure].all()
    E_gt = dfepe.synth.make_scene(1, 2000, seed=5, outlier_ratio=0.3, noise_px=0.5)["E_gt"][0].double().numpy()
    got = np.zeros(len(q), np.uint8)
    emu.emu_ransac5_is_inlier(_p(np.ascontiguousarray(ref.unit(E_gt))), _p(np.ascontiguousarray(q)), len(q), ref.threshold2(1.0, KITTI_K),
                              _p(got))
    assert 0.5 * len(q) < got.sum() < len(q)  # both decisions occur


def test_cabi_argument_checks_without_launching(dfepe):
    L = dfepe._lib.lib()
    call = lambda B, N, t=1.0, p=0.999, it=1000: L.dfepe_ransac_essential(None, None, B, N, t, p, it, 0, None, None, None, None,
                                                                          None, None, None, None, None, None)
    assert call(0, 100) == 0                       # empty batch
    assert call(4, 5) == -3                        # OpenCV returns the stacked models of the one sample: not built
    assert call(4, 4097) == -3 and call(65536, 100) == -3
    assert call(4, 100, it=0) == -1 and call(4, 100, t=-1.0) == -1
    assert call(4, 100) == -1 and call(4, 6) == -1  # null pointers
    assert L.dfepe_ransac5_workspace_bytes(8, 1000, 1000) >= 8 * 1000 * 10 * 4 + 8 * 9 * 8
    assert L.dfepe_ransac5_workspace_bytes(0, 1000, 1000) == 0
    assert L.dfepe_version() == 154
