"""The optimal correction's per-lane arithmetic (csrc/correct_matches_math.h), compiled for the HOST with g++ through
tests/emu/emu_correct_matches.cpp, against the fp64 restatement in tests/correct_matches_ref.py -- and the restatement itself
against a route that does not use the sextic at all (a scan over the pencil of epipolar lines).  Also the C ABI's argument
checks (no launch) and the host-side grid.  Runs without a GPU.

Inputs: synth.make_scene(8, 100, seed=3) in float64 and its F_gt; the reference's grid for a 1241 x 376 image as both point
sets ("grid"), the grid against the second-image points of the scene's noisy matches ("grid_vs_matches": different points in the
two images, corrections of up to ~270 px) and the matches themselves ("matches").  Figures seen on them (printed by the tests):
the two routes' minimal costs agree to 5.2e-10 relative, the restatement's output is within 4.1e-10 px of its epipolar line and
its squared displacement equals its cost to 2.5e-10 relative; the header agrees with the restatement to 1.5e-13 relative in cost
and 3.9e-12 px in position, with every real root of numpy.roots among its candidates and no near-tie among the 2400 points."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import correct_matches_ref as ref  # noqa: E402

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EMU_DIR = os.path.join(REPO, "tests", "emu")
CSRC = os.path.join(REPO, "pytorch-deepfepe_amd", "csrc")
IM_SHAPE = (376, 1241)
SETS = ["grid", "grid_vs_matches", "matches"]


@pytest.fixture(scope="module")
def emu():
    out = os.path.join(EMU_DIR, "_build")
    os.makedirs(out, exist_ok=True)
    lib = os.path.join(out, "libemu_correct_matches.so")
    srcs = [os.path.join(EMU_DIR, "emu_correct_matches.cpp"), os.path.join(CSRC, "correct_matches_math.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", f"-I{CSRC}", srcs[0], "-o", lib], check=True)
    L = ctypes.CDLL(lib)
    P = ctypes.c_void_p
    L.emu_correct_matches.argtypes = [P, P, P, ctypes.c_int, P, P, P]
    L.emu_correct_matches.restype = None
    L.emu_correct_matches_max_candidates.restype = ctypes.c_int
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def emu_correct(L, F, p, q):
    """-> out [n,5] fp64 (corrected p, corrected q, cost), and per point the list of candidate t the header evaluated."""
    F = np.ascontiguousarray(F, np.float64)
    p, q = np.ascontiguousarray(p, np.float32), np.ascontiguousarray(q, np.float32)
    n, C = len(p), L.emu_correct_matches_max_candidates()
    out, cand, ncand = np.zeros((n, 5)), np.zeros((n, C)), np.zeros(n, np.int32)
    L.emu_correct_matches(_p(F), _p(p), _p(q), n, _p(out), _p(cand), _p(ncand))
    assert (ncand >= 1).all() and (ncand <= C).all()
    return out, [cand[i, :ncand[i]] for i in range(n)]


def point_sets(dfepe):
    """name -> (F [8,3,3] fp64, P [8,100,2], Q [8,100,2]) float32 points, as the kernel reads them."""
    sc = dfepe.synth.make_scene(8, 100, seed=3, dtype=torch.float64)
    F = sc["F_gt"].numpy()
    m = sc["matches_xy_ori"].numpy().astype(np.float32)
    g = np.broadcast_to(ref.grid(IM_SHAPE)[0], (8, 100, 2))
    return {"grid": (F, g, g), "grid_vs_matches": (F, g, m[:, :, 2:]), "matches": (F, m[:, :, :2], m[:, :, 2:])}


@pytest.fixture(scope="module")
def cases(dfepe):
    """The inputs and the restatement's answer for them, computed once and shared."""
    out = {}
    for name, (F, P, Q) in point_sets(dfepe).items():
        out[name] = (F, P, Q, [ref.correct_matches(F[b], P[b], Q[b]) for b in range(len(F))])
    return out


def rel(a, b, floor=0.0):
    return float((np.abs(a - b) / np.maximum(np.abs(b), 1e-300))[np.abs(a - b) > floor].max(initial=0.0))


def test_the_grid_is_the_references(dfepe):
    g1, g2 = dfepe.compat.utils_misc.get_virt_x1x2_grid(IM_SHAPE)
    assert g1.dtype == np.float32 and g1.shape == (100, 2) and np.array_equal(g1, g2) and g1 is not g2
    assert np.array_equal(g1, ref.grid(IM_SHAPE)[0])
    assert g1[1, 0] == np.float32(1241 * 0.1) and g1[10, 1] == np.float32(376 * 0.1) and g1[99, 0] == np.float32(1241 * 0.9)
    assert np.array_equal(dfepe.compat.utils_misc.get_virt_x1x2_grid([376, 1241, 3])[0], g1)  # image_size with channels


@pytest.mark.parametrize("name", SETS)
def test_restatement_reaches_the_minimum_of_the_pencil_scan(cases, name):
    F, P, Q, R = cases[name]
    worst = max(rel(R[b]["cost"], ref.pencil_min_cost(F[b], P[b], Q[b])) for b in range(len(F)))
    print(f"{name}: minimal cost, sextic route against the scan over the pencil: {worst:.2e} relative")
    assert worst <= 1e-7


@pytest.mark.parametrize("name", SETS)
def test_restatement_output_is_on_the_geometry_and_its_cost_is_the_displacement(cases, name):
    F, P, Q, R = cases[name]
    dist = max(ref.line_distance(F[b], R[b]["p"], R[b]["q"]).max() for b in range(len(F)))
    disp = max(rel(((P[b] - R[b]["p"]) ** 2).sum(1) + ((Q[b] - R[b]["q"]) ** 2).sum(1), R[b]["cost"]) for b in range(len(F)))
    print(f"{name}: distance to the epipolar line {dist:.2e} px, |p-p'|^2 + |q-q'|^2 against the cost {disp:.2e} relative")
    assert dist <= 1e-9
    assert disp <= 1e-7


@pytest.mark.parametrize("name", SETS)
def test_header_agrees_with_the_restatement(emu, cases, name):
    """Cost to 1e-9 relative (absolute floor 1e-12 px^2), positions before float32 rounding to 1e-6 px (seen: 4e-12 px, so
    the fall-back bound from a longdouble polish was not needed), near-ties (none here) capped at 1 % of the points."""
    F, P, Q, R = cases[name]
    cost = pos = 0.0
    ties = 0
    for b in range(len(F)):
        out, _ = emu_correct(emu, F[b], P[b], Q[b])
        assert np.isfinite(out).all()
        cost = max(cost, rel(out[:, 4], R[b]["cost"], floor=1e-12))
        keep = ~R[b]["near_tie"]
        ties += int((~keep).sum())
        pos = max(pos, np.abs(out[keep, :2] - R[b]["p"][keep]).max(), np.abs(out[keep, 2:4] - R[b]["q"][keep]).max())
    print(f"{name}: cost {cost:.2e} relative, position {pos:.2e} px, near-ties {ties} of {P.shape[0] * P.shape[1]}")
    assert ties <= 0.01 * P.shape[0] * P.shape[1]
    assert cost <= 1e-9
    assert pos <= 1e-6


@pytest.mark.parametrize("name", SETS)
def test_every_real_root_is_among_the_headers_candidates(emu, cases, name):
    """A real root of numpy.roots (|imag| <= 1e-9 max(1, |t|)) counts as found when a candidate lies within that same
    1e-9 max(1, |t|) of it; t = infinity is always a candidate."""
    F, P, Q, R = cases[name]
    n_roots = 0
    for b in range(len(F)):
        _, cand = emu_correct(emu, F[b], P[b], Q[b])
        for i, roots in enumerate(R[b]["roots"]):
            assert np.isinf(cand[i]).sum() == 1
            c = cand[i][np.isfinite(cand[i])]
            assert len(c) <= 12
            for t in roots:
                n_roots += 1
                assert len(c) and np.abs(c - t).min() <= 1e-9 * max(1.0, abs(t)), (b, i, t, c)
    assert n_roots >= 2 * P.shape[0] * P.shape[1]  # a sextic with a real root has at least two


def test_points_already_on_the_geometry_stay(emu, dfepe):
    sc = dfepe.synth.make_scene(8, 100, seed=3, dtype=torch.float64)
    F = sc["F_gt"].numpy()
    p, q = sc["pts1_virt_ori"].numpy()[:, :, :2].astype(np.float32), sc["pts2_virt_ori"].numpy()[:, :, :2].astype(np.float32)
    for b in range(8):
        out, _ = emu_correct(emu, F[b], p[b], q[b])
        assert out[:, 4].max() <= 1e-6  # float32 rounding of a pixel coordinate: within 2^-14 px of the geometry
        assert np.abs(out[:, :2] - p[b]).max() <= 2.0 ** -13 and np.abs(out[:, 2:4] - q[b]).max() <= 2.0 ** -13


def test_a_point_on_the_epipole_is_nan_and_its_neighbours_are_not(emu):
    e = np.array([512.0, 128.0, 1.0])
    F = np.array([[0, -e[2], e[1]], [e[2], 0, -e[0]], [-e[1], e[0], 0]])
    g = ref.grid(IM_SHAPE)[0].copy()
    g[37] = (512, 128)
    out, _ = emu_correct(emu, F, g, g)
    assert np.isnan(out[37]).all() and np.isnan(ref.correct_one(F, g[37], g[37])["cost"])
    rest = np.arange(100) != 37
    assert np.isfinite(out[rest]).all()
    r = ref.correct_matches(F, g[rest], g[rest])  # x^T [e]_x x = 0: every pair of equal points is already on the geometry
    assert np.abs(out[rest, :2] - r["p"]).max() <= 1e-6 and out[rest, 4].max() <= 1e-12
    out, _ = emu_correct(emu, np.zeros((3, 3)), g[:4], g[:4])  # no geometry at all: nothing finite arises
    assert np.isnan(out).all()


def test_cabi_argument_checks_without_launching(dfepe):
    L = dfepe._lib.lib()
    x = ctypes.c_void_p(256)  # a non-null address that is never dereferenced: every call below returns before a launch
    call = lambda B, M, stride=9, F=x, p=x, q=x, po=x, qo=x: L.dfepe_correct_matches(None, F, stride, p, q, B, M, po, qo, None)
    assert call(0, 100) == 0 and call(4, 0) == 0 and call(0, 0, stride=0) == 0
    assert call(0, 100, F=None, p=None, q=None, po=None, qo=None) == 0  # empty tensors have no address
    assert call(-1, 100) == -1 and call(4, -1) == -1
    assert call(4, 100, stride=3) == -1 and call(4, 100, stride=-9) == -1 and call(0, 100, stride=1) == -1
    for k in ("F", "p", "q", "po", "qo"):
        assert call(4, 100, **{k: None}) == -1
    assert "dfepe_correct_matches" in dfepe.EXPORTED_SYMBOLS
    assert L.dfepe_version() == 154


def test_no_cpu_path(dfepe):
    with pytest.raises(dfepe.DfepeError):
        dfepe.ops.correct_matches(torch.eye(3), torch.zeros(1, 4, 2), torch.zeros(1, 4, 2))
