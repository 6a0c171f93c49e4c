"""The adjoint of the textbook eight-point solvers without a GPU: the fp64 restatement (tests/eight_point_adjoint_ref.py) against the
reference's own float64 autograd (tests/golden/eight_point_adjoint.npz) and against its 50-digit twin, the condition every scene case
is chosen under, the host build of csrc/eight_point_adjoint_math.h (tests/emu/emu_eight_point_adjoint.cpp, compiled with g++)
through the same check() as the GPU, and the FORCE_110 rank-2 formula against float64 autograd at a generic matrix.  The C ABI's
refusals are made before any HIP call, so they are tested here too."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eight_point_adjoint_cases as ec  # noqa: E402
import eight_point_adjoint_ref as er  # noqa: E402

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EMU_DIR = os.path.join(REPO, "tests", "emu")
CSRC = os.path.join(REPO, "pytorch-deepfepe_amd", "csrc")
F32 = np.float32
INVALID, UNSUPPORTED = -1, -3
SQRT2, NO_ROWNORM, FORCE_110, NO_HARTLEY = 4, 8, 16, 32


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(REPO, "tests", "golden", "eight_point_adjoint.npz"))


@pytest.fixture(scope="module")
def emu():
    out = os.path.join(EMU_DIR, "_build")
    os.makedirs(out, exist_ok=True)
    lib = os.path.join(out, "libemu_eight_point_adjoint.so")
    srcs = [os.path.join(EMU_DIR, "emu_eight_point_adjoint.cpp"), os.path.join(CSRC, "eight_point_adjoint_math.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", f"-I{CSRC}", srcs[0], "-o", lib], check=True)
    L = ctypes.CDLL(lib)
    i, p = ctypes.c_int, ctypes.c_void_p
    L.emu_eight_point_bwd.argtypes = [p, p, p, i, i, i, ctypes.c_uint, p, p, p, p, p]
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def run_emu(L, case, want=("g_X", "g_Y", "g_w")):
    S, B, N = case["S"], case["B"], case["N"]
    got = {"g_X": np.zeros((B, N, 2), F32) if "g_X" in want else None, "g_Y": np.zeros((B, N, 2), F32) if "g_Y" in want else None,
           "g_w": np.zeros((S, B, N), F32) if "g_w" in want else None}
    rc = L.emu_eight_point_bwd(_p(case["X"]), _p(case["Y"]), _p(case["w"]), B, N, S, ec.flags_of(case), _p(case["F_out"]), _p(case["g_F"]),
                               _p(got["g_X"]), _p(got["g_Y"]), _p(got["g_w"]))
    assert rc == 0
    return got


def test_case_list_covers_what_it_says():
    cases = ec.scene_cases()
    assert {c["N"] for c in cases} == set(ec.NS) and {c["S"] for c in cases} == {1, 3} and {c["B"] for c in cases} == set(ec.BATCHES)
    assert {(c["N"], c["essential"], c["normalize"]) for c in cases} == {(N, e, n) for N in ec.NS for e, n in ec.FLAG_COMBOS}
    assert {c["wfam"] for c in cases} == {"none", "range", "zeros"}
    assert {(c["S"], c["B"]) for c in cases} == {(S, B) for S in (1, 3) for B in ec.BATCHES}
    for c in cases:
        if c["wfam"] == "zeros":
            z = (c["w"] == 0.0).sum(-1)
            assert (z >= 1).all() and (c["N"] - z >= 9).all()


def test_every_scene_case_meets_the_condition():
    """(lam_8 - lam_9) / lam_1 >= 1e-6 for every problem and, without FORCE_110, (s2 - s3) / s1 >= 1e-3: what the bound of check()
    rests on.  The seeds are chosen so (eight_point_adjoint_cases.make); this is the assertion."""
    for case in ec.scene_cases():
        r = ec.reference(case)
        assert (r.gap_lam >= ec.MIN_GAP_LAM).all(), (ec.name_of(case), float(r.gap_lam.min()))
        if not case["essential"]:
            assert (r.gap_s >= ec.MIN_GAP_S).all(), (ec.name_of(case), float(r.gap_s.min()))
        assert np.isfinite(r.gX).all() and np.isfinite(r.gY).all() and np.isfinite(r.gw).all()


def _twin_of(case, s, b):
    return er.twin(case["X"][b], case["Y"][b], None if case["w"] is None else case["w"][s, b], case["essential"], case["normalize"],
                   case["F_out"][s, b], case["g_F"][s, b])


def test_restatement_within_1e9_of_its_twin():
    """Problem (0, 0) and the last problem of every scene case: per output tensor within 1e-9 max |g| of the 50-digit twin."""
    worst = 0.0
    for case in ec.scene_cases():
        r = ec.reference(case)
        for s, b in {(0, 0), (case["S"] - 1, case["B"] - 1)}:
            tX, tY, tw = _twin_of(case, s, b)
            for name, got, ref in (("gX", r.gXs[s, b], tX), ("gY", r.gYs[s, b], tY), ("gw", r.gw[s, b], tw)):
                if name == "gw" and case["N"] == 8:
                    # the N = 8 rule (g_w written as 0): the twin, which does not apply it, finds nothing above its 50 digits
                    assert np.all(got == 0.0) and np.abs(ref).max() <= 1e-30 * np.abs(tX).max(), (ec.name_of(case), np.abs(ref).max())
                    continue
                err, top = np.abs(got - ref).max(), np.abs(ref).max()
                assert err <= ec.TWIN_BOUND * top, (ec.name_of(case), s, b, name, err, top)
                worst = max(worst, err / top if top > 0 else 0.0)
    print(f"restatement vs twin: worst {worst:.2e} of max |g|")


def test_restatement_reproduces_the_reference(golden):
    """The reference's own float64 autograd through _F_from_XY / _E_from_XY (its Hartley transforms detached), to 1e-9 relative."""
    cases = ec.golden_cases()
    assert len(cases) == 32
    for k, c in enumerate(cases):
        for key in ("X", "Y", "g"):
            assert np.array_equal(golden[f"{k}_{key}"], c[key]), (k, key)
        assert (c["ws"] is None) == (f"{k}_ws" not in golden.files)
        if c["ws"] is not None:
            assert np.array_equal(golden[f"{k}_ws"], c["ws"])
        r = er.problem(c["X"], c["Y"], c["ws"], c["essential"], c["normalize"], golden[f"{k}_out"], c["g"])
        assert np.abs(r.out - golden[f"{k}_out"]).max() <= 1e-9 * np.abs(golden[f"{k}_out"]).max(), k
        pairs = [("gX", r.gX), ("gY", r.gY)] + ([("gws", r.gw)] if c["ws"] is not None else [])
        for name, got in pairs:
            ref = golden[f"{k}_{name}"]
            assert np.abs(got - ref).max() <= 1e-9 * np.abs(ref).max(), (k, name, float(np.abs(got - ref).max() / np.abs(ref).max()))


def test_golden_separates_the_two_hartley_rules(golden):
    """With normalize, a gradient that passes through the centroid and the scale is at least 4 yardsticks from the reference's on
    every golden case: the one-yardstick comparison of the GPU test is a test of the rule.  (Finite differences of the restatement's
    forward WITH moving transforms, central, fp64: a check of the data, independent of any implementation of the adjoint.)"""
    for k, c in enumerate(ec.golden_cases()):
        if not c["normalize"]:
            continue
        ref_out, g = golden[f"{k}_out"], c["g"].astype(np.float64)
        X = c["X"].astype(np.float64)

        def value(Xv):
            out = er.problem(Xv, c["Y"], c["ws"], c["essential"], True, ref_out, None).out
            return (g * out).sum()

        n = int(np.abs(golden[f"{k}_gX"]).sum(1).argmax())
        fd = np.empty(2)
        for j in range(2):
            h = 1e-6
            Xp, Xm = X.copy(), X.copy()
            Xp[n, j] += h
            Xm[n, j] -= h
            fd[j] = (value(Xp) - value(Xm)) / (2 * h)
        sep = np.abs(fd - golden[f"{k}_gX"][n]).max() / float(golden[f"{k}_yard_gX"])
        assert sep >= 4.0, (k, sep)


def test_force_110_formula_against_autograd_at_a_generic_matrix():
    """M = U diag(1,1,0) V^T of a generic 3x3 (three distinct singular values, none small): the header's P against float64 autograd,
    and the rank-2 formula of SURVEY.md A.3 likewise."""
    import torch

    rng = np.random.default_rng(11)
    for essential in (True, False):
        for _ in range(5):
            F0 = torch.tensor(rng.standard_normal((3, 3)), requires_grad=True)
            G = rng.standard_normal((3, 3))
            U, S, Vh = torch.linalg.svd(F0)
            D = torch.diag(S.new_tensor([1.0, 1.0, 0.0])) if essential else torch.diag(S * S.new_tensor([1.0, 1.0, 0.0]))
            ((U @ D @ Vh) * torch.tensor(G)).sum().backward()
            Un, sn, Vn = U.detach().numpy(), S.detach().numpy(), Vh.detach().numpy().T
            ours = Un @ er.rank2_P(Un.T @ G @ Vn, sn, essential) @ Vn.T
            assert np.abs(ours - F0.grad.numpy()).max() <= 1e-11 * np.abs(F0.grad.numpy()).max()


def test_host_build_passes_the_check(emu):
    for case in ec.scene_cases() + ec.exact_cases():
        ec.check(case, run_emu(emu, case))


def test_svd3_of_the_host_build_and_its_guard_at_rank_one(emu):
    """F = U diag(s) V^T with orthonormal factors at generic matrices; at a rank-1 matrix (s2 = s3 = 0) the guard rule leaves u2 = 0:
    nothing is a NaN of the step's own making."""
    rng = np.random.default_rng(3)
    dp = ctypes.POINTER(ctypes.c_double)
    emu.emu_eight_point_svd3.argtypes = [dp] * 4
    emu.emu_eight_point_svd3.restype = None

    def svd3(F):
        F = np.ascontiguousarray(F, np.float64)
        U, s, V = np.empty((3, 3)), np.empty(3), np.empty((3, 3))
        emu.emu_eight_point_svd3(*(a.ctypes.data_as(dp) for a in (F, U, s, V)))
        return U, s, V

    for _ in range(5):
        F = rng.standard_normal((3, 3))
        U, s, V = svd3(F)
        assert np.abs(U @ np.diag(s) @ V.T - F).max() <= 1e-14 and np.abs(s - np.linalg.svd(F, compute_uv=False)).max() <= 1e-14
        assert np.abs(U.T @ U - np.eye(3)).max() <= 1e-14 and np.abs(V.T @ V - np.eye(3)).max() <= 1e-14
    a, b = np.array([1.0, 2.0, -2.0]), np.array([2.0, -1.0, 2.0])
    U, s, V = svd3(np.outer(a, b))
    assert np.isfinite(U).all() and np.isfinite(V).all() and abs(s[0] - 9.0) <= 1e-13 and s[1] <= 1e-13 and s[2] <= 1e-13
    assert np.abs(s[0] * np.outer(U[:, 0], V[:, 0]) - np.outer(a, b)).max() <= 1e-14


def test_exact_essential_geometry_is_finite_where_svd_backward_is_not():
    """The exact family has s1 = s2 up to the float32 rounding of the points; the FORCE_110 adjoint does not divide by s1 - s2, so the
    twin (the reference of this family) is of ordinary size."""
    for case in ec.exact_cases():
        r = ec.reference(case)
        for b in range(case["B"]):
            s = er.problem(case["X"][b], case["Y"][b], None, True, False, None, None).s
            assert (s[0] - s[1]) / s[0] < 1e-5
        assert np.isfinite(r.gX).all() and np.isfinite(r.gY).all() and np.isfinite(r.gw).all()


def test_each_output_alone_and_a_non_finite_point_stays_local(emu):
    case = ec.nonfinite_case()
    full = run_emu(emu, case)
    ec.check(case, full)
    assert np.isnan(full["g_X"][1]).all()
    clean = dict(case, X=case["X"].copy())
    clean.pop("_ref", None)
    clean["X"][1, case["N"] // 2, 0] = 0.0
    other = run_emu(emu, clean)
    for key in ("g_X", "g_Y"):
        assert np.array_equal(full[key][[0, 2]], other[key][[0, 2]])
    assert np.array_equal(full["g_w"][:, [0, 2]], other["g_w"][:, [0, 2]])
    for key in ("g_X", "g_Y", "g_w"):
        assert np.array_equal(run_emu(emu, case, want=(key,))[key], full[key], equal_nan=True)


# ---- the C ABI: refusals before any HIP call, the workspace ---------------------------------------------------------------------------
def _addr(align=0):
    buf = ctypes.create_string_buffer(64)  # host memory: only looked at, never dereferenced before the refusals
    _addr.keep.append(buf)
    return (ctypes.addressof(buf) + 15) // 16 * 16 + align


_addr.keep = []


def test_symbols_and_version(dfepe):
    L = dfepe._lib.lib()
    raw = ctypes.CDLL(dfepe.LIB_PATH)
    for name in ("dfepe_eight_point_bwd_workspace_bytes", "dfepe_eight_point_bwd"):
        assert hasattr(raw, name) and name in dfepe.EXPORTED_SYMBOLS
    assert L.dfepe_version() == 154


def test_workspace_size(dfepe):
    L = dfepe._lib.lib()
    for B, N, S in ((1, 8, 1), (70, 129, 1), (3, 10, 2), (8, 1000, 16), (0, 10, 3), (-1, 10, 3), (2, 0, 3), (2, 10, 0)):
        want = S * B * N * 4 * 8 if (B > 0 and N > 0 and S > 1) else 0
        assert L.dfepe_eight_point_bwd_workspace_bytes(B, N, S) == want, (B, N, S)


def test_refusals_without_a_launch_in_the_documented_order(dfepe):
    L = dfepe._lib.lib()
    a = _addr()
    base = SQRT2 | NO_ROWNORM

    def f(B=2, N=10, S=1, flags=base, X=a, Y=a, w=None, Fo=a, g=a, gX=a, gY=a, gw=a, ws=None):
        return L.dfepe_eight_point_bwd(None, X, Y, w, B, N, S, flags, Fo, g, gX, gY, gw, ws)

    assert f(B=-1) == INVALID and f(N=7) == INVALID and f(N=-1) == INVALID and f(S=0) == INVALID
    for bad in (0, SQRT2, NO_ROWNORM, base | 1, base | 2, base | 64, base | 128, base | (1 << 20)):
        assert f(flags=bad) == INVALID, bad
    for extra in (0, FORCE_110, NO_HARTLEY, FORCE_110 | NO_HARTLEY):
        assert f(B=0, flags=base | extra) == 0
    assert f(B=0, X=None, Y=None, Fo=None, g=None, gX=None, gY=None, gw=None) == 0       # nothing to do: before the pointer checks
    assert f(B=0, N=7) == INVALID and f(B=0, flags=SQRT2) == INVALID and f(B=0, S=0) == INVALID     # ... and after the shape and flags
    for k in ("X", "Y", "Fo", "g"):
        assert f(**{k: None}) == INVALID
    assert f(gX=None, gY=None, gw=None) == INVALID
    for k in ("X", "Y", "gX", "gY"):
        assert f(**{k: _addr(4)}) == INVALID
    assert f(S=2) == INVALID and f(S=2, ws=_addr(8)) == INVALID                           # several sets need the 16-byte workspace
    assert f(N=2 ** 30, B=3) == UNSUPPORTED and f(N=2 ** 29, B=2, S=3, ws=a) == UNSUPPORTED
    assert f(N=2 ** 30, B=3, X=None) == INVALID                                             # pointers before the size


def test_python_layer_refuses_cpu_tensors(dfepe):
    import torch

    X = torch.zeros(2, 9, 2, requires_grad=True)
    with pytest.raises(dfepe.DfepeError):
        dfepe.ops.eight_point(X, X, None, essential=True)
    with pytest.raises(dfepe.DfepeError):
        dfepe.compat.utils_F._F_from_XY(X[0], X[0])
