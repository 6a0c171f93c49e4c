"""The odometry evaluation without a GPU: the fp64 restatement (tests/odometry_ref.py) against the reference's own output
(tests/golden/odometry.npz, made by tests/golden/make_golden_odometry.py); the arithmetic header csrc/odometry_math.h, compiled
for the host with g++ through tests/emu/emu_odometry.cpp and walking the kernel's own association order for several launch plans,
against the restatement inside check()'s bounds; check()'s teeth; and the C ABI's refusals that need no launch.

Figures seen here (printed by the tests).  Restatement against the golden file: trajectory within 0.22 of golden_chain_tol (6.0e-12
at entries of size 307, n = 300), snippet errors equal as float32, scale within 0.11 of golden_scale_tol.  Chain spread (sequential
against tree order of the restatement, the unit of check()'s bound): 2.0e-13 at entries of size 63 for n = 1591 with rotations up
to pi, 0 for k <= 2.  Host build of the header in the shipped plan (256 lanes x 8 poses): at most 0.26 of the bound from the
sequential restatement, and bit-equal to it for the first 8 poses of every sequence; its snippet results equal the restatement's
bit for bit except where atan2 of libm and of numpy differ in the last place."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import odometry_cases as C  # noqa: E402
import odometry_ref as R  # noqa: E402

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EMU_DIR = os.path.join(REPO, "tests", "emu")
CSRC = os.path.join(REPO, "pytorch-deepfepe_amd", "csrc")
PLANS = [(C.THREADS, C.CHUNK), (64, 1), (128, 3), (256, 1)]
CPU_CHAIN = ["n0", "n1", "n2", "n63", "n64", "n65", "n7", "n8", "n9", "n511", "n512", "n513", "n1591", "n2047", "n2048", "n2049",
             "ragged", "ragged_c2b_seq", "ragged_c2b_pose", "n513_c2b_pose"]


@pytest.fixture(scope="module")
def emu():
    out = os.path.join(EMU_DIR, "_build")
    os.makedirs(out, exist_ok=True)
    lib = os.path.join(out, "libemu_odometry.so")
    srcs = [os.path.join(EMU_DIR, "emu_odometry.cpp"), os.path.join(CSRC, "odometry_math.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", f"-I{CSRC}", srcs[0], "-o", lib], check=True)
    L = ctypes.CDLL(lib)
    P = ctypes.c_void_p
    L.emu_pose_chain.argtypes = [P, ctypes.c_int, P, ctypes.c_long, ctypes.c_int, ctypes.c_int, P]
    L.emu_pose_chain.restype = ctypes.c_int
    L.emu_snippet_errors.argtypes = [P, P, ctypes.c_int, ctypes.c_int, ctypes.c_int, P, P, P, P]
    L.emu_snippet_errors.restype = None
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def emu_chain(L, case, threads, chunk):
    S, n_max = case["rel"].shape[:2]
    out = np.full((S, n_max + 1, 12), C.SENTINEL)
    for s, n in enumerate(case["lengths"]):
        rel = np.ascontiguousarray(case["rel"][s])
        c = None if case["cam2body"] is None else np.ascontiguousarray(case["cam2body"][s])
        buf = np.zeros((int(n) + 1, 12))
        assert L.emu_pose_chain(_p(rel), int(n), _p(c), case["c2b_stride"], threads, chunk, _p(buf)) == 0
        out[s, :n + 1] = buf
    return out


def emu_snippets(L, case):
    got = C.expected(case)
    for s, nw in enumerate(case["windows"]):
        nw, Ls = int(nw), case["L"]
        e64, sc, al, comp = np.zeros((nw, 2)), np.zeros(nw), np.zeros((nw, 12)), np.zeros((nw, Ls, 12))
        L.emu_snippet_errors(_p(np.ascontiguousarray(case["est"][s])), _p(np.ascontiguousarray(case["gt"][s])), nw, Ls,
                             int(case["compensate"]), _p(e64), _p(sc), _p(al), _p(comp))
        with np.errstate(all="ignore"):
            got["errors"][s, :nw] = e64.astype(np.float32)
        got["scale"][s, :nw], got["aligned"][s, :nw], got["compensated"][s, :nw] = sc, al, comp
        got["stats"][s] = R.stats(got["errors"][s, :nw])
    return got


# ---- the restatement against the reference's own output ------------------------------------------------------------------------
@pytest.mark.parametrize("s", [0, 1])
def test_restatement_reproduces_the_references_trajectory(golden, s):
    g = golden("odometry")
    rel, c = g[f"rel_cam_{s}"].astype(np.float64).reshape(-1, 12), g[f"cam2body_{s}"].astype(np.float64).reshape(12)
    body = R.body_poses(rel, c)
    want_body = g[f"rel_body_{s}"].reshape(-1, 12)
    assert np.abs(body - want_body).max() <= 16 * R.U * np.abs(want_body).max()  # two products and an inverse of entries <= 3
    want = g[f"abs_{s}"].reshape(-1, 12)
    for got in (R.chain_sequential(rel, c), R.chain_tree(rel, c), R.chain_sequential(want_body)):
        d, tol = np.abs(got - want).max(axis=1), R.golden_chain_tol(want)
        print(f"sequence {s}: restatement against get_abs_poses {d.max():.2e} (entries up to {np.abs(want).max():.0f}), worst "
              f"ratio to the bound {(d[1:] / tol[1:]).max():.2f}")
        assert (d <= tol).all()
        assert np.array_equal(got[0], want[0])


@pytest.mark.parametrize("s", [0, 1])
@pytest.mark.parametrize("L", [5, 3])
def test_restatement_reproduces_pose_seq_ate(golden, s, L):
    g = golden("odometry")
    est, gt = g[f"abs_{s}"].reshape(-1, 12), g[f"gt_{s}"].astype(np.float64).reshape(-1, 12)
    want_e, want_s = g[f"errors{L}_{s}"], g[f"scale{L}_{s}"]
    assert len(want_e) == len(est) - L  # the reference never scores the last window
    r = R.snippet_errors(est, gt, len(est) - L, L)
    er = np.abs(r["errors"].astype(np.float64) - want_e) / R.error_tol(want_e)
    sr = np.abs(r["scale"] - want_s) / (R.golden_scale_tol(r["kappa"], L) * np.abs(want_s))
    print(f"sequence {s}, L = {L}: errors {er.max():.2f} float32 spacings, scale {sr.max():.2f} of its bound, kappa <= {r['kappa'].max():.4f}")
    assert er.max() <= 1.0 and sr.max() <= 1.0 and r["kappa"].max() < 1e3 and not r["degenerate"].any()
    if L == 5:
        want_a = g[f"aligned5_{s}"].reshape(-1, 12)
        tol = R.golden_scale_tol(r["kappa"], L)[:, None] * np.abs(want_a)
        assert (np.abs(r["aligned"] - want_a) <= tol).all()


@pytest.mark.parametrize("s", [0, 1])
def test_restatement_reproduces_compensate_poses_and_compute_pose_error(golden, s):
    g = golden("odometry")
    est, gt = g[f"abs_{s}"].reshape(-1, 12)[10:15], g[f"gt_{s}"].astype(np.float64).reshape(-1, 12)[10:15]
    r = R.snippet_errors(est, gt, 1, 5)
    want = g[f"comp_est_{s}"].reshape(5, 12)
    assert np.abs(r["compensated"][0] - want).max() <= 8 * R.U * np.abs(want).max()
    rg = R.snippet_errors(gt, gt, 1, 5)
    assert np.abs(rg["compensated"][0] - g[f"comp_gt_{s}"].reshape(5, 12)).max() <= 8 * R.U * np.abs(g[f"comp_gt_{s}"]).max()
    # compute_pose_error on its own: the compensated snippets scored as given
    r2 = R.snippet_errors(g[f"comp_est_{s}"].reshape(5, 12), g[f"comp_gt_{s}"].reshape(5, 12), 1, 5, compensated=False)
    ate, re, scale = g[f"cpe_{s}"]
    assert abs(r2["scale"][0] - scale) <= R.golden_scale_tol(r2["kappa"], 5)[0] * abs(scale)
    assert abs(r2["errors64"][0, 0] - ate) <= R.spacing32(ate) and abs(r2["errors64"][0, 1] - re) <= R.spacing32(re) + R.RE_FLOOR


# ---- the header, compiled for the host, in the kernel's association order ------------------------------------------------------
def test_shipped_plan_is_the_one_the_cases_aim_at(dfepe):
    assert (dfepe._lib.POSE_CHAIN_THREADS, dfepe._lib.POSE_CHAIN_CHUNK) == (C.THREADS, C.CHUNK)
    assert dfepe._lib.SNIPPET_MAX_L == 64


@pytest.mark.parametrize("name", CPU_CHAIN)
def test_header_in_kernel_order_agrees_with_the_sequential_restatement(emu, name):
    case = C.chain_case(name)
    for threads, chunk in PLANS:
        got = emu_chain(emu, case, threads, chunk)
        fig = C.check(case, got)
        if (threads, chunk) == (C.THREADS, C.CHUNK):
            print(f"{name}: plan {threads} x {chunk}: {fig['max_diff']:.2e} from sequential (spread of the restatement's two orders "
                  f"{fig['max_spread']:.2e}, entries up to {fig['max_entry']:.0f}), worst ratio to the bound {fig['worst_ratio']:.2f}")
            for s, n in enumerate(case["lengths"]):  # a lane's own chunk from the identity: the sequential loop, bit for bit
                k = min(int(n), chunk) + 1
                assert np.array_equal(got[s, :k], case["seq"][s][:k])
    assert emu.emu_pose_chain(None, 0, None, 0, 96, 4, None) == -1 and emu.emu_pose_chain(None, 0, None, 0, 64, 0, None) == -1


@pytest.mark.parametrize("name", list(C.SNIPPET_CASES))
def test_header_snippets_agree_with_the_restatement(emu, name):
    case = C.snippet_case(name)
    fig = C.check(case, emu_snippets(emu, case))
    print(f"{name}: errors {fig['err_ratio']:.2f} of a float32 spacing, scale / aligned {fig['scale_ratio']:.2f} of kappa 2^-52 "
          f"(kappa <= {fig['kappa']:.4f}), stats {fig['stats_ratio']:.2f} of their bound, {fig['degenerate']} degenerate windows")
    if name == "L1":
        assert fig["degenerate"] == sum(case["windows"])
    if name == "L5_stationary_gt":
        assert fig["degenerate"] == 1


# ---- check() has teeth -----------------------------------------------------------------------------------------------------------
def _wrong_chain(case, **kw):
    out = C.expected(case)
    for s, n in enumerate(case["lengths"]):
        c = None if case["cam2body"] is None else (case["cam2body"][s] if case["c2b_stride"] == 0 else case["cam2body"][s, :n])
        out[s, :n + 1] = R.chain_sequential(case["rel"][s, :n], c, **kw)
    return out


def test_check_accepts_the_reference_itself():
    for name in ("n65", "ragged_c2b_pose"):
        C.check(C.chain_case(name), C.expected(C.chain_case(name)))
    for name in C.SNIPPET_CASES:
        C.check(C.snippet_case(name), C.expected(C.snippet_case(name)))


def test_check_rejects_swapped_operands():
    case = C.chain_case("n65")
    with pytest.raises(AssertionError, match="from the sequential result"):
        C.check(case, _wrong_chain(case, swapped=True))
    assert np.array_equal(_wrong_chain(case, swapped=True)[0, :2], C.expected(case)[0, :2])  # one pose has no order


def test_check_rejects_the_rigid_inverse():
    for name in ("ragged_c2b_seq", "n65"):  # sheared 3x3 blocks, and rotations that are rotations only to float32
        case = C.chain_case(name)
        with pytest.raises(AssertionError, match="from the sequential result"):
            C.check(case, _wrong_chain(case, rigid=True))


@pytest.mark.parametrize("seam", [C.CHUNK, C.WAVE_CAP, C.TILE])
def test_check_rejects_a_dropped_seam_pose(seam):
    case = C.chain_case("n2049")
    with pytest.raises(AssertionError, match=f"pose {seam + 1} is"):
        C.check(case, _wrong_chain(case, drop=seam))


def test_check_rejects_a_write_past_the_length():
    case = C.chain_case("ragged")
    got = C.expected(case)
    got[1, 66] = got[1, 65]  # the sequence of 65 poses has entries 0 .. 65
    with pytest.raises(AssertionError, match="past its length"):
        C.check(case, got)


def test_check_rejects_the_last_window_kept():
    case = C.snippet_case("L5")
    got = C.expected(case)
    s = 1  # the sequence with one window: score a second one, as a loop to len - L + 1 would
    r = R.snippet_errors(case["est"][s], case["gt"][s], 2, 5)
    got["errors"][s, :2], got["scale"][s, :2], got["aligned"][s, :2] = r["errors"], r["scale"], r["aligned"]
    with pytest.raises(AssertionError, match="past the last window"):
        C.check(case, got)
    full = R.snippet_errors(case["est"][4], case["gt"][4], C.SNIP_M - 5 + 1, 5)  # every window of the sequence, the last included
    got = C.expected(case)
    got["errors"] = np.concatenate([got["errors"], np.full((5, 1, 2), C.SENTINEL, np.float32)], axis=1)
    got["errors"][4] = full["errors"]
    with pytest.raises(AssertionError):
        C.check(case, got)


def test_check_rejects_est_and_gt_in_the_documented_roles():
    for name in ("L5", "L5_as_given", "L64"):
        case = C.snippet_case(name)
        got = C.expected(case)
        for s, nw in enumerate(case["windows"]):
            r = R.snippet_errors(case["est"][s], case["gt"][s], int(nw), case["L"], compensated=case["compensate"], documented_roles=True)
            got["errors"][s, :nw], got["scale"][s, :nw], got["aligned"][s, :nw] = r["errors"], r["scale"], r["aligned"]
            got["stats"][s] = R.stats(r["errors"])
        with pytest.raises(AssertionError, match="times its bound"):
            C.check(case, got)


def test_check_rejects_a_trapped_degenerate_window_and_wrong_stats():
    case = C.snippet_case("L5_stationary_gt")
    got = C.expected(case)
    assert np.isnan(got["errors"][0, 10, 0]) and np.isnan(got["stats"][0, 0])
    got["errors"][0, 10, 0], got["scale"][0, 10] = 0.0, 1.0
    with pytest.raises(AssertionError, match="pattern differs"):
        C.check(case, got)
    case = C.snippet_case("L5")
    got = C.expected(case)
    got["stats"][4, 1] = np.sqrt(got["stats"][4, 1] ** 2 * 125 / 124)  # the sample standard deviation instead of the population's
    with pytest.raises(AssertionError, match="stats"):
        C.check(case, got)


# ---- the C ABI's refusals that need no launch ----------------------------------------------------------------------------------
def test_pose_chain_argument_checks_without_launching(dfepe):
    L = dfepe._lib.lib()
    x = ctypes.c_void_p(256)  # a non-null address that is never dereferenced: every call below returns before a launch
    call = lambda S, n, stride=0, rel=x, out=x, c=None: L.dfepe_pose_chain(None, rel, None, c, stride, S, n, out)
    assert call(0, 100) == 0 and call(0, 0) == 0 and call(0, 5, rel=None, out=None) == 0
    assert call(-1, 100) == -1 and call(4, -1) == -1
    assert call(4, 100, stride=3) == -1 and call(0, 100, stride=9) == -1 and call(4, 100, stride=-12, c=x) == -1
    assert call(4, 100, rel=None) == -1 and call(4, 100, out=None) == -1 and call(4, 0, out=None) == -1
    assert call(1, 2 ** 31 // 12) == -3
    assert "dfepe_pose_chain" in dfepe.EXPORTED_SYMBOLS and L.dfepe_version() == 154


def test_snippet_errors_argument_checks_without_launching(dfepe):
    L = dfepe._lib.lib()
    x = ctypes.c_void_p(256)
    names = ("est", "gt", "windows", "errors", "scale", "aligned", "stats")

    def call(S, m, W, Ls, **kw):
        a = {k: x for k in names}
        a.update(kw)
        return L.dfepe_snippet_errors(None, a["est"], a["gt"], a["windows"], S, m, W, Ls, 0, a["errors"], a["scale"], a["aligned"], None,
                                      a["stats"])

    assert call(0, 100, 95, 5) == 0 and call(0, 0, 0, 1) == 0 and call(0, 100, 95, 5, **{k: None for k in names}) == 0
    assert call(-1, 100, 95, 5) == -1 and call(2, -1, 95, 5) == -1 and call(2, 100, -1, 5) == -1
    assert call(2, 100, 95, 0) == -3 and call(2, 100, 36, 65) == -3 and call(2, 100, 95, -5) == -3 and call(0, 100, 95, 65) == -3
    for k in names:
        assert call(2, 100, 95, 5, **{k: None}) == -1
    assert "dfepe_snippet_errors" in dfepe.EXPORTED_SYMBOLS and L.dfepe_version() == 154


def test_ops_refuse_on_the_host(dfepe):
    import torch
    with pytest.raises(dfepe.DfepeError):
        dfepe.ops.pose_chain(torch.zeros(1, 4, 3, 4, dtype=torch.float64))
    with pytest.raises(dfepe.DfepeError):
        dfepe.ops.snippet_errors(torch.zeros(1, 9, 3, 4), torch.zeros(1, 9, 3, 4))
    assert dfepe.compat.eval_tools.Exp_table_processor.pose_seq_ate.__name__ == "pose_seq_ate"
    assert np.allclose(dfepe.compat.eval_tools.relative_pose_cam_to_body(np.eye(4), np.eye(4)), np.eye(4))
