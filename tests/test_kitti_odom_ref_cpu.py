"""The KITTI odometry table without a GPU: the fp64 restatement (tests/kitti_odom_ref.py) against the data the reference ships for
this stage (tests/golden/kitti_odom.npz, made by tests/golden/make_golden_kitti_odom.py): its per-segment error rows and its five
published numbers per sequence; the other four alignments shown NOT to give those numbers; the margins of every test input's
segment ends; the per-item arithmetic csrc/trajectory_math.h, compiled for the host with g++ through tests/emu/emu_trajectory.cpp,
against the restatement inside check()'s bounds; check()'s teeth; and the C ABI's refusals that need no launch.

Figures seen here (printed by the tests).  Restatement against the shipped rows: at most 3.7e-15 absolute, 958 / 464 / 958 / 464
rows; against the twenty published numbers: within 4.8e-4 of the printed value except RPE (m) of deepF 10 (0.25242 against 0.253).
Spread of the restatement's two orders on the golden sequences (scale_7dof): t_rel 3.4e-14, r_rel 5.9e-14, ATE 3.9e-13 m,
RPE 4.5e-15 m and 1.7e-13 deg, scale c 1.6e-15; margins of the segment ends >= 3.7e-4 m (09) and 2.8e-3 m (10) against bounds of
1.2e-9 and 4.9e-10."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kitti_odom_cases as C  # noqa: E402
import kitti_odom_ref as K  # noqa: E402

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EMU_DIR = os.path.join(REPO, "tests", "emu")
CSRC = os.path.join(REPO, "pytorch-deepfepe_amd", "csrc")
KEYS = [(r, q) for r in C.RUNS for q in C.SEQS]


# ---- the restatement against the shipped data ----------------------------------------------------------------------------------
@pytest.mark.parametrize("run,seq", KEYS)
def test_restatement_reproduces_the_shipped_segment_rows(golden, run, seq):
    g = golden("kitti_odom")
    ref = K.evaluate(g[f"est_{run}_{seq}"], g[f"gt_{seq}"], "scale_7dof")
    rows, want = ref["seg"]["rows"][ref["seg"]["valid"]], g[f"errors_{run}_{seq}"]
    assert rows.shape == want.shape and len(rows) == (958 if seq == "09" else 464)
    assert np.array_equal(rows[:, 0], want[:, 0]) and np.array_equal(rows[:, 3], want[:, 3])
    # first frame, length and speed are equal; the translation column is within 1e-12 of each entry.  The rotation column is
    # arccos(a) / len with a within a few roundings of 1: an angle of 1e-3 rad is known to 2^-52 / 1e-3 = 2e-13 at best, 2e-10 of
    # itself, so "1e-12 relative" cannot hold entry by entry for ANY fp64 evaluation (seen: 4.8e-12 .. 8.5e-11 for the four
    # orders of the restatement, at absolute differences <= 1.3e-15).  It is held to 1e-12 of the entry plus what eight roundings
    # of the arccos argument (the trace, the subtraction and the division, on both sides) do to the angle: angle_tol.
    with np.errstate(all="ignore"):
        rel = np.abs(rows - want) / np.abs(want)
    theta = want[:, 1] * want[:, 3]
    rot_tol = 1e-12 * want[:, 1] + K.angle_tol(np.cos(theta), 8 * K.U) / want[:, 3]
    print(f"{run} {seq}: {len(rows)} rows, largest difference {np.abs(rows - want).max():.1e}; translation column {rel[:, 2].max():.1e} "
          f"relative, rotation column {rel[:, 1].max():.1e} relative = {(np.abs(rows - want)[:, 1] / rot_tol).max():.2f} of its bound")
    assert np.array_equal(rows[:, 4], want[:, 4]) and (rel[:, 2] <= 1e-12).all()
    assert (np.abs(rows - want)[:, 1] <= rot_tol).all()


@pytest.mark.parametrize("run,seq", KEYS)
def test_restatement_reproduces_the_published_numbers(golden, run, seq):
    g = golden("kitti_odom")
    got, want = K.evaluate(g[f"est_{run}_{seq}"], g[f"gt_{seq}"], "scale_7dof")["summary"], g[f"result_{run}_{seq}"]
    print(f"{run} {seq}: restated {got}, published {want}")
    C.assert_published(got, want, run, seq)


@pytest.mark.parametrize("run,seq", KEYS)
def test_the_alignment_is_pinned_by_the_published_ate(golden, run, seq):
    g = golden("kitti_odom")
    for mode in K.MODES:
        ate = K.evaluate(g[f"est_{run}_{seq}"], g[f"gt_{seq}"], mode)["summary"][2]
        if mode == "scale_7dof":
            assert abs(ate - g[f"result_{run}_{seq}"][2]) <= 5.5e-4
        else:
            assert abs(ate - g[f"result_{run}_{seq}"][2]) > 1.0, (mode, ate)


def test_no_segment_end_of_any_test_input_is_undecided():
    cases = [C.golden_case()] + [C.case(name) for name in C.CASES]
    for c in cases:
        for s, (ref, alt, b) in enumerate(c["ref"]):
            seg = ref["seg"]
            if len(seg["margin"]):
                print(f"{c['name']}[{s}]: smallest margin {seg['margin'].min():.2e} m against a bound of {K.dist_bound(seg['dist']):.1e} m")
            assert len(K.undecided(seg)) == 0
            assert np.array_equal(seg["last"], alt["seg"]["last"])  # the other summation order places every end the same
    assert C.case("short_of_100m")["ref"][0][0]["count"] == 0 and C.case("past_100m")["ref"][0][0]["count"] == 1
    assert np.array_equal(C.case("short_of_100m")["ref"][0][0]["summary"][:2], [0.0, 0.0])
    assert C.case("n513")["ref"][0][0]["count"] % 64 != 0 and len(C.case("n513")["ref"][0][0]["seg"]["first"]) % 64 != 0


def test_the_special_cases_are_what_they_claim():
    c = C.case("same_motion", "none")
    e, g = c["ref"][0][0]["align"]["est"], c["ref"][0][0]["align"]["gt"]
    E = K.mul(K.inv(K.mul(K.inv(g[:-1], "closed"), g[1:]), "closed"), K.mul(K.inv(e[:-1], "closed"), e[1:]))
    raw = (((E[:, 0] + E[:, 5]) + E[:, 10]) - 1.0) / 2.0
    assert (raw > 1.0).any()  # without the clamp arccos would give NaN here
    assert (c["ref"][0][0]["rpe_r"][raw >= 1.0] == 0.0).all() and np.isfinite(c["ref"][0][0]["summary"]).all()
    c = C.case("mirrored", "7dof")
    s = c["ref"][0][0]["align"]["sums"]
    Um, _, Vt = np.linalg.svd(s["C"])
    assert np.linalg.det(Um) * np.linalg.det(Vt) < 0
    assert abs(np.linalg.det(c["ref"][0][0]["align"]["r"]) - 1.0) < 1e-12
    c = C.case("stationary_est")
    assert not np.isfinite(c["ref"][0][0]["align"]["c"]) and not np.isfinite(c["ref"][0][0]["summary"][2])
    c = C.case("collinear")
    D = np.linalg.svd(c["ref"][0][0]["align"]["sums"]["C"])[1]
    assert D[1] <= 1e-12 * D[0] and np.isfinite(c["ref"][0][0]["align"]["c"])
    for name, zero in (("planar", (0, 1)), ("planar_est", (1,)), ("planar_gt", (0,))):  # axes along which C has a zero slice
        al = C.case(name, "7dof")["ref"][0][0]["align"]
        Cm, D = al["sums"]["C"], np.linalg.svd(al["sums"]["C"])[1]
        assert all(not np.moveaxis(Cm, ax, 0)[1].any() for ax in zero) and D[2] == 0.0 and D[1] > 1e-4 * D[0]
        assert np.abs(al["r"] @ al["r"].T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(al["r"]) - 1.0) < 1e-12
    assert [int(C.case(n)["gt_len"][0]) > 4096 for n in ("n4096", "n4097", "n4661")] == [False, True, True]
    c = C.case("m_lt_n")
    seg = c["ref"][0][0]["seg"]
    assert c["est_len"].tolist() == [300, 150] and ((seg["last"] >= 300) & (seg["last"] < 400)).any() and not seg["valid"][seg["last"] >= 300].any()


# ---- the header, compiled for the host ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    out = os.path.join(EMU_DIR, "_build")
    os.makedirs(out, exist_ok=True)
    lib = os.path.join(out, "libemu_trajectory.so")
    srcs = [os.path.join(EMU_DIR, "emu_trajectory.cpp"), os.path.join(CSRC, "trajectory_math.h"), os.path.join(CSRC, "odometry_math.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", f"-I{CSRC}", srcs[0], "-o", lib], check=True)
    return ctypes.CDLL(lib)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def emu_result(L, c):
    """what the kernels' per-item arithmetic gives, with the yardstick's sums and the yardstick's segment ends"""
    got = C.expected(c)
    for s, (ref, _, _) in enumerate(c["ref"]):
        m, n = int(c["est_len"][s]), int(c["gt_len"][s])
        al = ref["align"]
        rebased = K.rebase(c["est"][s, :m])
        est = np.ascontiguousarray(al["est"])
        if "sums" in al:
            q, rtc = al["sums"], np.zeros(13)
            L.emu_umeyama(_p(np.ascontiguousarray(q["mx"])), _p(np.ascontiguousarray(q["my"])), ctypes.c_double(q["sx"]),
                          _p(np.ascontiguousarray(q["C"].reshape(9))), int(c["mode"] != "6dof"), _p(rtc))
            got["rtc"][s] = rtc
            est = np.zeros((m, 12))
            L.emu_apply_sim(_p(np.ascontiguousarray(rebased)), m, _p(rtc), int(c["mode"] in ("7dof", "6dof")), _p(est))
            got["est"][s, :m] = est
        gt = np.ascontiguousarray(al["gt"])
        seg = ref["seg"]
        v = np.nonzero(seg["valid"])[0]
        k = len(v)
        rows, ca, an, tr = np.zeros((k, 5)), np.zeros(k), np.zeros(k), np.zeros(k)
        f, l = seg["first"][v].astype(np.int32), seg["last"][v].astype(np.int32)
        if k:
            L.emu_segment_rows(_p(np.ascontiguousarray(est[f])), _p(np.ascontiguousarray(est[l])), _p(np.ascontiguousarray(gt[f])),
                               _p(np.ascontiguousarray(gt[l])), _p(f), _p(l), _p(np.ascontiguousarray(seg["len"][v])), k, _p(rows), _p(ca),
                               _p(an), _p(tr))
            got["rows"][s].reshape(-1, 5)[v] = rows
        ca, an, tr, sq, st = (np.zeros(max(m, 1)) for _ in range(5))
        L.emu_frame_terms(_p(est), _p(gt), m, _p(ca), _p(an), _p(tr), _p(sq), _p(st))
        pairs = max(m - 1, 0)
        with np.errstate(all="ignore"):
            sm = got["summary"][s]
            sm[0] = 100.0 * (K.tsum(rows[:, 2], "seq") / k) if k else 0.0
            sm[1] = (K.tsum(rows[:, 1], "seq") / k) * 180.0 / np.pi * 100.0 if k else 0.0
            sm[2] = np.sqrt(K.tsum(sq[:m], "seq") / m) if m else np.nan
            sm[3] = K.tsum(tr[:pairs], "seq") / pairs if pairs else np.nan
            sm[4] = (K.tsum(an[:pairs], "seq") / pairs) * 180.0 / np.pi if pairs else np.nan
    return got


@pytest.mark.parametrize("name,mode", C.RUNS_OF_CASES)
def test_header_agrees_with_the_restatement_per_item(emu, name, mode):
    c = C.case(name, mode)
    print(C.report(f"{name} {mode}", C.check(c, emu_result(emu, c))))


@pytest.mark.parametrize("mode", K.MODES)
def test_header_agrees_with_the_restatement_on_the_golden_sequences(emu, mode):
    c = C.golden_case(mode)
    print(C.report(f"golden {mode}", C.check(c, emu_result(emu, c))))


def test_header_svd_reconstructs_and_is_orthogonal(emu):
    g = np.random.RandomState(5)
    for trial in range(50):
        A = g.randn(3, 3) * 10.0 ** g.uniform(-3, 3)
        if trial % 5 == 0:
            A[:, 2] = A[:, 0] * 1e-9 + A[:, 2] * 1e-12  # a tiny third singular value keeps its relative accuracy
        u, d, v = np.zeros(9), np.zeros(3), np.zeros(9)
        emu.emu_svd3(_p(np.ascontiguousarray(A.reshape(9))), _p(u), _p(d), _p(v))
        u, v = u.reshape(3, 3), v.reshape(3, 3)
        want = np.linalg.svd(A)[1]
        assert np.abs(u @ np.diag(d) @ v.T - A).max() <= 64 * K.U * np.abs(A).max()
        assert np.abs(u.T @ u - np.eye(3)).max() <= 64 * K.U and np.abs(v.T @ v - np.eye(3)).max() <= 64 * K.U
        assert (np.abs(np.sort(d)[::-1] - want) <= 64 * K.U * want[0]).all()  # what LAPACK itself promises


# ---- check() has teeth ---------------------------------------------------------------------------------------------------------
def test_check_accepts_both_orders_of_the_restatement():
    for name in ("n257", "ragged", "m_lt_n", "mirrored", "same_motion"):
        for mode in ("scale_7dof", "7dof"):
            c = C.case(name, mode)
            C.check(c, C.expected(c))
            print(C.report(f"{name} {mode} (tree sums, linalg inverse)", C.check(c, C.expected(c, which=1))))


def test_check_rejects_another_alignment_and_a_wrong_segment_end():
    c = C.case("n513")
    wrong = C.expected(C.case("n513", "scale"))
    with pytest.raises(AssertionError, match="times its bound"):
        C.check(c, wrong)
    got = C.expected(c)
    seg = c["ref"][0][0]["seg"]
    i = int(np.nonzero(seg["valid"])[0][3])
    e, g = c["ref"][0][0]["align"]["est"], c["ref"][0][0]["align"]["gt"]
    f, l = seg["first"][i], seg["last"][i] + 1  # one frame late, as `>=` instead of `>` would never be, but an off-by-one search is
    _, ang, t = K.rel_error(e[f:f + 1], e[l:l + 1], g[f:f + 1], g[l:l + 1], "closed")
    got["rows"][0].reshape(-1, 5)[i, 1:3] = [ang[0] / seg["len"][i], t[0] / seg["len"][i]]
    with pytest.raises(AssertionError, match="times its bound"):
        C.check(c, got)


def test_check_rejects_leaks_and_a_kept_segment_past_m():
    c = C.case("ragged")
    got = C.expected(c)
    got["est"][1, 120] = 0.0
    with pytest.raises(AssertionError, match="past its length"):
        C.check(c, got)
    c = C.case("m_lt_n")
    got = C.expected(c)
    seg = c["ref"][0][0]["seg"]
    i = int(np.nonzero((seg["last"] >= 300) & (seg["last"] < 400))[0][0])
    got["valid"][0].reshape(-1)[i] = 1
    with pytest.raises(AssertionError, match="scored pairs differ"):
        C.check(c, got)
    c = C.case("stationary_est")
    got = C.expected(c)
    got["summary"][0, 2] = 0.0  # a trapped division by sigma_x^2 = 0
    with pytest.raises(AssertionError, match="finite where the yardstick is not"):
        C.check(c, got)


# ---- the C ABI's refusals that need no launch ----------------------------------------------------------------------------------
def test_trajectory_align_argument_checks_without_launching(dfepe):
    L = dfepe._lib.lib()
    x = ctypes.c_void_p(256)  # a non-null address that is never dereferenced: every call below returns before a launch
    names = ("est", "gt", "est_out", "gt_out", "rtc")

    def call(S, n, mode=2, **kw):
        a = {k: x for k in names}
        a.update(kw)
        return L.dfepe_trajectory_align(None, a["est"], a["gt"], None, None, S, n, mode, a["est_out"], a["gt_out"], a["rtc"])

    assert call(0, 100) == 0 and call(0, 0) == 0 and call(0, 5, **{k: None for k in names}) == 0
    assert call(-1, 100) == -1 and call(4, -1) == -1 and call(4, 100, mode=5) == -1 and call(4, 100, mode=-1) == -1 and call(0, 100, mode=9) == -1
    for k in names:
        assert call(4, 100, **{k: None}) == -1
    assert call(4, 0, rtc=None) == -1
    assert call(1, 2 ** 31 // 12) == -3
    assert "dfepe_trajectory_align" in dfepe.EXPORTED_SYMBOLS and L.dfepe_version() == 154
    assert dfepe._lib.TRAJ_MODES == K.MODES


def test_kitti_odometry_errors_argument_checks_without_launching(dfepe):
    L = dfepe._lib.lib()
    x = ctypes.c_void_p(256)
    names = ("est", "gt", "dist", "rows", "valid", "count", "summary")

    def call(S, n, step=10, F=10, **kw):
        a = {k: x for k in names}
        a.update(kw)
        return L.dfepe_kitti_odometry_errors(None, a["est"], a["gt"], None, None, S, n, step, F, a["dist"], a["rows"], a["valid"], a["count"],
                                             a["summary"])

    assert call(0, 100) == 0 and call(0, 0, F=0) == 0 and call(0, 100, **{k: None for k in names}) == 0
    assert call(-1, 100) == -1 and call(2, -1) == -1 and call(2, 100, step=0) == -1 and call(2, 100, step=-3) == -1 and call(2, 100, F=-1) == -1
    for k in names:
        assert call(2, 100, **{k: None}) == -1
    assert call(2, 0, F=0, count=None) == -1 and call(2, 0, F=0, summary=None) == -1
    assert call(1, 2 ** 31 // 12) == -3 and call(1, 100, F=(2 ** 31 - 1) // 40 + 1) == -3
    assert call(2, 100, F=9) == -1 and call(2, 101, F=10) == -1 and call(2, 100, step=7, F=14) == -1  # rows for fewer first frames than there are
    assert "dfepe_kitti_odometry_errors" in dfepe.EXPORTED_SYMBOLS and L.dfepe_version() == 154


def test_ops_and_io_on_the_host(dfepe, golden, tmp_path):
    import torch
    ET = dfepe.compat.eval_tools
    with pytest.raises(dfepe.DfepeError):
        dfepe.ops.trajectory_align(torch.zeros(1, 4, 3, 4, dtype=torch.float64), torch.zeros(1, 4, 3, 4, dtype=torch.float64))
    with pytest.raises(dfepe.DfepeError):
        dfepe.ops.kitti_odometry_errors(torch.zeros(1, 4, 3, 4), torch.zeros(1, 4, 3, 4))
    # the writer reproduces the layout of the shipped files from the restatement's result; the reader reads a pose file back
    g = golden("kitti_odom")
    ref = K.evaluate(g["est_deepFEPE_10"], g["gt_10"])
    F = len(ref["seg"]["first"]) // 8
    res = dict(zip(("t_rel", "r_rel", "ATE", "RPE_trans", "RPE_rot"), ref["summary"]))
    res.update(segments=ref["seg"]["rows"].reshape(F, 8, 5), valid=ref["seg"]["valid"].reshape(F, 8))
    ET.write_kitti_result(str(tmp_path), "10", res)
    back = np.loadtxt(tmp_path / "errors" / "10.txt")
    assert back.shape == g["errors_deepFEPE_10"].shape and np.array_equal(back, ref["seg"]["rows"][ref["seg"]["valid"]])
    text = (tmp_path / "result.txt").read_text()
    assert text.splitlines()[0].split() == ["Sequence:", "10"] and "Trans. err. (%): \t 11.719 " in text and "RPE (deg): \t 0.212 " in text
    np.savetxt(tmp_path / "poses.txt", g["gt_10"].reshape(-1, 12)[:7])
    assert np.array_equal(ET.read_kitti_poses(str(tmp_path / "poses.txt")), g["gt_10"][:7])
