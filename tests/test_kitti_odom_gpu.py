"""dfepe_trajectory_align and dfepe_kitti_odometry_errors on the device, held to the fp64 restatement of tests/kitti_odom_ref.py
through the one check() of tests/kitti_odom_cases.py (which tests/test_kitti_odom_ref_cpu.py pins, and whose teeth it shows,
without a GPU), through the C ABI with sentinel-filled buffers, through ops and through compat.eval_tools; and the five numbers
against the ones the reference publishes (tests/golden/kitti_odom.npz).

Bounds (derived in tests/kitti_odom_ref.py, none of them from what the kernels give): every continuous value within 4 x the
distance between the restatement's two evaluation orders (sequential sums and closed-form inverses against tree sums and
numpy.linalg.inv) plus (frames + 64) 2^-52 max|entry|; angles through arccos' own conditioning; segment ends exact, with no
undecided pair in any input; NaN padding must not leak; what a sequence does not own keeps its sentinel.  Every test prints the
achieved fractions of the bounds.

Seen on an MI355X (98 tests, 4.5 s): every scored pair and count equal to the restatement's; worst fraction of a bound 0.28 (alignment
and aligned poses of the ragged batch in 7dof), segment errors <= 0.07, the five numbers 0.00; the shipped trajectories <= 0.01
throughout, their five numbers equal to the restatement's to every printed digit; two runs and a graph replay bit-equal."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kitti_odom_cases as C  # noqa: E402
import kitti_odom_ref as K  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.tensor(np.asarray(a), device=DEV)  # a copy: the cases' arrays are read-only


def _ptr(t):
    return None if t is None or t.numel() == 0 else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def run(dfepe, c, with_lengths=True):
    """both launches through the C ABI, every output buffer pre-filled with the sentinel"""
    L = dfepe._lib.lib()
    est, gt = _dev(c["est"]), _dev(c["gt"])
    el, gl = (_dev(c["est_len"]), _dev(c["gt_len"])) if with_lengths else (None, None)
    S, n_max = est.shape[:2]
    buf = {k: _dev(v) for k, v in C.blank(c).items()}
    rc = L.dfepe_trajectory_align(_stream(), _ptr(est), _ptr(gt), _ptr(el), _ptr(gl), S, n_max, K.MODES.index(c["mode"]),
                                  _ptr(buf["est"]), _ptr(buf["gt"]), _ptr(buf["rtc"]))
    assert rc == 0
    rc = L.dfepe_kitti_odometry_errors(_stream(), _ptr(buf["est"]), _ptr(buf["gt"]), _ptr(el), _ptr(gl), S, n_max, c["step"], c["F"],
                                       _ptr(buf["dist"]), _ptr(buf["rows"]), _ptr(buf["valid"]), _ptr(buf["count"]), _ptr(buf["summary"]))
    assert rc == 0
    return {k: v.cpu().numpy() for k, v in buf.items()}


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


@pytest.mark.parametrize("mode", K.MODES)
def test_golden_trajectories(dfepe, mode):
    c = C.golden_case(mode)
    got = run(dfepe, c)
    print(C.report(f"golden {mode}", C.check(c, got)))
    assert same_bits(got, run(dfepe, c))  # run to run, bit for bit
    if mode == "scale_7dof":
        z = np.load(C.GOLDEN, allow_pickle=False)
        for s, (r, q) in enumerate(c["keys"]):
            print(f"{r} {q}: {got['summary'][s]} against the published {z[f'result_{r}_{q}']}")
            C.assert_published(got["summary"][s], z[f"result_{r}_{q}"], r, q)
            assert int(got["count"][s]) == len(z[f"errors_{r}_{q}"])


@pytest.mark.parametrize("name,mode", C.RUNS_OF_CASES)
def test_synthetic_trajectories(dfepe, name, mode):
    c = C.case(name, mode)
    got = run(dfepe, c)
    print(C.report(f"{name} {mode}", C.check(c, got)))
    assert same_bits(got, run(dfepe, c))
    if len(c["gt_len"]) == 1 and c["est_len"][0] == c["gt_len"][0]:  # lengths == NULL means n_max
        assert same_bits(got, run(dfepe, c, with_lengths=False))
    if name == "stationary_est" and mode == "scale_7dof":
        assert not np.isfinite(got["rtc"][0, 12]) and not np.isfinite(got["summary"][0, 2:4]).any() and not np.isfinite(got["est"][0, :, 3]).any()
    if name in ("n1", "short_of_100m"):
        assert got["count"][0] == 0 and got["summary"][0, 0] == 0.0 and got["summary"][0, 1] == 0.0
    if name == "n1":
        assert np.isnan(got["summary"][0, 3:]).all()
    if name == "past_100m":
        assert got["count"][0] == 1 and got["valid"][0, 0, 0] == 1
    if name == "same_motion" and mode == "none":
        assert np.isfinite(got["summary"]).all() and got["summary"][0, 2] == 0.0


def test_lengths_are_clamped_to_the_buffers(dfepe):
    c = C.case("ragged")
    want = run(dfepe, c)
    wild = dict(c, est_len=np.array([10 ** 6, 120, 257], np.int32), gt_len=np.array([513, 120, 257], np.int32))
    assert same_bits(want, run(dfepe, wild))  # est_len is clamped to gt_len, gt_len to n_max
    none = dict(c, est_len=np.array([-5, 0, 0], np.int32), gt_len=np.array([-1, 0, 0], np.int32))
    got = run(dfepe, none)
    assert np.all(got["est"] == C.SENTINEL) and np.all(got["rows"] == C.SENTINEL) and not got["count"].any()
    assert np.isnan(got["summary"][:, 2:]).all() and not got["summary"][:, :2].any()


def _from_ops(c, al, r):
    """ops results in check()'s layout: ops zero-fills what the kernels leave alone; check() wants the sentinel there"""
    S, n_max, F = c["est"].shape[0], c["est"].shape[1], c["F"]
    got = {"est": al["est"].cpu().numpy().reshape(S, n_max, 12).copy(), "gt": al["gt"].cpu().numpy().reshape(S, n_max, 12).copy(),
           "rtc": torch.cat([al["r"].reshape(S, 9), al["t"], al["c"][:, None]], dim=1).cpu().numpy(), "dist": r["dist"].cpu().numpy().copy(),
           "rows": r["rows"].cpu().numpy().copy(), "valid": r["valid"].cpu().numpy().astype(np.uint8), "count": r["count"].cpu().numpy(),
           "summary": r["summary"].cpu().numpy()}
    assert r["valid"].dtype == torch.bool and got["rows"].shape == (S, F, 8, 5) and r["count"].dtype == torch.int32
    for s in range(S):
        m, n = int(c["est_len"][s]), int(c["gt_len"][s])
        k = -(-n // c["step"])
        assert not got["est"][s, m:].any() and not got["gt"][s, n:].any() and not got["dist"][s, n:].any() and not got["rows"][s, k:].any()
        got["est"][s, m:], got["gt"][s, n:], got["dist"][s, n:], got["rows"][s, k:], got["valid"][s, k:] = (C.SENTINEL,) * 4 + (7,)
    return got


def test_ops_layer(dfepe):
    for name, mode in (("ragged", "7dof"), ("m_lt_n", "scale_7dof"), ("n513_step7", "scale")):
        c = C.case(name, mode)
        est, gt = _dev(c["est"]).view(*c["est"].shape[:2], 3, 4), _dev(c["gt"])
        lens = dict(est_lengths=c["est_len"].tolist(), gt_lengths=_dev(c["gt_len"]))  # host values and a device tensor
        al = dfepe.ops.trajectory_align(est, gt, mode, **lens)
        r = dfepe.ops.kitti_odometry_errors(al["est"], al["gt"], step=c["step"], **lens)
        assert al["est"].shape == (*c["est"].shape[:2], 3, 4) and al["r"].shape == (len(c["est"]), 3, 3) and al["c"].dtype == torch.float64
        print(C.report(f"ops {name} {mode}", C.check(c, _from_ops(c, al, r))))
    c = C.case("m_lt_n")  # an estimate with fewer frames than the ground truth, unpadded
    short = dfepe.ops.trajectory_align(_dev(c["est"][:1, :300]), _dev(c["gt"][:1]), "scale_7dof")
    full = dfepe.ops.trajectory_align(_dev(c["est"][:1]), _dev(c["gt"][:1]), "scale_7dof", est_lengths=[300])
    assert torch.equal(short["est"], full["est"]) and torch.equal(short["c"], full["c"])
    with pytest.raises(ValueError):
        dfepe.ops.trajectory_align(_dev(c["est"]), _dev(c["gt"]), "8dof")
    with pytest.raises(ValueError):
        dfepe.ops.trajectory_align(_dev(c["est"]), _dev(c["gt"]), est_lengths=[300, 401])
    with pytest.raises(ValueError):
        dfepe.ops.kitti_odometry_errors(_dev(c["est"]), _dev(c["gt"]), step=0)
    with pytest.raises(ValueError):
        dfepe.ops.trajectory_align(_dev(c["gt"]), _dev(c["est"][:, :300]))  # more estimated frames than ground truth


def test_compat_eval_on_host_arrays_and_device_tensors(dfepe, tmp_path):
    ET = dfepe.compat.eval_tools
    z = np.load(C.GOLDEN, allow_pickle=False)
    c = C.golden_case()
    res = ET.kitti_odometry_eval(z["est_deepF_10"], z["gt_10"])  # numpy in, numpy and python scalars out
    assert isinstance(res["t_rel"], float) and isinstance(res["count"], int) and isinstance(res["segments"], np.ndarray)
    ref, _, b = c["ref"][3]
    five = np.array([res[k] for k in ("t_rel", "r_rel", "ATE", "RPE_trans", "RPE_rot")])
    assert (np.abs(five - ref["summary"]) <= b["summary"]).all() and res["count"] == 464
    C.assert_published(five, z["result_deepF_10"], "deepF", "10")
    ET.write_kitti_result(str(tmp_path), 10, res)
    rows = np.loadtxt(tmp_path / "errors" / "10.txt")
    assert rows.shape == (464, 5) and np.array_equal(rows[:, 0], z["errors_deepF_10"][:, 0])
    assert "ATE (m): \t 34.342 " in (tmp_path / "result.txt").read_text()
    dev = ET.kitti_odometry_eval(_dev(c["est"]).view(4, -1, 3, 4), _dev(c["gt"]).view(4, -1, 3, 4), lengths=(_dev(c["est_len"]), _dev(c["gt_len"])))
    assert dev["summary"].is_cuda and dev["summary"].shape == (4, 5) and dev["segments"].shape == (4, 160, 8, 5)
    assert np.array_equal(dev["summary"][3].cpu().numpy(), five)  # the batch and the single sequence: the same bits
    for mode in K.MODES:
        one = ET.kitti_odometry_eval(z["est_deepFEPE_09"], z["gt_09"], alignment=mode)
        ref, _, b = C.golden_case(mode)["ref"][0]
        assert (np.abs(one["summary"] - ref["summary"]) <= b["summary"]).all() and one["count"] == ref["count"]


def test_compat_eval_of_a_shorter_estimate_without_lengths(dfepe):
    """est [m,3,4] against gt [n,3,4], m < n, no lengths: the documented single-sequence call.  Both launches must take m from
    the estimate's shape: segments ending at or past m are dropped, ATE and RPE run over m frames, nothing is scored on padding."""
    ET = dfepe.compat.eval_tools
    for mode in K.MODES:
        c = C.case("m_lt_n", mode)
        ref, _, b = c["ref"][0]
        est, gt = c["est"][0, :300].reshape(300, 3, 4), c["gt"][0].reshape(400, 3, 4)
        for res in (ET.kitti_odometry_eval(est, gt, alignment=mode), ET.kitti_odometry_eval(_dev(est), _dev(gt), alignment=mode)):
            res = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in res.items()}
            frac = np.abs(res["summary"] - ref["summary"]) / b["summary"]
            print(f"m < n, {mode}: summary {res['summary']} at {frac.max():.2f} of its bound, {int(res['count'])} segments")
            assert (frac <= 1.0).all() and int(res["count"]) == ref["count"]
            assert np.array_equal(res["valid"].reshape(-1), ref["seg"]["valid"]) and res["segments"].shape == (40, 8, 5)
            assert (np.abs(res["aligned_poses"].reshape(400, 12)[:300] - ref["align"]["est"]) <= b["est"]).all()
            assert not res["aligned_poses"][300:].any() and abs(res["scale"] - ref["align"]["c"]) <= b["rtc"][12]


def _table_inputs(golden):
    """the odometry golden file's two sequences of camera motions (300 and 37 relative poses), as odometry_summary's tests use"""
    g = golden("odometry")
    n0, n1 = len(g["rel_cam_0"]), len(g["rel_cam_1"])
    rel = np.zeros((2, n0, 3, 4), np.float32)
    rel[0], rel[1, :n1] = g["rel_cam_0"], g["rel_cam_1"]
    c2b = np.stack([g["cam2body_0"], g["cam2body_1"]])
    gt = np.full((2, n0 + 1, 3, 4), np.nan, np.float32)
    gt[0], gt[1, :n1 + 1] = g["gt_0"], g["gt_1"]
    return g, _dev(rel), _dev(c2b), _dev(gt), [n0, n1]


def _check_table(g, out, s, n, mode):
    """one sequence of an odometry_table result: the table of the trajectory the chain kernel produced, against the restatement on
    that same trajectory"""
    est = out["abs_poses"].cpu().numpy().reshape(-1, 12)[:n + 1]
    ref, alt, b = K.reference(est, g[f"gt_{s}"].astype(np.float64).reshape(-1, 12), mode, 10)
    assert len(K.undecided(ref["seg"])) == 0
    got = out["summary"].cpu().numpy()
    assert (np.abs(got - ref["summary"]) <= b["summary"]).all() and int(out["count"].item()) == ref["count"]
    k = len(ref["seg"]["first"])
    assert np.array_equal(out["valid"].cpu().numpy().reshape(-1)[:k], ref["seg"]["valid"])
    return float((np.abs(got - ref["summary"]) / np.maximum(b["summary"], 1e-300)).max())


def test_odometry_table_single_and_batched(dfepe, golden):
    g, rel, c2b, gt, lengths = _table_inputs(golden)
    ET = dfepe.compat.eval_tools
    one = ET.odometry_table(rel[0], c2b[0], gt[0])
    assert one["abs_poses"].shape == (301, 3, 4) and one["summary"].shape == (5,) and one["segments"].shape == (31, 8, 5) and one["t_rel"].dim() == 0
    print(f"odometry_table: summary at {_check_table(g, one, 0, 300, 'scale_7dof'):.2f} of its bound, {int(one['count'])} segments")
    assert int(one["count"]) > 0
    for ln in (lengths, _dev(np.array(lengths, np.int32))):  # host values and a device tensor
        both = ET.odometry_table(rel, c2b, gt, alignment="7dof", lengths=ln)
        assert both["summary"].shape == (2, 5) and both["count"].shape == (2,)
        for s, n in enumerate(lengths):
            _check_table(g, {k: v[s] for k, v in both.items()}, s, n, "7dof")
    assert torch.equal(ET.odometry_table(rel, c2b, gt, lengths=lengths)["summary"][0], one["summary"])
    part = ET.odometry_table(rel[0, :200], c2b[0], gt[0])  # a chain of 201 poses against 301 ground-truth frames, no lengths
    assert part["abs_poses"].shape == (201, 3, 4) and part["segments"].shape == (31, 8, 5)
    print(f"odometry_table, m < n: summary at {_check_table(g, part, 0, 200, 'scale_7dof'):.2f} of its bound, {int(part['count'])} segments")


def test_odometry_table_under_graph_capture_replays_bit_equal(dfepe, golden):
    g, rel, c2b, gt, lengths = _table_inputs(golden)
    ET = dfepe.compat.eval_tools
    ln = _dev(np.array(lengths, np.int32))
    eager = ET.odometry_table(rel, c2b, gt, lengths=ln)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = ET.odometry_table(rel, c2b, gt, lengths=ln)
    graph.replay()
    torch.cuda.synchronize()
    for k, v in eager.items():
        a, b = v.cpu().numpy(), captured[k].cpu().numpy()
        assert np.array_equal(a, b, equal_nan=True), k
    _check_table(g, {k: v[1] for k, v in captured.items()}, 1, lengths[1], "scale_7dof")
