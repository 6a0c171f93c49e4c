"""dfepe_pose_chain and dfepe_snippet_errors on the device, held to the fp64 restatement of tests/odometry_ref.py through the one
check() of tests/odometry_cases.py (which tests/test_odometry_ref_cpu.py pins, and whose teeth it shows, without a GPU), and the
mirror compat.eval_tools against the reference's own output (tests/golden/odometry.npz).

Bounds (derived in tests/odometry_ref.py, none of them from what the kernels give).
  chain     per pose k: 4 x the distance between the restatement's sequential and tree orders on the same inputs, plus
            k 2^-52 max|entry_k|.  Seen on the CPU for the host build of the same header in the same association order (the
            device is expected to give the same bits: contraction is off in that code): n = 1591, rotations up to pi: 1.8e-13
            from sequential at a spread of 2.0e-13 and entries up to 63, 0.10 of the bound; n = 2048: 2.8e-13 at spread 4.4e-13,
            entries up to 98; the first 8 poses of every sequence bit-equal to the sequential loop.  On an MI355X: the same
            figures to every printed digit (n = 1591: 1.81e-13 at spread 1.99e-13; n = 2048: 2.84e-13 at 4.41e-13; n = 2049 with
            cam2body: 6.39e-13 at 9.95e-13, entries up to 123), worst ratio to the bound 0.26 (n = 512); snippet errors, scale and
            aligned 0.00 of their bounds (equal to the restatement), run-to-run bit-equal.
  snippets  errors: one float32 spacing of the value (+ 128 2^-53 on RE, the conditioning of atan2 at c ~ 2); scale and
            aligned: kappa 2^-52 relative, kappa = sum|est_t gt_t| / |sum est_t gt_t| < 1e3 asserted (seen <= 1.08); stats:
            the fp64 two-pass reduction over the same float32 errors within nw 2^-53 max|x| (mean) and 8 x that (std).
            Exactly-degenerate windows must show the reference's NaN / inf pattern; nothing else is exempt.
Every buffer holds a sentinel before the launch, so a row that must not be written is seen if it is."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import odometry_cases as C  # noqa: E402
import odometry_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return None if a is None else torch.tensor(np.asarray(a), device=DEV)  # a copy: the cases' arrays are read-only


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def run_chain(dfepe, case, with_lengths=True):
    rel, c2b = _dev(case["rel"]), _dev(case["cam2body"])
    S, n_max = case["rel"].shape[:2]
    ln = _dev(case["lengths"]) if with_lengths else None
    out = torch.full((S, n_max + 1, 12), C.SENTINEL, dtype=torch.float64, device=DEV)
    rc = dfepe._lib.lib().dfepe_pose_chain(_stream(), _ptr(rel) if n_max else None, _ptr(ln), _ptr(c2b), case["c2b_stride"], S, n_max,
                                           _ptr(out))
    assert rc == 0
    return out.cpu().numpy()


def run_snippets(dfepe, case):
    est, gt, wn = _dev(case["est"]), _dev(case["gt"]), _dev(case["windows"])
    S, m, W, L = est.shape[0], est.shape[1], case["W"], case["L"]
    f64 = dict(dtype=torch.float64, device=DEV)
    got = {"errors": torch.full((S, W, 2), C.SENTINEL, dtype=torch.float32, device=DEV), "scale": torch.full((S, W), C.SENTINEL, **f64),
           "aligned": torch.full((S, W, 12), C.SENTINEL, **f64), "compensated": torch.full((S, W, L, 12), C.SENTINEL, **f64),
           "stats": torch.full((S, 4), C.SENTINEL, **f64)}
    rc = dfepe._lib.lib().dfepe_snippet_errors(_stream(), _ptr(est), _ptr(gt), _ptr(wn), S, m, W, L, 0 if case["compensate"] else 1,
                                               _ptr(got["errors"]), _ptr(got["scale"]), _ptr(got["aligned"]), _ptr(got["compensated"]),
                                               _ptr(got["stats"]))
    assert rc == 0
    return {k: v.cpu().numpy() for k, v in got.items()}


@pytest.mark.parametrize("name", list(C.CHAIN_CASES))
def test_pose_chain(dfepe, name):
    case = C.chain_case(name)
    got = run_chain(dfepe, case)
    fig = C.check(case, got)
    print(f"{name}: {fig['max_diff']:.2e} from sequential (spread {fig['max_spread']:.2e}, entries up to {fig['max_entry']:.0f}), "
          f"worst ratio to the bound {fig['worst_ratio']:.2f}")
    for s, n in enumerate(case["lengths"]):  # a lane's own chunk from the identity is the sequential loop, bit for bit
        k = min(int(n), C.CHUNK) + 1
        assert np.array_equal(got[s, :k], case["seq"][s][:k])
    if len(case["lengths"]) == 1:  # lengths == NULL means n_max
        assert np.array_equal(run_chain(dfepe, case, with_lengths=False), got)


def test_pose_chain_is_bit_reproducible_and_clamps_lengths(dfepe):
    case = C.chain_case("ragged_c2b_pose")
    a, b = run_chain(dfepe, case), run_chain(dfepe, case)
    assert np.array_equal(a, b)
    wild = dict(case, lengths=np.array([-5, 65, 10 ** 6], np.int32))  # clamped to [0, n_max]: nothing outside the buffers
    got = run_chain(dfepe, wild)
    assert np.array_equal(got[0], a[0]) and np.array_equal(got[1], a[1]) and np.array_equal(got[2], a[2])


@pytest.mark.parametrize("name", list(C.SNIPPET_CASES))
def test_snippet_errors(dfepe, name):
    case = C.snippet_case(name)
    got = run_snippets(dfepe, case)
    fig = C.check(case, got)
    print(f"{name}: errors {fig['err_ratio']:.2f} of a float32 spacing, scale / aligned {fig['scale_ratio']:.2f} of kappa 2^-52 "
          f"(kappa <= {fig['kappa']:.4f}), stats {fig['stats_ratio']:.2f} of their bound, {fig['degenerate']} degenerate windows")
    assert np.array_equal(got["errors"], run_snippets(dfepe, case)["errors"], equal_nan=True)  # run to run, bit for bit
    if name == "L5_stationary_gt":
        assert fig["degenerate"] == 1 and np.isnan(got["stats"][0, 0]) and np.isnan(got["scale"][0, 10])
    if name == "L5":
        assert np.isnan(got["stats"][0]).all()  # the sequence without windows


def test_ops_layer(dfepe):
    case = C.chain_case("ragged_c2b_seq")
    S, n_max = case["rel"].shape[:2]
    out = torch.full((S, n_max + 1, 12), C.SENTINEL, dtype=torch.float64, device=DEV)
    a = dfepe.ops.pose_chain(_dev(case["rel"]).view(S, n_max, 3, 4), lengths=case["lengths"].tolist(),
                             cam2body=_dev(case["cam2body"]).view(S, 3, 4), out=out)
    assert a.shape == (S, n_max + 1, 3, 4) and a.dtype == torch.float64
    C.check(case, a.cpu().numpy().reshape(S, n_max + 1, 12))
    case = C.chain_case("ragged_c2b_pose")
    z = dfepe.ops.pose_chain(_dev(case["rel"]), lengths=_dev(case["lengths"]), cam2body=_dev(case["cam2body"]))
    C.check(case, _tail_to_sentinel(case, z.cpu().numpy().reshape(S, n_max + 1, 12)))  # without `out` the unwritten tail is zero
    with pytest.raises(ValueError):
        dfepe.ops.pose_chain(_dev(case["rel"]), lengths=[0, 65, 301])
    sc = C.snippet_case("L5")
    r = dfepe.ops.snippet_errors(_dev(sc["est"]), _dev(sc["gt"]), seq_length=5, windows=sc["windows"].tolist(), want_compensated=True)
    got = {"errors": r["errors"].cpu().numpy(), "scale": r["scale_factors"].cpu().numpy(),
           "aligned": r["aligned_poses"].cpu().numpy().reshape(5, -1, 12), "stats": r["stats"].cpu().numpy(),
           "compensated": r["compensated"].cpu().numpy().reshape(5, sc["W"], 5, 12)}
    for s, nw in enumerate(sc["windows"]):  # ops zero-fills what the kernel leaves alone; check() wants the sentinel there
        for k in ("errors", "scale", "aligned", "compensated"):
            assert not got[k][s, nw:].any()
            got[k][s, nw:] = C.SENTINEL
    C.check(sc, got)
    with pytest.raises(ValueError):
        dfepe.ops.snippet_errors(_dev(sc["est"]), _dev(sc["gt"]), seq_length=5, windows=[0, 1, 64, 65, C.SNIP_M - 4 + 1])
    with pytest.raises(dfepe.DfepeError):
        dfepe.ops.snippet_errors(_dev(sc["est"]), _dev(sc["gt"]), seq_length=65)


def _tail_to_sentinel(case, a):
    a = a.copy()
    for s, n in enumerate(case["lengths"]):
        assert not a[s, n + 1:].any()
        a[s, n + 1:] = C.SENTINEL
    return a


# ---- the mirror against the reference's own output -----------------------------------------------------------------------------
def _p44(a):
    out = np.tile(np.eye(4), (len(a), 1, 1))
    out[:, :3] = a
    return out


@pytest.mark.parametrize("s", [0, 1])
def test_compat_methods_against_the_golden_file(dfepe, golden, s, capsys):
    g = golden("odometry")
    P = dfepe.compat.eval_tools.Exp_table_processor
    body = g[f"rel_body_{s}"]
    got = P.get_abs_poses(list(_p44(body)))
    want = g[f"abs_{s}"]
    assert got.dtype == np.float64 and got.shape == want.shape
    # the kernel against the reference: the kernel's own bound (against the restatement) plus the restatement's against the file
    seq, tree = R.chain_sequential(body.reshape(-1, 12)), R.chain_tree(body.reshape(-1, 12))
    tol = R.chain_bound(seq, tree) + R.golden_chain_tol(want.reshape(-1, 12))
    assert (np.abs(got - want).reshape(len(want), 12).max(axis=1) <= tol).all()
    gt = g[f"gt_{s}"]
    for L in (5, 3):
        r = P.pose_seq_ate(want, gt, L)
        assert "Results" in capsys.readouterr().out
        e = r["errors"]
        assert isinstance(e, np.ndarray) and e.dtype == np.float32 and e.shape == (len(want) - L, 2)
        assert isinstance(r["scale_factors"], list) and isinstance(r["aligned_poses"], list) and len(r["scale_factors"]) == len(e)
        assert r["aligned_poses"][0].shape == (3, 4) and sorted(r) == ["aligned_poses", "errors", "scale_factors"]
        ref = R.snippet_errors(want.reshape(-1, 12), gt.astype(np.float64).reshape(-1, 12), len(e), L)
        assert (np.abs(e.astype(np.float64) - g[f"errors{L}_{s}"]) <= R.error_tol(g[f"errors{L}_{s}"])).all()
        stol = (R.golden_scale_tol(ref["kappa"], L) + R.scale_tol(ref["kappa"])) * np.abs(g[f"scale{L}_{s}"])
        assert (np.abs(np.array(r["scale_factors"]) - g[f"scale{L}_{s}"]) <= stol).all()
        if L == 5:
            assert (np.abs(np.stack(r["aligned_poses"]) - g[f"aligned5_{s}"]).reshape(len(e), 12)
                    <= (stol / np.abs(g[f"scale5_{s}"]))[:, None] * np.abs(g[f"aligned5_{s}"]).reshape(len(e), 12)).all()
    with pytest.raises(AssertionError):
        P.pose_seq_ate(want, gt[:-1], 5)
    ce, cg = P.compensate_poses(want[10:15]), P.compensate_poses(gt[10:15])
    assert ce.dtype == np.float64 and ce.shape == (5, 3, 4)
    assert np.abs(ce - g[f"comp_est_{s}"]).max() <= 16 * R.U * np.abs(g[f"comp_est_{s}"]).max()
    assert np.abs(cg - g[f"comp_gt_{s}"]).max() <= 16 * R.U * np.abs(g[f"comp_gt_{s}"]).max()
    if s == 0:  # longer than one snippet: 63 poses at a time behind the first
        long = P.compensate_poses(want[3:203])
        ref = R.snippet_errors(np.concatenate([want[3:4], want[130:193]]).reshape(-1, 12), want[:64].reshape(-1, 12), 1, 64)
        assert long.shape == (200, 3, 4) and np.array_equal(long[127:190].reshape(-1, 12), ref["compensated"][0][1:])  # third chunk
        assert np.array_equal(long[:5], P.compensate_poses(want[3:8]))
    cpe = P.compute_pose_error(g[f"comp_est_{s}"], g[f"comp_gt_{s}"])
    ate, re, scale = g[f"cpe_{s}"]
    assert sorted(cpe) == ["ATE", "RE", "scale_factor"] and isinstance(cpe["ATE"], np.float64)
    assert abs(cpe["ATE"] - ate) <= R.spacing32(ate) and abs(cpe["RE"] - re) <= R.spacing32(re) + R.RE_FLOOR
    k = R.snippet_errors(g[f"comp_est_{s}"].reshape(5, 12), g[f"comp_gt_{s}"].reshape(5, 12), 1, 5, compensated=False)["kappa"][0]
    assert abs(cpe["scale_factor"] - scale) <= (R.golden_scale_tol(k, 5) + R.scale_tol(k)) * abs(scale)


def _summary_inputs(golden):
    g = golden("odometry")
    n0, n1 = len(g["rel_cam_0"]), len(g["rel_cam_1"])
    rel = np.zeros((2, n0, 3, 4), np.float32)
    rel[0], rel[1, :n1] = g["rel_cam_0"], g["rel_cam_1"]
    c2b = np.stack([g["cam2body_0"], g["cam2body_1"]])
    gt = np.zeros((2, n0 + 1, 3, 4), np.float32)
    gt[0], gt[1, :n1 + 1] = g["gt_0"], g["gt_1"]
    return g, _dev(rel), _dev(c2b), _dev(gt), [n0, n1]


def _check_summary(g, out, s, n, L=5):
    """one sequence of an odometry_summary result against the golden file: trajectory, errors, scale, mean / std"""
    want = g[f"abs_{s}"].reshape(-1, 12)
    rel, c = g[f"rel_cam_{s}"].astype(np.float64).reshape(-1, 12), g[f"cam2body_{s}"].astype(np.float64).reshape(12)
    tol = R.chain_bound(R.chain_sequential(rel, c), R.chain_tree(rel, c)) + R.golden_chain_tol(want)
    got = out["abs_poses"].cpu().numpy().reshape(-1, 12)[:n + 1]
    assert (np.abs(got - want).max(axis=1) <= tol).all()
    nw = n + 1 - L
    e = out["errors"].cpu().numpy()[:nw]
    # the estimate scored here differs from the file's by the chain's rounding, at most tol.max() per entry: the errors and the
    # scale may move by what odometry_ref.perturbed_input_tol says on top of their own bounds
    ref = R.snippet_errors(want, g[f"gt_{s}"].astype(np.float64).reshape(-1, 12), nw, L)
    pert = R.perturbed_input_tol(tol.max(), L)
    assert e.dtype == np.float32 and (np.abs(e.astype(np.float64) - g[f"errors{L}_{s}"]) <= R.error_tol(g[f"errors{L}_{s}"]) + pert / L).all()
    stol = (R.golden_scale_tol(ref["kappa"], L) + R.scale_tol(ref["kappa"])) * np.abs(g[f"scale{L}_{s}"]) + pert / np.sqrt(ref["den"])
    assert (np.abs(out["scale_factors"].cpu().numpy()[:nw] - g[f"scale{L}_{s}"]) <= stol).all()
    assert not out["errors"].cpu().numpy()[nw:].any()
    st = np.array([out[k].item() for k in ("ATE_mean", "ATE_std", "RE_mean", "RE_std")])
    want_st = R.stats(e)
    assert (np.abs(st - want_st) <= R.stats_tol(e)).all()


def test_odometry_summary_single_and_batched(dfepe, golden):
    g, rel, c2b, gt, lengths = _summary_inputs(golden)
    ET = dfepe.compat.eval_tools
    one = ET.odometry_summary(rel[0], c2b[0], gt[0])
    assert one["abs_poses"].shape == (301, 3, 4) and one["errors"].shape == (296, 2) and one["ATE_mean"].dim() == 0
    assert one["abs_poses"].is_cuda and one["errors"].dtype == torch.float32
    _check_summary(g, one, 0, 300)
    per_pose = ET.odometry_summary(rel[0], _dev(_p44(g["cam2body_0"][None]).astype(np.float32)).expand(300, 4, 4), gt[0])
    assert all(torch.equal(one[k], per_pose[k]) or (torch.isnan(one[k]).all() and torch.isnan(per_pose[k]).all()) for k in one)
    for ln in (lengths, _dev(np.array(lengths, np.int32))):  # host values and a device tensor
        both = ET.odometry_summary(rel, c2b, gt, lengths=ln)
        assert both["errors"].shape == (2, 296, 2) and both["ATE_mean"].shape == (2,)
        for s, n in enumerate(lengths):
            _check_summary(g, {k: v[s] for k, v in both.items()}, s, n)
        assert torch.equal(both["abs_poses"][0], one["abs_poses"]) and torch.equal(both["errors"][0], one["errors"])


def test_odometry_summary_under_graph_capture_replays_bit_equal(dfepe, golden):
    g, rel, c2b, gt, lengths = _summary_inputs(golden)
    ET = dfepe.compat.eval_tools
    ln = _dev(np.array(lengths, np.int32))
    eager = ET.odometry_summary(rel, c2b, gt, lengths=ln)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = ET.odometry_summary(rel, c2b, gt, lengths=ln)
    graph.replay()
    torch.cuda.synchronize()
    for k, v in eager.items():
        a, b = v.cpu().numpy(), captured[k].cpu().numpy()
        assert np.array_equal(a, b, equal_nan=True), k
    _check_summary(g, {k: v[1] for k, v in captured.items()}, 1, lengths[1])
