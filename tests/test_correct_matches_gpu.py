"""dfepe_correct_matches on the device (ops.correct_matches and the virtual-point generator of compat.utils_misc) against the
fp64 restatement in tests/correct_matches_ref.py, which tests/test_correct_matches_cpu.py pins without a GPU.

Bounds.  The kernel computes in fp64 and writes float32.
  positions  |delta| <= 2^-13 px (1.22e-4): the float32 spacing at 1024-2048 px, i.e. half a spacing of output rounding plus fp64
             noise far below it; every reference coordinate is asserted to be below 2048 in magnitude.
  cost       the fp64 value is held to the CPU test's bound, 1e-9 relative with a floor of 1e-12 px^2; what the device returns is
             that value rounded to float32, so the returned cost must lie between the float32 roundings of the two ends of that
             interval (rounding is monotonic: this is the same bound seen through the output format, no wider).
A point whose two lowest candidate costs in the restatement are within 1e-6 relative may be left out of the position comparison
(at most 1 % of a test's points; there is none on these inputs), never of the cost comparison."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import correct_matches_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IM_SHAPE = (376, 1241)
POS_TOL = 2.0 ** -13
SHAPES = [(1, 1), (1, 100), (3, 100), (8, 100), (5, 37)]  # 300 lanes: a partial wavefront and a partial workgroup
SETS = ["grid", "grid_vs_matches"]


@pytest.fixture(scope="module")
def data(dfepe):
    """The inputs (float32 points, fp64 F) and the restatement's answers, computed once and left unchanged."""
    sc = dfepe.synth.make_scene(8, 100, seed=3, dtype=torch.float64)
    F = sc["F_gt"].numpy()
    m = sc["matches_xy_ori"].numpy().astype(np.float32)
    g = np.ascontiguousarray(np.broadcast_to(ref.grid(IM_SHAPE)[0], (8, 100, 2)))
    sets = {"grid": (g, g), "grid_vs_matches": (g, np.ascontiguousarray(m[:, :, 2:]))}
    d = {"F": F, "sets": sets, "ref": {}, "Ks": sc["Ks"].numpy()}
    for name, (P, Q) in sets.items():
        d["ref"][name] = [ref.correct_matches(F[b], P[b], Q[b]) for b in range(8)]
    d["ref"]["shared"] = [ref.correct_matches(F[0], g[b], sets["grid_vs_matches"][1][b]) for b in range(4)]
    d["virt"] = (sc["pts1_virt_ori"].numpy()[:, :, :2].astype(np.float32), sc["pts2_virt_ori"].numpy()[:, :, :2].astype(np.float32))
    return d


def run(dfepe, F, P, Q):
    new1, new2, cost = dfepe.ops.correct_matches(torch.as_tensor(F, device=DEV), torch.as_tensor(P, device=DEV),
                                                 torch.as_tensor(Q, device=DEV), want_cost=True)
    assert new1.dtype == new2.dtype == cost.dtype == torch.float32 and new1.device == torch.device(DEV)
    assert new1.shape == new2.shape == tuple(P.shape) and cost.shape == tuple(P.shape[:2])
    return new1.cpu().numpy(), new2.cpu().numpy(), cost.cpu().numpy()


def check(got, R, M):
    """got: the device's (new1, new2, cost) for some pairs; R: the restatement's dicts of those pairs; the first M points."""
    new1, new2, cost = got
    ties = n = 0
    for b, r in enumerate(R):
        p, q, c, tie = r["p"][:M], r["q"][:M], r["cost"][:M], r["near_tie"][:M]
        assert np.abs(p).max() < 2048 and np.abs(q).max() < 2048  # so that 2^-13 px is a float32 spacing or more
        lo = np.float32(c * (1 - 1e-9) - 1e-12)
        hi = np.float32(c * (1 + 1e-9) + 1e-12)
        print(f"pair {b}: cost off by {np.abs(cost[b].astype(np.float64) - c).max():.2e} px^2 (max cost {c.max():.3g}), "
              f"position off by {max(np.abs(new1[b] - p).max(), np.abs(new2[b] - q).max()):.2e} px")
        assert ((cost[b] >= lo) & (cost[b] <= hi)).all()
        keep = ~tie
        ties += int(tie.sum())
        n += len(tie)
        assert np.abs(new1[b][keep] - p[keep]).max(initial=0.0) <= POS_TOL
        assert np.abs(new2[b][keep] - q[keep]).max(initial=0.0) <= POS_TOL
    assert ties <= 0.01 * n


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("B,M", SHAPES)
def test_parity_with_the_restatement(dfepe, data, B, M, name):
    P, Q = data["sets"][name]
    got = run(dfepe, data["F"][:B], np.ascontiguousarray(P[:B, :M]), np.ascontiguousarray(Q[:B, :M]))
    check(got, data["ref"][name][:B], M)


def test_one_shared_F_for_all_pairs(dfepe, data):
    P, Q = data["sets"]["grid_vs_matches"]
    got = run(dfepe, data["F"][0], P[:4], Q[:4])  # F [3,3]
    check(got, data["ref"]["shared"], 100)
    again = run(dfepe, np.ascontiguousarray(np.broadcast_to(data["F"][0], (4, 3, 3))), P[:4], Q[:4])
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
    new1, _ = dfepe.ops.correct_matches(torch.as_tensor(data["F"][0], device=DEV), torch.as_tensor(P[:4], device=DEV),
                                        torch.as_tensor(Q[:4], device=DEV))  # want_cost=False: two outputs, same numbers
    assert np.array_equal(new1.cpu().numpy(), got[0])


@pytest.mark.parametrize("B,M", [(0, 100), (4, 0)])
def test_empty_batches_return_empty_tensors(dfepe, B, M):
    z = torch.zeros(B, M, 2, device=DEV)
    new1, new2, cost = dfepe.ops.correct_matches(torch.eye(3, device=DEV).expand(B, 3, 3), z, z, want_cost=True)
    assert new1.shape == new2.shape == (B, M, 2) and cost.shape == (B, M)


def test_points_already_on_the_geometry_stay(dfepe, data):
    """The scene's own virtual points rounded to float32 are within a rounding of the geometry: the correction returns them to
    2^-13 px with a cost of at most 1e-6 px^2."""
    p, q = data["virt"]
    new1, new2, cost = run(dfepe, data["F"], p, q)
    print(f"moved by {max(np.abs(new1 - p).max(), np.abs(new2 - q).max()):.2e} px, cost at most {cost.max():.2e} px^2")
    assert np.abs(new1 - p).max() <= POS_TOL and np.abs(new2 - q).max() <= POS_TOL
    assert cost.max() <= 1e-6 and cost.min() >= 0.0


def degenerate_case():
    e = np.array([512.0, 128.0, 1.0])
    F = np.array([[0, -e[2], e[1]], [e[2], 0, -e[0]], [-e[1], e[0], 0]])
    g = ref.grid(IM_SHAPE)[0].copy()
    g[37] = (512, 128)  # on the epipole in both images
    return F, g


def test_a_point_on_the_epipole_is_nan_and_the_other_lanes_are_unaffected(dfepe):
    F, g = degenerate_case()
    new1, new2, cost = run(dfepe, F[None], g[None], g[None])
    assert np.isnan(new1[0, 37]).all() and np.isnan(new2[0, 37]).all() and np.isnan(cost[0, 37])
    rest = np.arange(100) != 37
    r = ref.correct_matches(F, g[rest], g[rest])
    assert np.abs(new1[0, rest] - r["p"]).max() <= POS_TOL and np.abs(new2[0, rest] - r["q"]).max() <= POS_TOL
    # the same pair without the degenerate point: the 99 others get, bit for bit, what they got beside it
    alone = run(dfepe, F[None], g[rest][None], g[rest][None])
    assert np.array_equal(alone[0][0], new1[0, rest]) and np.array_equal(alone[1][0], new2[0, rest])
    # the compat functions map the NaN to 0 (utils_misc.py:177-178)
    um = dfepe.compat.utils_misc
    K = np.array([[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1.0]])
    for out in (um.get_virt_x1x2_np(IM_SHAPE, F, K, g, g), um.get_virt_x1x2(IM_SHAPE, F, K, g, g)):
        p1n, p2n, p1, p2 = (np.asarray(x) for x in out)
        assert np.array_equal(p1[37], [0, 0, 1]) and np.array_equal(p2[37], [0, 0, 1]) and np.isfinite(p1n).all()
        assert np.array_equal(p1[rest, :2], new1[0, rest]) and np.array_equal(p2[rest, :2], new2[0, rest])


def test_compat_functions_follow_the_references_lines(dfepe, data):
    """get_virt_x1x2_np / get_virt_x1x2 / get_virt_x1x2_batch against the restatement pushed through utils_misc.py:173-199: the
    swapped arguments of the correctMatches call (visible with different points in the two images), homogeneous output, inv(K),
    pts2_virt_normalized made from pts1_virt; shapes, dtypes, devices."""
    um = dfepe.compat.utils_misc
    g1, g2 = um.get_virt_x1x2_grid(IM_SHAPE)
    other = data["sets"]["grid_vs_matches"][1]
    for b in (0, 5):
        F, K = data["F"][b], data["Ks"][b]
        norm_tol = POS_TOL * np.abs(np.linalg.inv(K)).sum(1).max()  # a pixel error of 2^-13 through inv(K)
        for pts1_b, pts2_b in ((g1, g2), (g1, other[b])):
            want = ref.virt_through_the_reference_lines(F, K, pts1_b, pts2_b)
            got = um.get_virt_x1x2_np(IM_SHAPE, F, K, pts1_b, pts2_b)
            assert [x.dtype for x in got] == [np.float64, np.float64, np.float32, np.float32]
            assert all(x.shape == (100, 3) for x in got)
            assert np.abs(got[2] - want[2]).max() <= POS_TOL and np.abs(got[3] - want[3]).max() <= POS_TOL
            assert np.abs(got[0] - want[0]).max() <= norm_tol
            assert np.array_equal(got[0], got[1])                                            # :198
            assert np.array_equal(got[0], (np.linalg.inv(K) @ got[2].T).T)
            assert (got[2][:, 2] == 1).all() and (got[3][:, 2] == 1).all()
            if pts2_b is not g2:  # :176 -- pts1_virt started from pts2_virt_b: it is near those points, not near the grid
                assert np.abs(got[2][:, :2] - pts2_b).max() < np.abs(got[2][:, :2] - pts1_b).max()
            t = um.get_virt_x1x2(IM_SHAPE, F, K, pts1_b, pts2_b)
            assert all(isinstance(x, torch.Tensor) and x.dtype == torch.float32 and x.device.type == "cpu" for x in t)
            assert all(np.array_equal(x.numpy(), np.float32(y)) for x, y in zip(t, got))
        t = um.get_virt_x1x2(IM_SHAPE, F, K)  # the grid by default
        assert np.array_equal(t[2].numpy(), um.get_virt_x1x2_np(IM_SHAPE, F, K, g1, g2)[2])
    Fd, Kd = torch.as_tensor(data["F"], device=DEV), torch.as_tensor(data["Ks"], device=DEV)
    out = um.get_virt_x1x2_batch(IM_SHAPE, Fd, Kd)
    assert all(x.shape == (8, 100, 3) and x.dtype == torch.float32 and x.device == torch.device(DEV) for x in out)
    assert torch.equal(out[0], out[1]) and out[0].data_ptr() != out[1].data_ptr()
    key = (torch.device(DEV), IM_SHAPE)
    cached = um._virt_grids[key]
    um.get_virt_x1x2_batch([376, 1241, 3], Fd[:2], Kd[:2])
    assert um._virt_grids[key] is cached  # one grid per (device, image shape)
    for b in (0, 5):
        one = um.get_virt_x1x2(IM_SHAPE, data["F"][b], data["Ks"][b])
        assert np.array_equal(out[2][b].cpu().numpy(), one[2].numpy()) and np.array_equal(out[3][b].cpu().numpy(), one[3].numpy())
        # inv(K) by cofactors on the device against numpy's: float32 roundings of two fp64 values that agree to ~1e-16
        np.testing.assert_allclose(out[0][b].cpu().numpy(), one[0].numpy(), rtol=2.0 ** -22, atol=2.0 ** -24)


def test_end_to_end_the_f_loss_of_the_ground_truth_is_at_the_float32_floor(dfepe):
    """The reference's comment on get_virt_x1x2: "SHOULD BE ALL ZEROS: compute_epi_residual(pts1_virt_ori, pts2_virt_ori, F_gts)".
    The virtual points of get_virt_x1x2_batch under the F_gt they were made for, through the float32 residual kernel and through
    get_all_loss_DeepF with F_gt as every layer's estimate.

    The bound is 1e-4 unless the floor of exactly consistent points is higher, and then 4 x that floor; the floor is what the same
    kernel returns for the restatement's points rounded to float32 (no code of the correction involved).  It IS higher: rounding
    a corrected point to float32 moves it by up to 2^-14 px, and a grid point at distance r from its epipole turns its epipolar
    line by that over r, which a partner at distance R from the other epipole sees as R / r times as much -- KITTI-like forward
    motion puts the epipoles inside the image.  The same residual of those points evaluated on the host with numpy: at most 7.9e-4
    in fp64 and 1.1e-3 in float32 arithmetic, 2e-5 to 7e-5 on average over a pair; the test prints the kernel's own figures."""
    sc = dfepe.synth.make_scene(4, 100)
    F, K = sc["F_gt"].to(DEV), sc["Ks"].to(DEV)
    g = ref.grid(IM_SHAPE)[0]
    R = [ref.correct_matches(sc["F_gt"][b].double().numpy(), g, g) for b in range(4)]
    homo = lambda k: torch.as_tensor(np.stack([np.c_[np.float32(r[k]), np.ones(100, np.float32)] for r in R]), device=DEV)
    floor = dfepe.ops.epi_residual(homo("p"), homo("q"), F.float(), 0.5)
    floor_max, floor_mean = float(floor.max()), float(floor.mean())
    bound_max = 1e-4 if floor_max <= 1e-4 else 4 * floor_max
    bound_mean = 1e-4 if floor_mean <= 1e-4 else 4 * floor_mean
    p1n, p2n, p1, p2 = dfepe.compat.utils_misc.get_virt_x1x2_batch(IM_SHAPE, F, K)
    res = dfepe.ops.epi_residual(p1, p2, F.float(), 0.5)
    print(f"epi_residual of the virtual points under F_gt: max {float(res.max()):.2e}, mean {float(res.mean()):.2e}; "
          f"of the restatement's points: max {floor_max:.2e}, mean {floor_mean:.2e}")
    assert float(res.max()) <= bound_max
    depth = 2
    eye = torch.eye(3, device=DEV).repeat(4, 1, 1)
    Ff = F.float()
    outs = {"weights": None, "F_est": Ff, "T1": eye, "T2": eye, "out_layers": [Ff] * depth, "residual_layers": [], "weights_layers": [],
            "epi_res_layers": []}
    losses = dfepe.compat.train_good_utils.get_all_loss_DeepF(outs, p1, p2, K, {"depth": depth, "clamp_at": 0.02},
                                                              get_residual_summaries=False)[0]
    print(f"loss_F {float(losses['loss_F']):.2e}, per layer {[float(x) for x in losses['loss_layers']]}")
    assert 0.0 <= float(losses["loss_F"]) <= bound_mean  # a mean over the virtual points of the same residual
    assert all(0.0 <= float(x) <= bound_mean for x in losses["loss_layers"])
