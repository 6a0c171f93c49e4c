"""dfepe_correct_matches on the device at every geometry and launch edge: every family of tests/correct_matches_cases.py through
ops.correct_matches and the same check() that the host header goes through in tests/test_correct_matches_ref_cpu.py (float32 output:
cost through np.float32 of the interval's ends, positions to max(2^-13 px, the float32 spacing at the reference coordinate)), the
exact relations, the launch edges of the 256-lane workgroups and of F + (i / M) * f_stride, NaN lanes, the C ABI's output extents
and the wrappers.  The reference is the fp64 restatement only; nothing here imports mpmath or reads the reference project.

Launch inputs are assembled from the families' own points (and their cached restatement), so a launch costs no new reference."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import correct_matches_cases as cs  # noqa: E402
import correct_matches_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = cs.names()
INTEGER = ["forward_integer"] + [f"near_epipole[{s:g},{side}]" for s in cs.SIGMAS for side in cs.SIDES]  # all under F = [e]x
RINGS = ["rings[5]", "rings[50]", "close_matches", "on_line_rounded", "far"]                                # all under the rings' F


def device(dfepe, F, P, Q, want_cost=True):
    """F [B,3,3] or [3,3], P, Q [B,M,2] -> [B,M,5] float32 (corrected p, corrected q, cost; cost column NaN-free only if asked)."""
    out = dfepe.ops.correct_matches(torch.as_tensor(np.ascontiguousarray(F), device=DEV), torch.as_tensor(np.ascontiguousarray(P), device=DEV),
                                    torch.as_tensor(np.ascontiguousarray(Q), device=DEV), want_cost=want_cost)
    assert all(o.dtype == torch.float32 and o.device == torch.device(DEV) for o in out)
    new1, new2 = out[0].cpu().numpy(), out[1].cpu().numpy()
    assert new1.shape == new2.shape == tuple(P.shape)
    cost = out[2].cpu().numpy() if want_cost else np.zeros(P.shape[:2], np.float32)
    return np.concatenate((new1, new2, cost[..., None]), -1)


def pair(names, n):
    """One pair of n points from families that share their F: (F, P, Q, R) with R the matching slice of their restatements."""
    fams = [cs.family(x) for x in names]
    assert all(np.array_equal(f[0], fams[0][0]) for f in fams)
    P, Q = np.concatenate([f[1] for f in fams])[:n], np.concatenate([f[2] for f in fams])[:n]
    assert len(P) == n
    R = {k: np.concatenate([cs.reference(x)[k] for x in names])[:n] for k in ("p", "q", "cost", "near_tie")}
    return fams[0][0], P, Q, R


def nine_pairs():
    """Nine distinct pairs of 129 points under six geometries."""
    groups = [INTEGER[0:3], INTEGER[3:6], INTEGER[6:9], INTEGER[9:12], RINGS[0:3], RINGS[2:5],
              ["planar_translation", "planar_translation", "planar_translation"], ["near_infinity[1e-12]"] * 3, ["rectified"] * 3]
    return [pair(g, 129) for g in groups]


@pytest.mark.parametrize("name", NAMES)
def test_every_family_through_the_check(dfepe, name):
    F, P, Q = cs.family(name)
    got = device(dfepe, F[None], P[None], Q[None])[0]
    cs.check(got, name)
    if name == "on_geometry":  # integer pixels exactly on an integer geometry: the outputs are the inputs, bit for bit
        assert np.array_equal(got[:, :2], P) and np.array_equal(got[:, 2:4], Q)
    host = cs.header(F, P, Q)[0]
    c, p = cs.distance(got, host)
    print(f"CM {name}: device (float32) against the host header (fp64): cost {c:.2e} relative, position {p:.2e} px")


@pytest.mark.parametrize("name", NAMES)
def test_exact_relations(dfepe, name):
    """Bit for bit: -F, 2^+-40 F, want_cost=False, a shared F [3,3] against its broadcast [B,3,3].  To the bounds of check():
    correct(F^T, q, p) = (q', p') with the same cost."""
    F, P, Q = cs.family(name)
    P2, Q2 = np.stack((P, Q)), np.stack((Q, P))  # two pairs, so that the shared F is used by more than one
    got = device(dfepe, F, P2, Q2)
    Fs = np.stack((-F, F * 2.0 ** 40, F * 2.0 ** -40, F))
    rel = device(dfepe, Fs, np.broadcast_to(P, (4,) + P.shape), np.broadcast_to(Q, (4,) + Q.shape))
    for k, what in enumerate(("-F", "2^40 F", "2^-40 F", "F [B,3,3]")):
        assert np.array_equal(rel[k], got[0], equal_nan=True), f"{name}: {what}"
    assert np.array_equal(device(dfepe, np.broadcast_to(F, (2, 3, 3)), P2, Q2), got, equal_nan=True)
    assert np.array_equal(device(dfepe, F, P2, Q2, want_cost=False)[..., :4], got[..., :4], equal_nan=True)
    t = device(dfepe, F.T[None], Q[None], P[None])[0]
    cs.check(np.ascontiguousarray(t[:, [2, 3, 0, 1, 4]]), name, tag=f"{name} transposed")


@pytest.mark.parametrize("total", [1, 63, 64, 65, 255, 256, 257, 511, 513])
def test_lane_totals_around_the_wavefront_and_the_workgroup(dfepe, total):
    F, P, Q, R = pair(INTEGER, total)
    got = device(dfepe, F[None], P[None], Q[None])[0]
    cs.check_against(got, F, P, Q, R, f"{total} lanes")


def test_every_lane_its_own_F(dfepe):
    """B = 257, M = 1: lane i reads F + i * 9, from six geometries in turn."""
    names = ["forward_integer", "rings[50]", "kitti", "planar_translation", "near_infinity[1e-12]", "rectified"]
    lanes = [(names[i % 6], (i // 6) % cs.N) for i in range(257)]
    F = np.stack([cs.family(n)[0] for n, _ in lanes])
    P = np.stack([cs.family(n)[1][j] for n, j in lanes])[:, None]
    Q = np.stack([cs.family(n)[2][j] for n, j in lanes])[:, None]
    got = device(dfepe, F, P, Q)[:, 0]
    for k, n in enumerate(names):
        sel = np.arange(k, 257, 6)
        R = {key: np.stack([cs.reference(n)[key][j] for _, j in lanes[k::6]]) for key in ("p", "q", "cost", "near_tie")}
        cs.check_against(got[sel], F[k], P[sel, 0], Q[sel, 0], R, f"own F, {n}")


def test_pair_boundaries_inside_a_workgroup(dfepe):
    """B = 3, M = 171: the pairs change at lanes 171 and 342, the workgroups at 256 and 512."""
    pairs = [pair(INTEGER, 171), pair(RINGS, 171), pair(["planar_translation"] * 3, 171)]
    got = device(dfepe, np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]), np.stack([p[2] for p in pairs]))
    for b, (F, P, Q, R) in enumerate(pairs):
        cs.check_against(got[b], F, P, Q, R, f"pair {b} of 3 x 171")


def test_a_lanes_result_does_not_depend_on_where_it_sits(dfepe):
    """B = 513, M = 129: 66177 lanes in 259 workgroups, nine distinct pairs repeated.  The first nine are held to the restatement,
    every other pair is bitwise its original."""
    nine = nine_pairs()
    idx = np.arange(513) % 9
    F, P, Q = (np.stack([nine[k][j] for k in idx]) for j in range(3))
    got = device(dfepe, F, P, Q)
    for b in range(9):
        cs.check_against(got[b], *nine[b][:3], nine[b][3], f"pair {b} of 513 x 129")
    assert np.array_equal(got, got[idx], equal_nan=True)


def test_nan_lanes_and_their_neighbours(dfepe):
    """A point on the epipole in the first image only (lanes 63 and 256), the second only (64) and both (255): all five outputs of
    those lanes are NaN, and every other lane is bitwise what it is without them."""
    F, P, Q, R = pair(INTEGER, 300)
    base = device(dfepe, F[None], P[None], Q[None])[0]
    P2, Q2 = P.copy(), Q.copy()
    e = cs.E_INTEGER.astype(np.float32)
    P2[63], Q2[64], P2[255], Q2[255], P2[256] = e, e, e, e, e
    got = device(dfepe, F[None], P2[None], Q2[None])[0]
    bad = np.zeros(300, bool)
    bad[[63, 64, 255, 256]] = True
    assert np.isnan(got[bad]).all() and np.isfinite(got[~bad]).all()
    assert np.array_equal(got[~bad], base[~bad])
    for i in np.flatnonzero(bad):
        assert np.isnan(ref.correct_one(F, P2[i], Q2[i])["cost"])
    R2 = ref.correct_matches(F, P2[bad], Q2[bad])
    cs.check_against(got[bad], F, P2[bad], Q2[bad], R2, "NaN lanes")  # NaN exactly where the restatement has NaN


@pytest.mark.parametrize("with_cost", [True, False])
@pytest.mark.parametrize("total", [1, 255, 257])
def test_cabi_writes_inside_its_outputs_only(dfepe, total, with_cost):
    """The outputs are views into larger tensors with 64 sentinel floats on either side."""
    F, P, Q, R = pair(INTEGER, total)
    L = dfepe._lib.lib()
    Fd, p, q = (torch.as_tensor(np.ascontiguousarray(x), device=DEV) for x in (F, P, Q))
    S = -12345.0
    bufs = [torch.full((64 + n + 64,), S, device=DEV) for n in (2 * total, 2 * total, total)]
    views = [b[64:-64] for b in bufs]
    torch.cuda.synchronize()
    rc = L.dfepe_correct_matches(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), Fd.data_ptr(), 0, p.data_ptr(), q.data_ptr(), 1,
                                 total, views[0].data_ptr(), views[1].data_ptr(), views[2].data_ptr() if with_cost else None)
    torch.cuda.synchronize()
    assert rc == 0
    for b in bufs:
        assert (b[:64] == S).all() and (b[-64:] == S).all()
    if not with_cost:
        assert (bufs[2] == S).all()
    got = np.concatenate((views[0].cpu().numpy().reshape(total, 2), views[1].cpu().numpy().reshape(total, 2),
                          views[2].cpu().numpy()[:, None]), 1)
    want = device(dfepe, F[None], P[None], Q[None])[0]
    assert np.array_equal(got[:, :4], want[:, :4]) and (not with_cost or np.array_equal(got[:, 4], want[:, 4]))
    assert L.dfepe_version() == 154


def test_wrapper_takes_strided_points_and_any_float_F(dfepe):
    F, P, Q, _ = pair(RINGS, 200)
    want = device(dfepe, F[None], P[None], Q[None])
    wide_p = torch.as_tensor(np.concatenate((P, Q), 1)[None], device=DEV)   # [1,200,4]: both views are non-contiguous
    p, q = wide_p[..., :2], wide_p[..., 2:]
    assert not p.is_contiguous() and not q.is_contiguous()
    Fd = torch.as_tensor(F, device=DEV)
    new1, new2, cost = dfepe.ops.correct_matches(Fd[None], p, q, want_cost=True)
    got = torch.cat((new1, new2, cost[..., None]), -1).cpu().numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(wide_p.cpu().numpy()[0], np.concatenate((P, Q), 1))  # the inputs are left alone
    # a float32 F is widened, not computed in float32: the same bits as the widened F handed over as float64
    F32 = Fd.float()
    a = dfepe.ops.correct_matches(F32, p, q, want_cost=True)
    b = dfepe.ops.correct_matches(F32.double(), p, q, want_cost=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_get_virt_x1x2_batch_with_both_epipoles_at_infinity(dfepe):
    """get_virt_x1x2_batch on the planar translations (sideways motion: the case no test reached) against the restatement pushed
    through the reference's lines.  The grid's points are the same in both images, so the call's swapped arguments do not show."""
    um = dfepe.compat.utils_misc
    Fs = np.stack([cs.family("planar_translation")[0], cs.family("planar_translation_rot")[0], cs.family("near_infinity[1e-12]")[0]])
    Ks = np.broadcast_to(cs.K, (3, 3, 3)).copy()
    out = um.get_virt_x1x2_batch(cs.IM_SHAPE, torch.as_tensor(Fs, device=DEV), torch.as_tensor(Ks, device=DEV))
    assert all(x.shape == (3, 100, 3) and x.dtype == torch.float32 for x in out)
    g1, g2 = ref.grid(cs.IM_SHAPE)
    norm_tol = cs.POS_FP32 * np.abs(np.linalg.inv(cs.K)).sum(1).max()  # a pixel error of 2^-13 through inv(K)
    for b in range(3):
        want = ref.virt_through_the_reference_lines(Fs[b], cs.K, g1, g2)
        got = [x[b].cpu().numpy() for x in out]
        # x^T K^-T [t]x K^-1 x = 0: under a pure translation equal points are on the geometry already; the rotation moves them
        moved = np.abs(want[2][:, :2] - g1).max()
        assert np.isfinite(want[2]).all() and (moved > 0.1 if b == 1 else moved <= 2.0 ** -13)
        assert np.abs(got[2] - want[2]).max() <= cs.POS_FP32 and np.abs(got[3] - want[3]).max() <= cs.POS_FP32
        # + the rounding of a normalised coordinate (at most 1 in magnitude) to float32
        assert np.abs(want[0]).max() <= 1.0 and np.abs(got[0] - want[0]).max() <= norm_tol + 2.0 ** -25 and np.array_equal(got[0], got[1])
        assert (got[2][:, 2] == 1).all() and (got[3][:, 2] == 1).all()
