"""dfepe_geo_misc on the device (csrc/geom.hip: geo_misc_kernel, kinds 0..6) against the float64 restatement of
tests/pose_helper_ref.py over the case table of tests/pose_helper_cases.py, with that table's own check(): kinds 0, 1, 2, 5, 6 to one
float32 ulp of the rounded reference plus the reference's conditioning term, kind 3 to 4 * 2^-24 + 4 K 2^-52 s1 / (s2 - s3) with the K
measured on the host build of svd3_closed (tests/test_pose_helper_ref_cpu.py), kind 4 as a set of rotations and +-t to the same
bound; the exact results where the formulas give them; every launch edge of the 256-lane workgroups; position independence; NaN rows;
the C entry point's argument checks.  The reference of a kind is computed once per process and shared by every test."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_helper_cases as cs  # noqa: E402
import pose_helper_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = (0, 1, 2, 3, 4, 5, 6)


def device(dfepe, kind, in0, in1=None):
    """[n,w] float32 numpy in -> [n,OUT_WIDTH[kind]] float32 numpy out, through ops.geo_misc."""
    a = torch.as_tensor(np.ascontiguousarray(in0), device=DEV)
    b = None if in1 is None else torch.as_tensor(np.ascontiguousarray(in1), device=DEV)
    out = dfepe.ops.geo_misc(kind, a, b)
    assert out.dtype == torch.float32 and out.shape == (len(in0), cs.OUT_WIDTH[kind])
    return out.cpu().numpy()


@pytest.mark.parametrize("kind", KINDS)
def test_every_family_through_the_check(dfepe, kind):
    in0, in1, names = cs.pool(kind)
    got = device(dfepe, kind, in0, in1)
    worst = cs.check(kind, got, slice(None), tag="device")
    print(f"POSEHELP kind {kind}: {len(in0)} items of {len(set(names))} families, worst error {worst:.3f} of its bound")


def test_the_public_wrappers_are_the_kinds(dfepe):
    """rot_to_quat, rot_angle_deg, vector_angle_deg, project_essential, decompose_essential, congruence, camera_rotation: the same
    bits as geo_misc on the same items, in the shapes they document."""
    o = dfepe.ops
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=DEV)
    p = {k: cs.pool(k) for k in KINDS}
    base = {k: device(dfepe, k, p[k][0], p[k][1]) for k in KINDS}
    assert np.array_equal(o.rot_to_quat(t(p[0][0].reshape(-1, 3, 3))).cpu().numpy(), base[0])
    assert np.array_equal(o.rot_angle_deg(t(p[1][0].reshape(-1, 3, 3)), t(p[1][1].reshape(-1, 3, 3))).cpu().numpy(), base[1][:, 0])
    assert np.array_equal(o.vector_angle_deg(t(p[2][0]), t(p[2][1])).cpu().numpy(), base[2][:, 0])
    assert np.array_equal(o.project_essential(t(p[3][0].reshape(-1, 3, 3))).cpu().numpy().reshape(-1, 9), base[3])
    R1, R2, tt = o.decompose_essential(t(p[4][0].reshape(-1, 3, 3)))
    assert R1.shape == R2.shape == (len(base[4]), 3, 3) and tt.shape == (len(base[4]), 3)
    assert np.array_equal(np.concatenate((R1.cpu().numpy().reshape(-1, 9), R2.cpu().numpy().reshape(-1, 9), tt.cpu().numpy()), 1), base[4])
    assert np.array_equal(o.congruence(t(p[5][0].reshape(-1, 3, 3)), t(p[5][1].reshape(-1, 3, 3))).cpu().numpy().reshape(-1, 9), base[5])
    assert np.array_equal(o.camera_rotation(t(p[6][0].reshape(-1, 4, 4))).cpu().numpy().reshape(-1, 9), base[6])


def test_exact_results(dfepe):
    """Where the formula gives the result exactly, so does the kernel: the quaternions of the 0 / +-1 rotations (every tie of the
    branch predicates), equal / opposite vectors at norm 1e12 (0 and 180), a zero vector (90), a rotation against itself (0)."""
    sl = cs.family_slice(0, "exact")
    got = device(dfepe, 0, cs.pool(0)[0][sl])
    for name, q in zip(cs.EXACT_ROTATIONS, got):
        want = np.array(cs.EXACT_QUATERNIONS[name], np.float32)
        assert np.array_equal(q, want) and np.array_equal(np.signbit(q), np.signbit(want)), (name, q)
    vp = cs.vector_pairs()
    got = device(dfepe, 2, np.stack([v[1] for v in vp]), np.stack([v[2] for v in vp]))[:, 0]
    n_exact = 0
    for (name, _, _, exact), a in zip(vp, got):
        if exact is not None:
            assert a == np.float32(exact), (name, a)
            n_exact += 1
    assert n_exact >= 18
    R0, R1, deg = cs.angle_pairs()
    got = device(dfepe, 1, R0.reshape(-1, 9), R1.reshape(-1, 9))[:, 0]
    assert (deg == 0.0).sum() == 4 and (got[deg == 0.0] == 0.0).all() and not np.signbit(got[deg == 0.0]).any()
    assert (got[deg == 180.0] == np.float32(180.0)).all()  # 180 - 3e-6 degrees rounds to 180 in float32
    assert (got[deg > 0.0] > 0.0).all()


def test_generating_pose_is_among_the_candidates(dfepe):
    """[t]x R in float32, at every scale: one of the two rotations is R and t is +-t, as far as the float32 rounding of E lets the
    float64 reference on the same input recover them, plus the bound of kind 3."""
    R, t = cs.poses()
    in0 = cs.pool(4)[0]
    ex = cs.expected(4)
    for name in ("txR", "txR*2^-20", "txR*1e-6", "txR*1e+6"):
        sl = cs.family_slice(4, name)
        got = device(dfepe, 4, in0[sl]).astype(np.float64)
        for j, i in enumerate(range(sl.start, sl.stop)):
            ref_R = min(np.abs(ex["R1"][i].reshape(3, 3) - R[j]).max(), np.abs(ex["R2"][i].reshape(3, 3) - R[j]).max())
            ref_t = min(np.abs(ex["t"][i] - t[j]).max(), np.abs(ex["t"][i] + t[j]).max())
            got_R = min(np.abs(got[j, 0:9].reshape(3, 3) - R[j]).max(), np.abs(got[j, 9:18].reshape(3, 3) - R[j]).max())
            got_t = min(np.abs(got[j, 18:21] - t[j]).max(), np.abs(got[j, 18:21] + t[j]).max())
            assert got_R <= ref_R + ex["tol"][i] and got_t <= ref_t + ex["tol"][i], (name, j, got_R, ref_R, got_t, ref_t)


@pytest.mark.parametrize("kind", (3, 4))
def test_a_power_of_two_changes_no_bit(dfepe, kind):
    """The prescale of svd3_closed is exact: 2^+-20 E for every family, and [e_k]x from float32 denormals (2^-140) to 2^120."""
    in0 = cs.pool(kind)[0]
    base = device(dfepe, kind, in0)
    for k in (-20, 20):
        assert np.array_equal(device(dfepe, kind, in0 * np.float32(2.0 ** k)), base), k
    sl = cs.family_slice(kind, "axis")
    for k in (-140, -126, 120):
        x = in0[sl] * np.float32(2.0 ** k)
        assert (x != 0).sum() == 2 * len(x)
        assert np.array_equal(device(dfepe, kind, x), base[sl]), k


@pytest.mark.parametrize("n", cs.LAUNCH_SIZES)
def test_launch_sizes(dfepe, n):
    """n = 0 (an empty tensor, nothing launched), one lane, either side of a wavefront and of a workgroup, four workgroups: every kind,
    every item held to the restatement, and the memory behind the output untouched."""
    for kind in KINDS:
        in0, in1, idx = cs.batch(kind, n, offset=3 * kind)
        w = cs.OUT_WIDTH[kind]
        a = torch.as_tensor(np.ascontiguousarray(in0), device=DEV)
        b = None if in1 is None else torch.as_tensor(np.ascontiguousarray(in1), device=DEV)
        out = dfepe.ops.geo_misc(kind, a, b)
        assert out.shape == (n, w) and out.dtype == torch.float32
        if n:
            cs.check(kind, out.cpu().numpy(), idx, tag=f"n = {n}")
        # the same launch through the C entry point into the middle of a larger buffer
        S = -12345.0
        buf = torch.full((64 + n * w + 64,), S, device=DEV)
        torch.cuda.synchronize()
        rc = dfepe._lib.lib().dfepe_geo_misc(kind, a.data_ptr() if n else None, None if b is None or not n else b.data_ptr(), n,
                                             buf[64:].data_ptr() if n else None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc == 0
        assert (buf[:64] == S).all() and (buf[64 + n * w:] == S).all()
        assert torch.equal(buf[64:64 + n * w].view(n, w), out)


@pytest.mark.parametrize("kind", KINDS)
def test_an_items_bits_do_not_depend_on_where_it_sits(dfepe, kind):
    """257 items, shuffled: each item's output is bit for bit what a launch of that item alone gives (for a handful of them, from
    both workgroups), and what it is at any other position of the batch."""
    in0, in1, idx = cs.batch(kind, 257)
    perm = np.random.default_rng(kind).permutation(257)
    got = device(dfepe, kind, in0[perm], None if in1 is None else in1[perm])
    straight = device(dfepe, kind, in0, in1)
    assert np.array_equal(got, straight[perm])
    for pos in (0, 1, 63, 64, 255, 256):
        one = device(dfepe, kind, in0[perm[pos]][None], None if in1 is None else in1[perm[pos]][None])
        assert np.array_equal(one[0], got[pos]), pos
    cs.check(kind, got, idx[perm], tag="shuffled")


@pytest.mark.parametrize("kind", KINDS)
def test_a_nan_row_stays_in_its_row(dfepe, kind):
    """Rows 0, 63, 255 and 256 of 300 are NaN (in0; for the two-input kinds row 64 has the NaN in in1): NaN there, every other row
    bit for bit what it is without them, and the call returns."""
    in0, in1, idx = cs.batch(kind, 300)
    base = device(dfepe, kind, in0, in1)
    a, b = in0.copy(), None if in1 is None else in1.copy()
    bad = [0, 63, 255, 256]
    a[bad] = np.nan
    if b is not None:
        b[64] = np.nan
        bad.append(64)
    got = device(dfepe, kind, a, b)
    mask = np.zeros(300, bool)
    mask[bad] = True
    assert np.isnan(got[mask]).all()
    assert np.array_equal(got[~mask], base[~mask]) and np.isfinite(got[~mask]).all()


def test_the_c_entry_point_rejects_what_it_cannot_run(dfepe):
    L = dfepe._lib.lib()
    x = torch.zeros(4, 16, device=DEV)
    o = torch.full((4, 21), 7.0, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for kind in (-1, 7, 8, 1 << 20):
        assert L.dfepe_geo_misc(kind, x.data_ptr(), x.data_ptr(), 4, o.data_ptr(), st) != 0
    for kind in (1, 2, 5):  # the two-input kinds without in1
        assert L.dfepe_geo_misc(kind, x.data_ptr(), None, 4, o.data_ptr(), st) != 0
    for kind in KINDS:
        assert L.dfepe_geo_misc(kind, None, x.data_ptr(), 4, o.data_ptr(), st) != 0
        assert L.dfepe_geo_misc(kind, x.data_ptr(), x.data_ptr(), 4, None, st) != 0
        assert L.dfepe_geo_misc(kind, x.data_ptr(), x.data_ptr(), -1, o.data_ptr(), st) != 0
        assert L.dfepe_geo_misc(kind, None, None, 0, None, st) == 0
    torch.cuda.synchronize()
    assert (o == 7.0).all()  # nothing was launched
    with pytest.raises(dfepe._lib.DfepeError):
        dfepe.ops.geo_misc(1, x[:, :9].contiguous(), None)
