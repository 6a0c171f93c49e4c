"""The float64 restatement of the pose helpers (tests/pose_helper_ref.py) and its case table (tests/pose_helper_cases.py) are
themselves right: the quaternion against the generating axis-angle, the angles against np.longdouble and the generating angle, the
projection as the nearest matrix with singular values (1, 1, 0), the decomposition against oracle.get_M2s and the generating pose,
the stated gaps, condition numbers and branch memberships of every family -- and the HOST build of csrc/dfepe_math.h's svd3_closed
(tests/emu/emu_svd3.cpp) over the same table against np.linalg.svd, which is where the constant K_SVD3 of the GPU suite's kind-3
bound comes from.  Runs without a GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_helper_cases as cs  # noqa: E402
import pose_helper_ref as ref  # noqa: E402

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EMU_DIR = os.path.join(REPO, "tests", "emu")
CSRC = os.path.join(REPO, "pytorch-deepfepe_amd", "csrc")


@pytest.fixture(scope="module")
def emu():
    out = os.path.join(EMU_DIR, "_build")
    os.makedirs(out, exist_ok=True)
    lib = os.path.join(out, "libemu_svd3.so")
    srcs = [os.path.join(EMU_DIR, "emu_svd3.cpp"), os.path.join(EMU_DIR, "rowgroup.h"), os.path.join(CSRC, "dfepe_math.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", f"-I{EMU_DIR}", f"-I{CSRC}", srcs[0], "-o", lib], check=True)
    L = ctypes.CDLL(lib)
    P, I = ctypes.c_void_p, ctypes.c_int
    L.emu_svd3_closed.argtypes = [P, I, P, P, P]
    L.emu_svd3_closed.restype = None
    L.emu_project_essential.argtypes = [P, I, P, P]
    L.emu_project_essential.restype = None
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_project(L, E32):
    E32 = np.ascontiguousarray(E32, np.float32).reshape(-1, 9)
    o64, o32 = np.zeros((len(E32), 9)), np.zeros((len(E32), 9), np.float32)
    L.emu_project_essential(_p(E32), len(E32), _p(o64), _p(o32))
    return o64, o32


def quat_to_matrix(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


# ---- kind 0 ---------------------------------------------------------------------------------------------------------------------
def test_quaternion_is_the_generating_axis_angle(oracle):
    g = np.random.default_rng(11)
    for deg in (1e-3, 1.0, 60.0, 90.0, 120.0, 179.0, 179.999, 180.0):
        for _ in range(4):
            k = g.standard_normal(3)
            k /= np.linalg.norm(k)
            R32 = cs.rodrigues(k, np.radians(deg)).astype(np.float32)
            q, _, _, _ = ref.quat(R32)
            want = np.concatenate(([np.cos(np.radians(deg) / 2)], np.sin(np.radians(deg) / 2) * k))
            # float32 rounding of R (6e-8 per entry) through the best-conditioned branch: every component to a few 1e-7; at 180 degrees
            # q and -q are the same rotation and q0 ~ 0 has either sign
            assert min(np.abs(q - want).max(), np.abs(q + want).max() if deg >= 179.999 else np.inf) <= 4e-7, (deg, q, want)
            assert q[0] >= 0.0 and abs(np.linalg.norm(q) - 1.0) <= 4e-7
            np.testing.assert_allclose(q, oracle.R_to_q(torch.from_numpy(R32.astype(np.float64)))[:, 0].numpy(), rtol=0, atol=2 * ref.EPS64)
    for name, x in cs.rotations().items():
        for R32 in x:
            q = ref.quat(R32)[0]
            assert q[0] >= 0.0 and np.abs(quat_to_matrix(q / np.linalg.norm(q)) - R32.astype(np.float64)).max() <= 5e-7, name


def test_quaternion_branches_flips_and_exact_ties():
    ex = cs.expected(0)
    margins = []
    for k in range(4):
        sl = cs.family_slice(0, f"branch{k}")
        assert (ex["branch"][sl] == k).all(), (k, ex["branch"][sl])
        if k < 3:
            assert 4 <= ex["flip"][sl].sum() <= 8, (k, ex["flip"][sl])  # both states of the q0 >= 0 flip
        else:
            assert not ex["flip"][sl].any()                              # q0 = t / (2 sqrt(t)) > 0
        for R32 in cs.rotations()[f"branch{k}"]:
            d = np.diag(R32.astype(np.float64))
            margins.append(min(abs(d[2]), abs(d[0] - d[1]) if d[2] < 0 else abs(d[0] + d[1])))
    assert min(margins) >= 0.02, min(margins)  # no generic case sits on a predicate
    sl = cs.family_slice(0, "exact")
    br = dict(zip(cs.EXACT_ROTATIONS, ex["branch"][sl]))
    # M22 == 0 is "not negative", M00 == M11 is "not greater", M00 == -M11 is "not less": the second alternative every time
    assert br == {"identity": 3, "x180": 0, "y180": 1, "z180": 2, "x90": 3, "x-90": 3, "y90": 3, "y-90": 3, "z90": 3, "z-90": 3,
                  "xy180": 1, "xz180": 2, "yz180": 2, "cyc": 3, "cyc'": 3}, br
    for name, q in zip(cs.EXACT_ROTATIONS, ex["want"][sl]):
        np.testing.assert_array_equal(q.astype(np.float32), np.array(cs.EXACT_QUATERNIONS[name], np.float32), err_msg=name)
        assert not np.signbit(q).any() or name in ("x-90", "y-90", "z-90", "cyc'"), name  # the zeros are +0
    assert np.bincount(ex["branch"], minlength=4).min() >= 12
    for R32 in cs.rotations()["rounded"]:
        r = R32.astype(np.float64)
        assert 1e-9 < np.abs(r @ r.T - np.eye(3)).max() < 1e-6  # not exactly orthonormal


# ---- kinds 1, 2 -------------------------------------------------------------------------------------------------------------------
def test_rotation_angle_against_longdouble_and_the_generating_angle(oracle):
    R0, R1, deg = cs.angle_pairs()
    ex = cs.expected(1)
    worst = 0.0
    for i in range(len(deg)):
        a, cond = ex["want"][i, 0], ex["cond"][i, 0]
        assert a == oracle.rotation_angle_deg(R0[i].astype(np.float64), R1[i].astype(np.float64)) or abs(a - oracle.rotation_angle_deg(R0[i], R1[i])) <= 1e-9
        # the same float32 inputs in extended precision: the float64 restatement's own error.  The axis part cancels to
        # ~2^-52 absolutely, which is 1e-10 of the 1e-4 degree cases and invisible in float32
        assert abs(a - ref.rotation_angle_longdouble(R0[i], R1[i])) <= 1e-9 * max(a, 1e-4), (deg[i], a)
        # the generating angle, to the float32 rounding of the two matrices (2 x 6e-8 rad on the chord = 2e-5 degrees)
        assert abs(a - deg[i]) <= 2e-5, (deg[i], a)
        worst = max(worst, cond)
        assert cond <= 2.0 ** -24 * max(a, 1e-4)  # the term is far inside a float32 ulp: atan2 has no ill-conditioned end
    assert ex["want"][deg == 0.0].max() == 0.0     # R0 is R1 bit for bit: the axis part cancels exactly
    print(f"kind 1: largest conditioning term {worst:.3e} degrees")


def test_vector_angle_against_the_oracle_and_the_exact_cases(oracle):
    vp = cs.vector_pairs()
    ex = cs.expected(2)
    worst = {}
    for i, (name, a, b, exact) in enumerate(vp):
        ang, cond = ex["want"][i, 0], ex["cond"][i, 0]
        assert abs(ang - oracle.vector_angle_deg(a, b)) <= 1e-12 * 180.0, name
        if exact is not None:
            assert np.float32(ang) == np.float32(exact), (name, ang)
        fam = name.split("[")[0]
        worst[fam] = max(worst.get(fam, 0.0), cond)
        if fam in ("near_parallel", "near_antiparallel"):
            off = ang if fam == "near_parallel" else 180.0 - ang
            # 1e-3 degrees by construction; float32 rounding of a unit vector moves the direction by up to 1e-7 rad = 6e-6 degrees... and
            # the 1e-10 terms of the formula add acos(1 - 3e-10) = 1.4e-3 degrees in quadrature
            assert 0.9e-3 <= off <= 3.0e-3, (name, off)
        if fam in ("equal", "opposite"):
            # |v| ~ 1: the 1e-10 terms are not absorbed, the cosine is n^2 / ((n + 1e-10)^2 + 1e-10) and the angle sqrt(2 (1 - cos)),
            # about 1e-3 degrees: what the formula gives, not 0 (or 180)
            n = np.sqrt((a.astype(np.longdouble) ** 2).sum())
            off = float(np.degrees(np.sqrt(2 * (1 - n * n / ((n + np.longdouble(1e-10)) ** 2 + np.longdouble(1e-10))))))
            assert 5e-4 <= off <= 3e-3 and abs((ang if fam == "equal" else 180.0 - ang) - off) <= 1e-6 * off + 1e-12 * 180.0, (name, ang, off)
    print("kind 2: largest conditioning terms (degrees):", {k: f"{v:.2e}" for k, v in worst.items()})
    # acos is ill-conditioned at +-1 only: 4 ulps of a cosine 1 - 3e-10 (|v| ~ 1) are 2e-9 degrees; of the cosine 1 itself (the 1e12
    # cases, whose result is 0 or 180 exactly) sqrt(2 * 4 * 2^-53) rad = 2.4e-6 degrees
    assert max(v for k, v in worst.items() if "1e12" not in k) <= 2e-9 and max(worst.values()) <= 2.5e-6


# ---- kinds 3, 4 -------------------------------------------------------------------------------------------------------------------
def test_families_have_the_gaps_they_state():
    fam = cs.essentials()
    gap = {k: np.array([ref.relative_gap(x) for x in v]) for k, v in fam.items()}
    for k in ("txR", "txR*2^-20", "txR*1e-6", "txR*1e+6", "axis"):
        assert gap[k].min() >= 1.0 - 1e-6, (k, gap[k])
        s = np.array([ref.singular_values(x) for x in fam[k]])
        assert (np.abs(s[:, 0] - s[:, 1]) <= 4e-7 * s[:, 0]).all() and (s[:, 2] <= 4e-7 * s[:, 0]).all()
    assert gap["generic"].min() >= 1e-2 and gap["generic"].max() <= 1.0
    assert min(np.linalg.svd(x.astype(np.float64), compute_uv=False)[2] for x in fam["generic"]) > 0.0
    mags = [np.abs(x).max() for x in fam["generic"]]
    assert min(mags) < 0.1 and max(mags) > 10.0
    assert (np.abs(gap["small_gap"] - 1e-6) <= 2e-7).all(), gap["small_gap"]
    for x in fam["rank1"]:
        s = ref.singular_values(x)
        assert s[0] > 0.0 and s[1] <= 1e-7 * s[0]
    assert not fam["zero"].any()
    np.testing.assert_array_equal(fam["txR*2^-20"], fam["txR"] * np.float32(2.0 ** -20))
    assert set(np.unique(fam["axis"])) == {-1.0, 0.0, 1.0}


def test_projection_is_idempotent_and_nearest():
    g = np.random.default_rng(5)
    for name, x in cs.essentials().items():
        if name in cs.DEGENERATE:
            continue
        for E32 in x:
            P = ref.project(E32)
            assert np.abs(np.linalg.svd(P, compute_uv=False) - [1, 1, 0]).max() <= 1e-14
            # idempotent, as far as a gap of (s2 - s3) / s1 = 1 of P itself lets float32(P) -> project -> differ: float32 rounding of P
            assert np.abs(ref.project(P.astype(np.float32)) - P).max() <= 4 * 2.0 ** -24, name
            # nearest in the Frobenius norm among the matrices with singular values (1, 1, 0), up to the scale of E
            s = ref.singular_values(E32)
            En = E32.astype(np.float64) / s[0]
            d0 = np.linalg.norm(En - P)
            for _ in range(4):
                Q1, Q2 = (cs.rodrigues(g.standard_normal(3), 10.0 ** g.uniform(-3, 0)) for _ in range(2))
                assert np.linalg.norm(En - Q1 @ P @ Q2) >= d0 - 1e-12, name


def test_decomposition_is_the_oracles_and_recovers_the_generating_pose(oracle):
    R, t = cs.poses()
    ex = cs.expected(4)
    in0 = cs.pool(4)[0]
    for name in cs.essentials():
        sl = cs.family_slice(4, name)
        for j, i in enumerate(range(sl.start, sl.stop)):
            Rs, ts = oracle.get_M2s(torch.from_numpy(in0[i].astype(np.float64).reshape(3, 3)))
            np.testing.assert_allclose(ex["R1"][i].reshape(3, 3), Rs[0].numpy(), atol=1e-12)
            np.testing.assert_allclose(ex["R2"][i].reshape(3, 3), Rs[1].numpy(), atol=1e-12)
            np.testing.assert_allclose(ex["t"][i], ts[0][:, 0].numpy(), atol=1e-12)
            if name not in cs.DEGENERATE:
                cs.check_so3(ex["R1"][i], name)
                cs.check_so3(ex["R2"][i], name)
            if name.startswith("txR"):
                # float32 rounding of E (relative 6e-8) through a decomposition with unit gap
                assert min(np.abs(ex["R1"][i].reshape(3, 3) - R[j]).max(), np.abs(ex["R2"][i].reshape(3, 3) - R[j]).max()) <= 5e-7, name
                assert min(np.abs(ex["t"][i] - t[j]).max(), np.abs(ex["t"][i] + t[j]).max()) <= 5e-7, name


# ---- kinds 5, 6 -------------------------------------------------------------------------------------------------------------------
def test_congruence_and_camera_rotation_references():
    F, A = cs.congruences()
    ex = cs.expected(5)
    L = np.longdouble
    for i in range(len(F)):
        want = (A[i].astype(L).T @ F[i].astype(L) @ A[i].astype(L)).astype(np.float64).reshape(9)
        assert (np.abs(ex["want"][i] - want) <= ex["cond"][i] + 1e-300).all()
    print(f"kind 5: largest conditioning term {ex['cond'].max():.3e} (entries up to {np.abs(ex['want']).max():.3e})")
    ex6, in6 = cs.expected(6), cs.pool(6)[0]
    conds = {}
    for name, m in cs.motions().items():
        sl = cs.family_slice(6, name)
        c = np.array([np.linalg.cond(x.astype(np.float64)) for x in m])
        conds[name] = (c.max(), ex6["cond"][sl].max())
        own = 0.0
        for x32, inv3, term in zip(m, ex6["want"][sl], ex6["cond"][sl, 0]):
            x = x32.astype(np.float64)
            if not name.startswith("general"):
                assert (x[3] == [0, 0, 0, 1]).all()
                assert np.abs(inv3.reshape(3, 3) - x[:3, :3].T).max() <= 2e-7  # a rotation rounded to float32: the inverse is the transpose
            else:
                assert np.abs(x[3] - [0, 0, 0, 1]).max() > 0.1  # a non-trivial last row
            # np.linalg.inv's own error on the nine entries that are compared, against Gauss-Jordan in np.longdouble, stays inside the
            # term cond2(delta) 2^-52 |block|_2 that the GPU suite grants on top of the float32 rounding
            e = np.abs(inv3.reshape(3, 3) - ref.inverse_longdouble(x32)[:3, :3].astype(np.float64)).max()
            assert e <= term, (name, e, term)
            own = max(own, e / term)
        conds[name] += (own,)
    assert conds["general"][0] <= cs.MAX_COND and conds["rigid"][0] <= 4.0 and 1e5 <= conds["rigid_far"][0] <= 4e6, conds
    ill = np.array([np.linalg.cond(x.astype(np.float64)) for x in cs.motions()["general_ill"]])
    assert ill.min() >= 1e2 and ill.max() <= cs.MAX_COND and ill.max() >= 5e2, ill
    print("kind 6: (largest condition number, largest conditioning term, reference's own error in units of it):",
          {k: (f"{a:.3g}", f"{b:.2e}", f"{c:.2f}") for k, (a, b, c) in conds.items()})
    full = np.stack([np.linalg.inv(x.astype(np.float64).reshape(4, 4)) @ x.astype(np.float64).reshape(4, 4) for x in in6])
    assert np.abs(full - np.eye(4)).max() <= 1e-9


# ---- the host build of svd3_closed ------------------------------------------------------------------------------------------------
def test_host_svd3_closed_stays_within_the_recorded_K(emu):
    """K = |host projection (float64, before the rounding to float32) - numpy's| / (2^-52 s1 / (s2 - s3)), per family; the rounded
    host output then passes the GPU suite's own check with margin 1."""
    in0, _, names = cs.pool(3)
    o64, o32 = host_project(emu, in0)
    ex = cs.expected(3)
    K = {}
    for i, name in enumerate(names):
        if name in cs.DEGENERATE:
            continue
        k = np.abs(o64[i] - ex["want"][i]).max() / (ref.EPS64 / ref.relative_gap(in0[i]))
        K[name] = max(K.get(name, 0.0), k)
    print("svd3_closed on the host, K per family:", {k: round(v, 1) for k, v in K.items()})
    assert max(K.values()) <= cs.K_SVD3, K
    assert max(K.values()) >= cs.K_SVD3 / 4.0, "K_SVD3 is far above what is observed: record the measured value"
    cs.check(3, o32, slice(None), tag="host")
    tol1 = np.array([cs.projection_tolerance(x, margin=1.0) for x in in0])
    live = np.array([n not in cs.DEGENERATE for n in names])
    assert (np.abs(o32.astype(np.float64) - ex["want"]).max(1)[live] <= tol1[live]).all()
    # the full factorisation: F = U S V^T to 2^-50 |F|, U and V orthonormal, S descending and >= 0
    F = np.ascontiguousarray(in0.astype(np.float64))
    U, S, V = np.zeros_like(F), np.zeros((len(F), 3)), np.zeros_like(F)
    emu.emu_svd3_closed(_p(F), len(F), _p(U), _p(S), _p(V))
    for i in range(len(F)):
        u, v = U[i].reshape(3, 3), V[i].reshape(3, 3)
        scale = max(np.abs(F[i]).max(), 1e-300)
        # small_gap: u3 and v3 are off by up to K 2^-52 s1 / (s2 - s3) each, and not by the same angle, which the product shows
        rec = 2 * cs.K_SVD3 * ref.EPS64 / ref.relative_gap(in0[i]) if names[i] == "small_gap" else 64 * ref.EPS64
        # a rounded outer product has s2 ~ 1e-8 s1 and no second triplet to speak of: kinds 3 and 4 promise invariants only there, and
        # only orthonormality is held here (seen: the product misses such an F by 7e-6 |F|, the cross products of sym3_null_vector
        # being round-off to 1e-2 and yet above its rank-1 threshold)
        if names[i] not in cs.DEGENERATE:
            assert np.abs(u @ np.diag(S[i]) @ v.T - F[i].reshape(3, 3)).max() <= rec * scale, names[i]
        assert np.abs(u.T @ u - np.eye(3)).max() <= 64 * ref.EPS64 and np.abs(v.T @ v - np.eye(3)).max() <= 64 * ref.EPS64, names[i]
        assert S[i][0] >= 0.0 and S[i][1] >= 0.0 and S[i][2] >= 0.0
        if names[i] in cs.DEGENERATE:  # s2 and s3 are round-off here, in whatever order the rank-1 route leaves them
            continue
        assert S[i][0] >= S[i][1] >= S[i][2]
        assert np.abs(S[i] - np.linalg.svd(F[i].reshape(3, 3), compute_uv=False)).max() <= rec * scale, names[i]


def test_host_projection_does_not_see_a_power_of_two(emu):
    """The prescale of svd3_closed is exact: 2^k E gives the same bits, down to float32 denormals (2^-140 [e_k]x) and up to 2^120."""
    in0, _, names = cs.pool(3)
    base = host_project(emu, in0)[0]
    for k in (-20, 20):
        np.testing.assert_array_equal(host_project(emu, in0 * np.float32(2.0 ** k))[0], base)
    sl = cs.family_slice(3, "axis")
    for k in (-140, -126, 120):
        x = in0[sl] * np.float32(2.0 ** k)
        assert (x != 0).sum() == 2 * len(x)  # nothing flushed
        np.testing.assert_array_equal(host_project(emu, x)[0], base[sl])
