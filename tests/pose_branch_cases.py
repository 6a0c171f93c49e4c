"""Large-rotation cases of the pose loss: essential matrices whose decomposition lands on every branch of the trace-method quaternion
(csrc/pose_math.h: rot_to_quat, branches 0..3 and the sign flip q0 >= 0), with the float64 yardsticks of oracle.rt_loss.  Shared by the
host test (tests/test_emu_cpu.py, emulated loss tail) and the GPU tests (tests/test_pose_branches_gpu.py: pose.hip, loss_tail_jac,
dfepe_loss_tail).  Scenes of synth.make_scene rotate by ~0.03 rad: branch 3, no flip, every time."""
import functools
import importlib

import numpy as np
import torch

N_DIRECTIONS = 4
FD_STEP = 1e-6


def _rodrigues(axis, angle):
    k = axis / np.linalg.norm(axis)
    Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(angle) * Kx + (1.0 - np.cos(angle)) * (Kx @ Kx)


def _skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def _inputs():
    """Deterministic (numpy.random.default_rng(0)).  For each of the axes x, y, z and each angle in 100, 130, 150, 170 degrees three
    rotations about axis + 0.15 N(0, I), the sign of the axis alternating from case to case; six rotations of 1..60 degrees about
    random axes: 42 cases.  t a random unit vector; E = ([t]x R)^T / |.| (get_Rt_loss decomposes E^T), as it is (layer 0) and with
    0.01 N(0, 1) on every entry (layer 1), rounded to fp32.  Ground truth: R_gt = (3 degrees about a random axis) R, q_gt its
    trace-method quaternion, t_gt = t + 0.05 N(0, I); delta with inv(delta)[:3, :3] = R_gt."""
    g = np.random.default_rng(0)
    Rs, sign = [], 1.0
    for ax in range(3):
        for deg in (100.0, 130.0, 150.0, 170.0):
            for _ in range(3):
                axis = sign * np.eye(3)[ax] + 0.15 * g.standard_normal(3)
                sign = -sign
                Rs.append(_rodrigues(axis, np.radians(deg)))
    for _ in range(6):
        Rs.append(_rodrigues(g.standard_normal(3), np.radians(g.uniform(1.0, 60.0))))
    B = len(Rs)
    E = np.zeros((2, B, 3, 3))
    R_gt, t_gt = np.zeros((B, 3, 3)), np.zeros((B, 3))
    for b, R in enumerate(Rs):
        t = g.standard_normal(3)
        t /= np.linalg.norm(t)
        e = (_skew(t) @ R).T
        e /= np.linalg.norm(e)
        E[0, b] = e
        E[1, b] = e + 0.01 * g.standard_normal((3, 3))
        R_gt[b] = _rodrigues(g.standard_normal(3), np.radians(3.0)) @ R
        t_gt[b] = t + 0.05 * g.standard_normal(3)
    return E.astype(np.float32), R_gt, t_gt


def branch_of(R):
    """(branch, margin of the predicates on the way to it, sign flip) of the trace-method quaternion of R, as oracle.R_to_q and
    pose_math.h choose them (m = R^T has R's diagonal)."""
    d0, d1, d2 = R[0, 0], R[1, 1], R[2, 2]
    m = R.T
    if d2 < 0:
        br, second = (0, d0 - d1) if d0 > d1 else (1, d0 - d1)
        q0 = (m[1, 2] - m[2, 1]) if br == 0 else (m[2, 0] - m[0, 2])
    else:
        br, second = (2, d0 + d1) if d0 < -d1 else (3, d0 + d1)
        q0 = (m[0, 1] - m[1, 0]) if br == 2 else 1.0
    return br, min(abs(d2), abs(second)), bool(q0 < 0)


class PoseCases:
    pass


@functools.lru_cache(maxsize=None)
def make_cases():
    """The inputs (fp32 tensors, as the kernels see them), the float64 reference and its directional derivatives, and the conditions on
    the reference alone, asserted here before anyone compares anything: computed once per process and shared."""
    dfepe = importlib.import_module("pytorch-deepfepe_amd")
    oracle = importlib.import_module("oracle.deepf_oracle")
    E32, R_gt, t_gt = _inputs()
    L, B = E32.shape[:2]
    c = PoseCases()
    c.L, c.B = L, B
    c.E = torch.from_numpy(E32).contiguous()                                   # [L,B,3,3] fp32
    q_gt = dfepe.synth.rotation_to_quaternion_np(R_gt)                          # [B,4], q0 >= 0
    c.q_gt = torch.from_numpy(q_gt.astype(np.float32)).contiguous()
    c.t_gt = torch.from_numpy(t_gt.astype(np.float32)).contiguous()
    c.R_gt = torch.from_numpy(R_gt.astype(np.float32)).contiguous()
    # the reference sees the same fp32-representable numbers
    q64, t64 = c.q_gt.double().reshape(B, 4, 1), c.t_gt.double().reshape(B, 3, 1)
    delta = torch.eye(4, dtype=torch.float64).repeat(B, 1, 1)
    delta[:, :3, :3] = c.R_gt.double().transpose(1, 2)  # inv(delta)[:3, :3] = R_gt (the translation part is not read)
    E64 = c.E.double()

    def ref(Ex):
        return oracle.rt_loss([Ex[l] for l in range(L)], delta, q64, t64)

    r = ref(E64)
    c.q_l2, c.t_l2 = r["q_l2"].numpy(), r["t_l2"].numpy()
    c.R_deg, c.t_deg = r["R_deg"], r["t_deg"]
    # ---- conditions, on the reference alone ------------------------------------------------------------------------------
    branches, flips, margin, qgap, tgap = np.zeros(4, int), 0, np.inf, np.inf, np.inf
    n_sel = 0
    for l in range(L):
        for b in range(B):
            Rc, tc = oracle.get_M2s(E64[l, b].T)
            qe = [float((oracle.R_to_q(R) - q64[b]).norm()) for R in Rc]
            tn = t64[b] / t64[b].norm()
            te = [float((t - tn).norm()) for t in tc]
            qi = int(r["sel"][l, b, 0])
            assert qi == (0 if qe[0] < qe[1] else 1)
            br, mg, flip = branch_of(Rc[qi].numpy())
            if l == 0:
                branches[br] += 1
                flips += int(flip)
                n_sel += 1
            margin = min(margin, mg)
            qgap, tgap = min(qgap, abs(qe[0] - qe[1])), min(tgap, abs(te[0] - te[1]))
    c.branches, c.flips, c.margin, c.qgap, c.tgap = branches, flips, margin, qgap, tgap
    assert n_sel == 42
    assert (branches[:3] >= 10).all() and branches[3] >= 6, branches
    assert flips >= 15, flips
    assert margin >= 0.05, margin
    assert qgap >= 0.5 and tgap >= 0.5, (qgap, tgap)
    # ---- central differences of the float64 oracle in four random directions: d q_l2, d t_l2 per (direction, layer, pair) -----------
    gd = torch.Generator().manual_seed(5)
    c.D = torch.randn(N_DIRECTIONS, L, B, 3, 3, generator=gd, dtype=torch.float64)
    c.dq = np.zeros((N_DIRECTIONS, L, B))
    c.dt = np.zeros((N_DIRECTIONS, L, B))
    for k in range(N_DIRECTIONS):
        p, m = ref(E64 + FD_STEP * c.D[k]), ref(E64 - FD_STEP * c.D[k])
        c.dq[k] = (p["q_l2"].numpy() - m["q_l2"].numpy()) / (2 * FD_STEP)
        c.dt[k] = (p["t_l2"].numpy() - m["t_l2"].numpy()) / (2 * FD_STEP)
    c.GQ = torch.rand(L, B, generator=gd) + 0.5
    c.GT = torch.rand(L, B, generator=gd) + 0.5
    return c


def check_forward(c, q_l2, t_l2, R_deg, t_deg, tag=""):
    """The four per-(layer, pair) errors against oracle.rt_loss in float64, with the suite's bounds: atol 2e-6 / rtol 1e-5 for the L2
    errors, 2e-3 and 2e-2 degrees for the angles.  `sel` is not compared (the candidate order follows the SVD's sign gauge)."""
    f = lambda t: np.asarray(t.detach().cpu() if hasattr(t, "detach") else t, dtype=np.float64)
    q_l2, t_l2, R_deg, t_deg = f(q_l2), f(t_l2), f(R_deg), f(t_deg)
    print(f"POSEBR {tag} |q_l2 - ref| {np.abs(q_l2 - c.q_l2).max():.2e}  |t_l2 - ref| {np.abs(t_l2 - c.t_l2).max():.2e}  "
          f"R_deg {np.abs(R_deg - c.R_deg).max():.2e}  t_deg {np.abs(t_deg - c.t_deg).max():.2e}")
    np.testing.assert_allclose(q_l2, c.q_l2, atol=2e-6, rtol=1e-5)
    np.testing.assert_allclose(t_l2, c.t_l2, atol=2e-6, rtol=1e-5)
    np.testing.assert_allclose(R_deg, c.R_deg, atol=2e-3, rtol=0)
    np.testing.assert_allclose(t_deg, c.t_deg, atol=2e-2, rtol=0)


def check_adjoint(c, g_E, GQ, GT, tag=""):
    """<g_E, D> against the central differences of sum GQ q_l2 + sum GT t_l2 of the float64 oracle, per (direction, layer, pair),
    relative to the largest derivative: <= 2e-4 (the project's bound for the pose adjoint at well-separated matrices; central
    differences have no singular-value-gap problem, so it holds at exact essential matrices too).  GQ, GT: [L,B] or scalars."""
    g = g_E.detach().cpu().double()
    ana = (g[None] * c.D).sum(dim=(3, 4)).numpy()
    GQ = np.broadcast_to(np.asarray(GQ, dtype=np.float64), (c.L, c.B))
    GT = np.broadcast_to(np.asarray(GT, dtype=np.float64), (c.L, c.B))
    num = GQ[None] * c.dq + GT[None] * c.dt
    err = np.abs(ana - num).max() / np.abs(num).max()
    print(f"POSEBR {tag} directional derivative vs central differences: {err:.2e} (bound 2e-4)")
    assert np.isfinite(ana).all()
    assert err <= 2e-4, err
    return err
