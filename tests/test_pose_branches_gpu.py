"""The pose errors and their adjoint (csrc/pose_math.h) on all four branches of the trace-method quaternion and with the sign flip
q0 >= 0, through the three GPU entry points that use them: ops.pose_errors (pose.hip), ops.loss_tail_jac (loss_tail_jac +
loss_tail_bwd) and the one-launch dfepe_loss_tail of the captured step.  Cases, float64 yardsticks and bounds:
tests/pose_branch_cases.py (42 rotations of 100..170 degrees about x, y, z and 1..60 degrees about random axes; every scene of
synth.make_scene stays on branch 3 without the flip).  The F-taking entry points get T = K = I, so E = F.  GPU box only.

Measured on an MI355X, all three entry points alike: |q_l2 - ref| <= 1.8e-9, |t_l2 - ref| <= 7.5e-9, R_deg within 2.9e-7 degrees, t_deg
within 3.2e-7 degrees; directional derivatives within 4.0e-8 (pose_errors), 6.7e-8 (loss_tail_jac), 8.9e-8 (dfepe_loss_tail) of the largest
central difference; gradients of the three within 1.2e-7 of each other."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_branch_cases as pbc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COEF_Q, COEF_T = 0.7, 1.3  # balance_q, balance_t of the one-launch tail; its per-entry coefficients are these / (L B)
M_VIRT = 8


def virtual_points(B):
    g = torch.Generator().manual_seed(9)
    mk = lambda: torch.cat((torch.randn(B, M_VIRT, 2, generator=g), torch.ones(B, M_VIRT, 1)), 2).contiguous().to(DEV)
    return mk(), mk()


def run_pose_errors(dfepe, c, GQ, GT):
    E = c.E.to(DEV).requires_grad_(True)
    q_l2, t_l2, R_deg, t_deg, _sel = dfepe.ops.pose_errors(E, c.q_gt.to(DEV), c.t_gt.to(DEV), c.R_gt.to(DEV))
    ((q_l2 * GQ.to(DEV)).sum() + (t_l2 * GT.to(DEV)).sum()).backward()
    return [t.detach() for t in (q_l2, t_l2, R_deg, t_deg)], E.grad


def run_tail_jac(dfepe, c, GQ, GT):
    F = c.E.to(DEV).requires_grad_(True)
    eye = torch.eye(3, device=DEV)
    v1, v2 = virtual_points(c.B)
    r = dfepe.ops.loss_tail_jac(F, eye, eye, eye.repeat(c.B, 1, 1), v1, v2, 0.02, c.q_gt.to(DEV), c.t_gt.to(DEV), c.R_gt.to(DEV))
    assert torch.equal(r["E_layers"].detach(), c.E.to(DEV))  # T = K = I: what is decomposed is what was given
    ((r["q_l2"] * GQ.to(DEV)).sum() + (r["t_l2"] * GT.to(DEV)).sum()).backward()
    return [r["q_l2"].detach(), r["t_l2"].detach(), r["ang"][0], r["ang"][1]], F.grad


def run_one_launch_tail(dfepe, c):
    """dfepe_loss_tail as pipeline.hot_path_fused calls it: balance_F = 0, clamps of 10 (nothing gated), unit upstream.
    Its gradient is that of COEF_Q mean(q_l2) + COEF_T mean(t_l2)."""
    lib = dfepe._lib.lib()
    ops = dfepe.ops
    L, B = c.L, c.B
    F = c.E.to(DEV).contiguous()
    eye = torch.eye(3, device=DEV)
    Ks = eye.repeat(B, 1, 1).contiguous()
    v1, v2 = virtual_points(B)
    q_gt, t_gt, R_gt = c.q_gt.to(DEV), c.t_gt.to(DEV), c.R_gt.to(DEV)
    loss_sum, E = torch.empty(L, B, device=DEV), torch.empty(L, B, 3, 3, device=DEV)
    q_l2, t_l2, R_deg, t_deg = (torch.empty(L, B, device=DEV) for _ in range(4))
    sel = torch.empty(L, B, device=DEV, dtype=torch.int32)
    gF = torch.empty(L, B, 3, 3, device=DEV)
    packed = torch.empty(L + 4, device=DEV, dtype=torch.float64)
    scalars = torch.empty(4 + L, device=DEV)
    ws = dfepe.pipeline._tail_workspace(torch.device(DEV), B)
    with ops._on(F.device):
        rc = lib.dfepe_loss_tail(F.data_ptr(), L, B, eye.data_ptr(), eye.data_ptr(), 0, Ks.data_ptr(), v1.data_ptr(), v2.data_ptr(), M_VIRT,
                                 0.02, q_gt.data_ptr(), t_gt.data_ptr(), R_gt.data_ptr(), 10.0, 10.0, 0.0, COEF_Q, COEF_T, float(B),
                                 loss_sum.data_ptr(), E.data_ptr(), q_l2.data_ptr(), t_l2.data_ptr(), R_deg.data_ptr(), t_deg.data_ptr(),
                                 sel.data_ptr(), gF.data_ptr(), packed.data_ptr(), scalars.data_ptr(), ws.data_ptr(), 0, ops._stream())
    dfepe._lib.check(rc, "dfepe_loss_tail")
    torch.cuda.synchronize()
    assert torch.equal(E, F)
    # the loss the head reports is the one whose gradient g_F is
    want = COEF_Q * q_l2.double().mean() + COEF_T * t_l2.double().mean()
    np.testing.assert_allclose(scalars[0].item(), want.item(), rtol=1e-6)
    return [q_l2, t_l2, R_deg, t_deg], gF


@pytest.fixture(scope="module")
def cases():
    return pbc.make_cases()


def test_pose_errors_on_every_quaternion_branch(dfepe, cases):
    """pose.hip: forward against oracle.rt_loss (float64), backward with per-entry GQ / GT against central differences of it.

    Measured on an MI355X: forward as in the module docstring, adjoint 4.0e-8 (bound 2e-4)."""
    c = cases
    fwd, gE = run_pose_errors(dfepe, c, c.GQ, c.GT)
    pbc.check_forward(c, *fwd, tag="pose_errors")
    pbc.check_adjoint(c, gE, c.GQ.numpy(), c.GT.numpy(), tag="pose_errors")


def test_loss_tail_jac_on_every_quaternion_branch(dfepe, cases):
    """loss_tail_jac + loss_tail_bwd with ground truth, per-entry GQ / GT.

    Measured on an MI355X: forward as in the module docstring, adjoint 6.7e-8 (bound 2e-4)."""
    c = cases
    fwd, gF = run_tail_jac(dfepe, c, c.GQ, c.GT)
    pbc.check_forward(c, *fwd, tag="loss_tail_jac")
    pbc.check_adjoint(c, gF, c.GQ.numpy(), c.GT.numpy(), tag="loss_tail_jac")


def test_one_launch_loss_tail_on_every_quaternion_branch(dfepe, cases):
    """dfepe_loss_tail through the C ABI, with the arguments pipeline.hot_path_fused gives it.

    Measured on an MI355X: forward as in the module docstring, adjoint 8.9e-8 (bound 2e-4)."""
    c = cases
    fwd, gF = run_one_launch_tail(dfepe, c)
    pbc.check_forward(c, *fwd, tag="loss_tail")
    n = float(c.L * c.B)
    pbc.check_adjoint(c, gF, COEF_Q / n, COEF_T / n, tag="loss_tail")


def test_three_entry_points_agree_on_every_quaternion_branch(dfepe, cases):
    """The three run the same pose_math.h in float64 on the same fp32 matrix and round their results to fp32 once, so the forward
    values agree to a few ulp (rtol 1e-6; 1e-6 degrees absolute where an angle is near 0).  The gradients pass through different
    fp32 stages -- pose.hip writes the adjoint directly, loss_tail_bwd combines two stored fp32 Jacobians with fp32 coefficients, the
    one-launch tail applies its coefficients before the one rounding: <= 3 roundings of 2^-24 on either side of the larger of the
    two terms, which cancellation between the q and the t term can raise relative to their sum: 1e-5 of the largest entry of each
    (layer, pair).  Measured on an MI355X: 1.2e-7 for both pairs of entry points."""
    c = cases
    n = float(c.L * c.B)
    a_f, a_g = run_pose_errors(dfepe, c, c.GQ, c.GT)
    b_f, b_g = run_tail_jac(dfepe, c, c.GQ, c.GT)
    u = torch.ones(c.L, c.B)
    c_f, c_g = run_pose_errors(dfepe, c, u * (COEF_Q / n), u * (COEF_T / n))
    d_f, d_g = run_one_launch_tail(dfepe, c)
    for name, x, y, z in zip(("q_l2", "t_l2", "R_deg", "t_deg"), a_f, b_f, d_f):
        atol = 1e-6 if name.endswith("deg") else 1e-7
        np.testing.assert_allclose(y.cpu().numpy(), x.cpu().numpy(), rtol=1e-6, atol=atol, err_msg=name)
        np.testing.assert_allclose(z.cpu().numpy(), x.cpu().numpy(), rtol=1e-6, atol=atol, err_msg=name)

    def per_pair(x, y):
        x, y = x.double().cpu().flatten(2), y.double().cpu().flatten(2)
        return ((x - y).abs().amax(2) / y.abs().amax(2)).max().item()

    e1, e2 = per_pair(b_g, a_g), per_pair(d_g, c_g)
    print(f"POSEBR agree: loss_tail_jac vs pose_errors {e1:.2e}, loss_tail vs pose_errors {e2:.2e} (bound 1e-5)")
    assert e1 < 1e-5 and e2 < 1e-5
