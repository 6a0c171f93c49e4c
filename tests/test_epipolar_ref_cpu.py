"""Pins the float64 restatement of the epipolar residual (tests/epipolar_ref.py) and measures the two constants of its bounds.  CPU only.

  * values: against the reference's own outputs in tests/golden/fit.npz (tolerances of tests/test_oracle_golden.py) and against
    oracle.compute_epi_residual in float64 (1e-12 relative);
  * gradients: against float64 autograd of the oracle on every shared case of tests/epipolar_cases.py, 1e-10 relative per (layer, pair);
  * the constants: the oracle in torch float32 on the CPU, forward and autograd, on every shared case; the smallest c that holds it
    must be at most C_FWD_MEASURED / C_GRAD_MEASURED (a quarter of the bounds in use);
  * the inputs: at most 1 % of a case's points are flagged;
  * csrc/loss_tail_body.h under the row emulation (tests/emu) through the same check as the GPU entry points."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epipolar_cases as ec  # noqa: E402
import epipolar_ref as er  # noqa: E402
from test_emu_cpu import emu  # noqa: E402,F401  (the session fixture that builds the host emulation)

KINDS = ["general", "clean", "outlier40", "planar", "dense1000"]
T = torch.from_numpy


def test_values_match_the_references_own_outputs(oracle, golden):
    g = golden("fit")
    for kind in KINDS:
        p1, p2, F = g[f"{kind}_f32_pts1"], g[f"{kind}_f32_pts2"], g[f"{kind}_f32_out"]
        for key, c in (("epi_0p5", 0.5), ("epi_0p02", 0.02)):
            r = er.residual_ref(p1, p2, F, c)
            np.testing.assert_allclose(r.out, g[f"{kind}_f32_{key}"], atol=1e-6, rtol=1e-5)
            o = oracle.compute_epi_residual(T(p1).double(), T(p2).double(), T(F).double(), float(np.float32(c))).numpy()
            np.testing.assert_allclose(r.out, o, rtol=1e-12, atol=0)


def test_metrics_match_the_oracle(oracle):
    rng = np.random.default_rng(3)
    F = rng.standard_normal((3, 3, 3))
    X, Y = rng.standard_normal((3, 50, 2)), rng.standard_normal((3, 50, 2))
    Xh, Yh = rng.standard_normal((3, 50, 3)), rng.standard_normal((3, 50, 3))
    for homo, (x, y) in ((False, (X, Y)), (True, (Xh, Yh))):
        a = (T(F), T(x), T(y))
        np.testing.assert_allclose(er.sampson(F, x, y, homo), oracle.sampson_dist(*a, if_homo=homo).numpy(), rtol=1e-12)
        np.testing.assert_allclose(er.epi_distance(F, x, y, homo), torch.stack(oracle.epi_distance(*a, if_homo=homo)).numpy(), rtol=1e-12)
        for cl in (None, 0.3, 0.0):
            # the oracle's batched branch has eps = 1e-10 (utils_F.py:329); the restatement takes it as the float32 the kernel is given
            mine = er.sym_epi(F, x, y, homo, cl, eps=1e-10)
            np.testing.assert_allclose(mine, oracle.sym_epi_dist(*a, if_homo=homo, clamp_at=None if cl is None else float(np.float32(cl))).numpy(), rtol=1e-9)


def _torch_grad(r, case, dtype):
    """loss_sum [L,B] and d (sum g_ls loss_sum) / d F of oracle.compute_epi_residual in `dtype` on the restatement's own points."""
    oracle = __import__("importlib").import_module("oracle.deepf_oracle")
    x1, x2 = T(r.x1).to(dtype), T(r.x2).to(dtype)
    F = T(case.F).to(dtype).requires_grad_(True)
    outs = [oracle.compute_epi_residual(x1, x2, F[l], r.pt.clamp_at) for l in range(case.L)]
    per_point = torch.stack(outs)
    ls = per_point.sum(2)
    (ls * T(case.g_ls).to(dtype)).sum().backward()
    return per_point.detach().numpy().astype(np.float64), ls.detach().numpy().astype(np.float64), F.grad.numpy().astype(np.float64)


@pytest.fixture(scope="module")
def shared():
    out = []
    for (L, B, M, tf, cl, sp) in ec.shared_cases():
        case, clamp = ec.get(L, B, M, tf, cl, sp)
        out.append((case, ec.reference(case, clamp)))
    return out


def test_gradients_match_float64_autograd(oracle, shared):
    worst = 0.0
    for case, r in shared:
        _, ls, g = _torch_grad(r, case, torch.float64)
        np.testing.assert_allclose(r.loss_sum, ls, rtol=1e-12, atol=1e-300)
        mine = r.g_F(g_loss_sum=case.g_ls)
        scale = np.abs(g).max((2, 3))
        err = np.abs(mine - g).max((2, 3))
        live = scale > 0
        assert (err[~live] == 0).all()
        if live.any():
            worst = max(worst, (err[live] / scale[live]).max())
        # E and its adjoint: K^T T2^T F T1 K (train_good_utils.py:356-358)
        Fo = T(case.F).double().requires_grad_(True)
        T1, T2, K = (T(er.per_pair(a, case.B).copy()) for a in (case.T1, case.T2, case.K))
        E = K.transpose(1, 2) @ T2.transpose(1, 2) @ Fo @ T1 @ K
        np.testing.assert_allclose(r.E, E.detach().numpy(), rtol=1e-12, atol=1e-12 * np.abs(r.E).max())
        (E * T(case.g_E).double()).sum().backward()
        ge = r.g_F(g_E=case.g_E)
        np.testing.assert_allclose(ge, Fo.grad.numpy(), rtol=1e-10, atol=1e-12 * np.abs(ge).max())
    print(f"EPI restatement vs float64 autograd: {worst:.2e} per (layer, pair) (bound 1e-10)")
    assert worst <= 1e-10


def test_flagged_points_are_rare(shared):
    tot, n_near, n_sign = 0, 0, 0
    lo, hi = [10 ** 9, 10 ** 9], [0, 0]
    for case, r in shared:
        if case.special == "exact":
            near, sgn = r.flagged()
            assert sgn.mean() > 0.5  # the point of that case
            continue
        near, sgn = r.flagged()
        n = near.size
        assert (near | sgn).sum() <= 0.01 * n, (case.L, case.B, case.M, case.tform, r.pt.clamp_at, int(near.sum()), int(sgn.sum()), n)
        tot, n_near, n_sign = tot + n, n_near + int(near.sum()), n_sign + int(sgn.sum())
        lo = [min(lo[0], int(near.sum())), min(lo[1], int(sgn.sum()))]
        hi = [max(hi[0], int(near.sum())), max(hi[1], int(sgn.sum()))]
    print(f"EPI flagged: near-gate {lo[0]}..{hi[0]} and sign-uncertain {lo[1]}..{hi[1]} per case, {n_near} + {n_sign} of {tot} points")


def test_the_float32_oracle_sits_inside_a_quarter_of_the_bounds(shared):
    """Measures the two constants: the smallest c for which bound_fwd(c) holds the float32 oracle's per-point distances and per-pair
    sums, and the smallest for which bound_grad(c, G) holds its autograd (flagged points widened as everywhere)."""
    c_fwd, c_grad = 0.0, 0.0
    for case, r in shared:
        pp, ls, g = _torch_grad(r, case, torch.float32)
        unit = r.pt.bound_fwd(1.0)
        assert (pp[unit == 0] == r.pt.out[unit == 0]).all()  # an all-zero layer: exact
        q = lambda err, b: (err[b > 0] / b[b > 0]).max(initial=0.0)
        c_fwd = max(c_fwd, q(np.abs(pp - r.pt.out), unit), q(np.abs(ls - r.loss_sum), unit.sum(2)))
        if r.pt.clamp_at == 0.0:
            assert (ls == 0).all()
        G = np.abs(case.g_ls.astype(np.float64))
        widen = r.bound_grad(0.0, G)
        unit_g = r.bound_grad(1.0, G) - widen
        excess = np.maximum(np.abs(g - r.g_F(g_loss_sum=case.g_ls)) - widen, 0.0)
        if case.special == "exact":
            assert (np.abs(g) <= r.bound_contribution(G) * (1 + 1e-6)).all()
            continue
        assert (excess[unit_g == 0] == 0).all()
        c_grad = max(c_grad, (excess[unit_g > 0] / unit_g[unit_g > 0]).max(initial=0.0))
    print(f"EPI measured on the float32 oracle: c_fwd {c_fwd:.2f}, c_grad {c_grad:.2f}; in use {er.C_FWD} and {er.C_GRAD}")
    assert c_fwd <= er.C_FWD_MEASURED and c_grad <= er.C_GRAD_MEASURED
    assert er.C_FWD == 4 * er.C_FWD_MEASURED and er.C_GRAD == 4 * er.C_GRAD_MEASURED
    # the constants in the docstring are the measurement rounded up, not a looser guess
    assert c_fwd >= 0.8 * er.C_FWD_MEASURED - 0.1 and c_grad >= 0.8 * er.C_GRAD_MEASURED - 0.1


def _emu_tail(emu, case, clamp, coef_F, pose):
    I, P, F32 = ctypes.c_int, ctypes.c_void_p, ctypes.c_float
    emu.emu_loss_tail.restype = I
    emu.emu_loss_tail.argtypes = [P, I, I, P, P, I, P, P, P, I, F32, P, P, P, F32, F32, F32, F32, F32] + [P] * 9
    L, B, M = case.L, case.B, case.M
    t = lambda a: T(np.ascontiguousarray(a))
    T1 = t(er.per_pair(case.T1, B).astype(np.float32))
    T2 = t(er.per_pair(case.T2, B).astype(np.float32))
    F, K, v1, v2 = t(case.F), t(case.K), t(case.v1), t(case.v2)
    q, tg, R = t(case.q_gt), t(case.t_gt), t(case.R_gt)
    loss_sum, E = torch.zeros(L, B), torch.zeros(L, B, 3, 3)
    q_l2, t_l2, R_deg, t_deg = (torch.zeros(L, B) for _ in range(4))
    sel = torch.zeros(L, B, dtype=torch.int32)
    gF = torch.zeros(L, B, 3, 3)
    part = torch.zeros(B, 48, dtype=torch.float64)
    p = lambda x: x.data_ptr()
    rc = emu.emu_loss_tail(p(F), L, B, p(T1), p(T2), 9, p(K), p(v1), p(v2), M, clamp, p(q) if pose else None, p(tg), p(R), 10.0, 10.0,
                           coef_F, 0.7 if pose else 0.0, 1.3 if pose else 0.0, p(loss_sum), p(E), p(q_l2), p(t_l2), p(R_deg), p(t_deg),
                           p(sel), p(gF), p(part))
    assert rc == 0
    return loss_sum.numpy(), E.numpy(), gF.numpy()


@pytest.mark.parametrize("L,B,M", ec.EMU_SHAPES)
def test_loss_tail_body_on_the_host_within_the_bounds(emu, L, B, M):
    """tail_floss_row<IT> for every IT rung and both parities of L under the row emulation, T1 != T2 per pair: loss_sum, E and
    g_F = coef_F x the restatement's sums (no ground truth: no pose part); with ground truth, the F-loss part as the difference of
    two runs (coef_F = c and 0), one float32 rounding of the larger operand added to the bound."""
    case, clamp = ec.pick(L, B, M)
    r = ec.reference(case, clamp)
    coef = np.float32(0.37 / (L * B * M))
    ls, E, g = _emu_tail(emu, case, clamp, coef, pose=False)
    ec.check(f"emu tail {L},{B},{M}", r, loss_sum=ls, g_F=g, g_ref=r.g_F(g_loss_sum=float(coef)), g_bound=r.bound_grad(G=float(coef)), E=E)
    ls1, _, g1 = _emu_tail(emu, case, clamp, coef, pose=True)
    ls0, _, g0 = _emu_tail(emu, case, clamp, 0.0, pose=True)
    assert np.array_equal(ls1, ls) and np.array_equal(ls0, ls)
    extra = er.U32 * np.maximum(np.abs(g1), np.abs(g0))
    ec.check(f"emu tail+pose {L},{B},{M}", r, g_F=g1.astype(np.float64) - g0, g_ref=r.g_F(g_loss_sum=float(coef)),
             g_bound=r.bound_grad(G=float(coef)), extra_abs=extra)
