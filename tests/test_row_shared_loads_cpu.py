"""Row-shared data arrives once per row: the backward fit reads the forward's record (and g_F, F_out) in lane slices and broadcasts
the pieces in-row (csrc/w8pt16_bwd_body.h, rec_f / rec_d in csrc/w8pt16_body.h).  Here: the SAME body under the host emulation
(tests/emu/), held to the references and bounds the suite already has (tests/fit_adjoint_cases.py) at the shapes where the new loads can
go wrong: rows with padding lanes, IT 1, 2, 7, 8 and 0, with and without pass A, with point gradients, and a record of another layout.
The loss tail keeps its per-float loads of the virtual points (the wide-load variant measured slower), so its code is the
parent's; its test here only adds shapes the suite did not have (M = 1, 4, 7, L = 16, per-pair T1 / T2) and unaligned point tensors.  tests/test_row_shared_loads_gpu.py runs the builds."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fit_adjoint_cases as fac  # noqa: E402
from test_emu_cpu import IMAGE_SIZE, LOGITS, RAW, emu, emu_bwd, emu_fwd, relerr  # noqa: E402,F401  (emu: the session fixture)

BWD_SHAPES = [(1, 100), (5, 100), (3, 9), (4, 16), (3, 17), (2, 128), (2, 300)]  # IT 7 | 7 | 1 | 1 | 2 | 8 | 0
BWD_VARIANTS = ["raw_logits_gF", "raw_logits_all", "homog_gF", "homog_all", "raw_points"]


def _flags(a):
    return (RAW if a["raw"] else 0) | (LOGITS if a["logits"] else 0) | a["flags"]


def _emu_case(emu, case, spoil=None):
    a = case.launch
    F, _res, _epi, save, wout = emu_fwd(emu, a["pts1"], a["pts2"], a["weights"], _flags(a))
    if spoil is not None:
        spoil(save)
    gW, gP1, gP2 = emu_bwd(emu, a["pts1"], a["pts2"], wout if a["logits"] else a["weights"], _flags(a), save, F, a["gF"], a["gRes"], a["gEpi"],
                           want_pts=a["want_pts"], gW_extra=a["gW_extra"])
    return F, {"weights": gW, "pts1": gP1, "pts2": gP2}


@pytest.mark.parametrize("variant", BWD_VARIANTS)
@pytest.mark.parametrize("B,N", BWD_SHAPES)
def test_backward_body_with_sliced_record_vs_oracle_autograd(emu, B, N, variant):
    """Logits and plain weights, g_F alone and with g_residual / g_epi (pass A reads F_out from the lanes), point gradients: float64
    autograd of the oracle at the bounds of fit_adjoint_cases."""
    case = fac.make_case(B, N, 300 + N + B, variant)
    F, grads = _emu_case(emu, case)
    fac.check(case, F, grads, tag="emu-sliced")


@pytest.mark.parametrize("slot", [126, 127])
def test_backward_body_poisons_a_record_of_another_layout(emu, slot):
    """Lane 15 holds the layout mark (float 126) and the tag (127), compares both and the row takes its verdict: a pair whose record
    carries another value in either place gets NaN in every gradient entry, its neighbours get what they get from a clean run."""
    case = fac.make_case(3, 100, 77, "raw_logits_all")

    def spoil(save):
        save[1, slot] = 0.0

    _, clean = _emu_case(emu, case)
    _, bad = _emu_case(emu, case, spoil)
    assert torch.isnan(bad["weights"][1]).all()
    assert torch.equal(bad["weights"][[0, 2]], clean["weights"][[0, 2]]) and torch.isfinite(clean["weights"]).all()


# ---- the loss tail -----------------------------------------------------------------------------------------------------------------
def _tail_inputs(dfepe, oracle, L, B, M, seed):
    sc = dfepe.synth.make_scene(B, 50, seed=seed)
    v1, v2 = sc["pts1_virt_ori"], sc["pts2_virt_ori"]
    rep = (M + v1.shape[1] - 1) // v1.shape[1]
    v1, v2 = v1.repeat(1, rep, 1)[:, :M].contiguous(), v2.repeat(1, rep, 1)[:, :M].contiguous()
    g = torch.Generator().manual_seed(seed)
    T = oracle.hw_matrix(IMAGE_SIZE, torch.float64)
    Tinv = torch.linalg.inv(T)
    Fn = Tinv.T @ sc["F_gt"].double() @ Tinv
    Fn = Fn / Fn.flatten(1).norm(dim=1)[:, None, None]
    Fl = torch.stack([Fn + 0.003 * (l + 1) * torch.randn(B, 3, 3, generator=g, dtype=torch.float64) for l in range(L)]).float().contiguous()
    return sc, v1, v2, T, Fl


def _shifted(t):
    """The same values one float further on: a contiguous tensor whose address is not a multiple of 16."""
    buf = torch.empty(t.numel() + 1)
    assert buf.data_ptr() % 16 == 0
    out = buf[1:].view(t.shape)
    out.copy_(t)
    return out


def _emu_tail(emu, Fl, T1, T2, t_stride, Ks, v1, v2, q_gt, t_gt, R_gt, coefs, clamps=(0.02, 0.1, 0.5)):
    I, P, F32 = ctypes.c_int, ctypes.c_void_p, ctypes.c_float
    emu.emu_loss_tail.restype = I
    emu.emu_loss_tail.argtypes = [P, I, I, P, P, I, P, P, P, I, F32, P, P, P, F32, F32, F32, F32, F32] + [P] * 9
    L, B, M = Fl.shape[0], Fl.shape[1], v1.shape[1]
    out = {"loss_sum": torch.zeros(L, B), "E": torch.zeros(L, B, 3, 3), "q_l2": torch.zeros(L, B), "t_l2": torch.zeros(L, B),
           "R_deg": torch.zeros(L, B), "t_deg": torch.zeros(L, B), "sel": torch.zeros(L, B, dtype=torch.int32), "gF": torch.zeros(L, B, 3, 3),
           "part": torch.zeros(B, 48, dtype=torch.float64)}
    p = lambda x: x.data_ptr()
    rc = emu.emu_loss_tail(p(Fl), L, B, p(T1), p(T2), t_stride, p(Ks), p(v1), p(v2), M, clamps[0], p(q_gt), p(t_gt), p(R_gt), clamps[1], clamps[2],
                           coefs[0], coefs[1], coefs[2], *(p(out[k]) for k in ("loss_sum", "E", "q_l2", "t_l2", "R_deg", "t_deg", "sel", "gF", "part")))
    assert rc == 0
    return out


@pytest.mark.parametrize("t_stride", [0, 9])
@pytest.mark.parametrize("L,B,M", [(5, 2, 1), (1, 3, 7), (16, 2, 4)])
def test_tail_body_vs_oracle_wherever_the_points_lie(emu, dfepe, oracle, L, B, M, t_stride):
    """M = 1 and 7 (less than a row) and M = 4 at L = 16, T1 / T2 shared by the launch and per pair: every output against the oracle
    (bounds of test_loss_tail_body_vs_oracle); at M = 4 the same launch on point tensors moved by one float must give every output
    bit for bit -- where the points lie changes no number."""
    sc, v1, v2, T, Fl = _tail_inputs(dfepe, oracle, L, B, M, seed=11 + L + M)
    assert v1.data_ptr() % 16 == 0 and v2.data_ptr() % 16 == 0
    Ks = sc["Ks"].contiguous()
    q_gt, t_gt = sc["qs_cam"].reshape(B, 4).contiguous(), sc["ts_cam"].reshape(B, 3).contiguous()
    R_gt = sc["delta_Rtijs_4_4"][:, :3, :3].transpose(1, 2).contiguous()
    Tf = T.float().contiguous() if t_stride == 0 else T.float().expand(B, 3, 3).contiguous()
    clamp, cq, ct, bF, bq, bt = 0.02, 0.1, 0.5, 0.7, 1.0, 0.1
    coefs = (bF / (L * B * M), bq / (L * B), bt / (L * B))
    r = _emu_tail(emu, Fl, Tf, Tf, t_stride, Ks, v1, v2, q_gt, t_gt, R_gt, coefs)
    if M % 4 == 0:
        for w1, w2 in ((_shifted(v1), _shifted(v2)), (v1, _shifted(v2))):
            s = _emu_tail(emu, Fl, Tf, Tf, t_stride, Ks, w1, w2, q_gt, t_gt, R_gt, coefs)
            for k in r:
                assert torch.equal(r[k].view(torch.int32) if r[k].dtype == torch.float32 else r[k], s[k].view(torch.int32) if s[k].dtype == torch.float32 else s[k]), k
    Fo = Fl.double().clone().requires_grad_(True)
    outs = {"T1": T.expand(B, 3, 3), "T2": T.expand(B, 3, 3), "out_layers": [Fo[l] for l in range(L)], "F_est": Fo[-1],
            "epi_res_layers": [], "weights_layers": []}
    losses, _, _, E_layers = oracle.f_loss(outs, v1.double(), v2.double(), Ks.double(), L, clamp)
    assert relerr(r["loss_sum"].numpy(), (losses["loss_per_pair"] * M).detach().numpy()) < 2e-5
    assert relerr(r["E"].numpy(), torch.stack(E_layers).detach().numpy()) < 2e-6
    pose = oracle.rt_loss(E_layers, sc["delta_Rtijs_4_4"].double(), sc["qs_cam"].double(), sc["ts_cam"].double())
    np.testing.assert_allclose(r["q_l2"].numpy(), pose["q_l2"].detach().numpy(), atol=2e-6, rtol=1e-5)
    np.testing.assert_allclose(r["t_l2"].numpy(), pose["t_l2"].detach().numpy(), atol=2e-6, rtol=1e-5)
    (bF * losses["loss_F"] + oracle.qt_training_loss(pose["q_l2"], pose["t_l2"], cq, ct, bq, bt)).backward()
    assert relerr(r["gF"].numpy(), Fo.grad.numpy()) < 3e-4
