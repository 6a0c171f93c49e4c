"""Row-shared data arrives once per row, on the GPU: the backward fit with the forward's record, g_F and F_out in lane slices
(csrc/w8pt16_bwd_body.h) in every kernel family that shares the body.  References and bounds are the suite's own: float64 autograd of
the oracle through tests/fit_adjoint_cases.py.  The loss tail keeps its per-float loads of the virtual points (the wide-load variant
measured slower), so its code is the parent's; its test here only adds the shapes the suite did not have (M = 1, 4, 7,
L = 16, per-pair T1 / T2) against the unfused kernels (ops.floss, ops.pose_errors) at the tolerances of tests/test_api_path_gpu.py, and
point tensors that are not 16-byte aligned.  tests/test_row_shared_loads_cpu.py runs the same
bodies under the host emulation.  GPU box only."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fit_adjoint_cases as fac  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = float(fac.IMAGE_SIZE[0]), float(fac.IMAGE_SIZE[1])

# (B, N, row_per_pair): rows and workgroups past the end of the batch at IT 7; IT 1 and 2 with ragged padding; IT 8; IT 0 in the row
# kernel (forced) and the cooperative workgroup at the same shape
BWD_SHAPES = [(1, 100, False), (5, 100, False), (21, 100, False), (3, 9, False), (4, 16, False), (3, 17, False), (2, 128, False),
              (2, 300, True), (2, 300, False)]
# logits | plain weights, each with g_F alone (UP = false) and with g_residual and g_epi (pass A: F_out from the lanes)
BWD_VARIANTS = ["raw_logits_gF", "raw_logits_all", "homog_gF", "homog_all"]


def run_device(dfepe, case, row_per_pair=False, spoil=None):
    a = case.launch
    d = lambda t: None if t is None else t.to(DEV).contiguous()
    pts1, pts2, w = d(a["pts1"]), d(a["pts2"]), d(a["weights"])
    F, _res, _epi, save, w_out = dfepe.ops.w8pt_forward(pts1, pts2, w, a["raw"], W, H, 0.5, want_epi=True, want_save=True, logits=a["logits"],
                                                       row_per_pair=row_per_pair, extra_flags=a["flags"])
    if spoil is not None:
        spoil(save)
    out = dfepe.ops.w8pt_backward(pts1, pts2, w_out if a["logits"] else w, a["raw"], W, H, 0.5, save, F, d(a["gF"]), d(a["gRes"]), d(a["gEpi"]),
                                  logits=a["logits"], gW_extra=d(a["gW_extra"]), want_pts=a["want_pts"], row_per_pair=row_per_pair,
                                  extra_flags=a["flags"])
    torch.cuda.synchronize()
    gW, gP1, gP2 = out if a["want_pts"] else (out, None, None)
    return F, {"weights": gW, "pts1": gP1, "pts2": gP2}


@pytest.mark.parametrize("variant", BWD_VARIANTS)
@pytest.mark.parametrize("B,N,rpp", BWD_SHAPES)
def test_backward_with_sliced_record_vs_oracle_autograd(dfepe, B, N, rpp, variant):
    case = fac.make_case(B, N, 300 + N + B, variant)
    F, grads = run_device(dfepe, case, row_per_pair=rpp)
    fac.check(case, F, grads, tag="sliced")


@pytest.mark.parametrize("B,N,rpp", [(5, 100, False), (3, 17, False), (2, 300, True)])
def test_backward_point_gradients_with_sliced_record(dfepe, B, N, rpp):
    """PGRAD reads u3, v3, s3 and F_out again behind pass B: IT 7, 2 and 0."""
    case = fac.make_case(B, N, 300 + N + B, "raw_points")
    F, grads = run_device(dfepe, case, row_per_pair=rpp)
    fac.check(case, F, grads, tag="sliced-points")


@pytest.mark.parametrize("slot", [126, 127])
@pytest.mark.parametrize("B,N,rpp", [(21, 100, False), (2, 300, True), (2, 300, False)])
def test_backward_poisons_a_record_of_another_layout(dfepe, B, N, rpp, slot):
    """The layout mark (float 126) and the tag (127) are compared by lane 15 of the row, which broadcasts one verdict: a pair whose
    record carries another value in either place gets NaN in every entry, the other pairs what a clean launch gives them."""
    case = fac.make_case(B, N, 300 + N + B, "raw_logits_all")
    victim = B - 1

    def spoil(save):
        save[victim, slot] = 0.0

    _, clean = run_device(dfepe, case, row_per_pair=rpp)
    _, bad = run_device(dfepe, case, row_per_pair=rpp, spoil=spoil)
    assert torch.isfinite(clean["weights"]).all()
    assert torch.isnan(bad["weights"][victim]).all()
    assert torch.equal(bad["weights"][:victim], clean["weights"][:victim])


def test_deferred_head_step_gives_the_same_loss_scalars(dfepe):
    """w8pt16_bwd_head_kernel shares the body: one step at B = 21 (a workgroup with five pairs), L = 2 with the loss head riding on
    the first backward launch against the step that launches it on its own."""
    B, N, depth = 21, 100, 2
    sc = dfepe.pipeline.scene_to_device(dfepe.synth.make_scene(B, N, seed=9, outlier_ratio=0.2, depth_layers=depth), DEV)
    a = dfepe.pipeline.hot_path_step(sc, fac.IMAGE_SIZE, depth, 0.02, qt=True)
    b = dfepe.pipeline.hot_path_step(sc, fac.IMAGE_SIZE, depth, 0.02, qt=True, defer_loss_head=True)
    torch.cuda.synchronize()
    for k in ("loss", "loss_F", "loss_qt", "loss_layers", "packed"):
        assert torch.equal(a[k].detach(), b[k].detach()), k
    assert torch.equal(a["grad_logits"], b["grad_logits"]) and torch.isfinite(a["grad_logits"]).all()


# ---- the loss tail -----------------------------------------------------------------------------------------------------------------
def _shifted(t):
    """The same values one float further on: contiguous, but not at a multiple of 16 bytes."""
    buf = torch.empty(t.numel() + 1, device=t.device)
    assert buf.data_ptr() % 16 == 0
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


_TAIL_CACHE = {}


def _tail_case(dfepe, L, B, M):
    """Inputs of one tail launch and what the unfused kernels make of them (computed once per shape)."""
    key = (L, B, M)
    if key not in _TAIL_CACHE:
        d = dfepe.pipeline.scene_to_device(dfepe.synth.make_scene(B, 60, seed=7 + M + L, outlier_ratio=0.2, noise_px=0.5, depth_layers=1, M_virt=M), DEV)
        g = torch.Generator().manual_seed(5 + M)
        T = torch.tensor([[2.0 / W, 0.0, -1.0], [0.0, 2.0 / H, -1.0], [0.0, 0.0, 1.0]], device=DEV)
        Tinv = torch.linalg.inv(T.double())
        Fn = Tinv.T @ d["F_gt"].double() @ Tinv
        Fn = Fn / Fn.flatten(1).norm(dim=1)[:, None, None]
        Fl = torch.stack([Fn + 0.003 * (l + 1) * torch.randn(B, 3, 3, generator=g, dtype=torch.float64).to(DEV) for l in range(L)]).float().contiguous()
        c = dict(d=d, T=T, Fl=Fl, v1=d["pts1_virt_ori"].float().contiguous(), v2=d["pts2_virt_ori"].float().contiguous(),
                 q=d["qs_cam"].reshape(B, 4).float().contiguous(), t=d["ts_cam"].reshape(B, 3).float().contiguous(), R=d["R_gt"].float().contiguous(),
                 K=d["Ks"].float().contiguous())
        assert c["v1"].shape == (B, M, 3) and c["v1"].data_ptr() % 16 == 0 and c["v2"].data_ptr() % 16 == 0
        Fb = Fl.clone().requires_grad_(True)
        ls, E = dfepe.ops.floss(Fb, T, T, c["K"], c["v1"], c["v2"], 0.02)
        q, t, Rd, td, sel = dfepe.ops.pose_errors(E, d["qs_cam"], d["ts_cam"], d["R_gt"])
        bF, bq, bt, cq, ct = 0.7, 1.0, 0.1, 0.1, 0.5
        (bF * (ls / M).mean() + bq * q.clamp(max=cq).mean() + bt * t.clamp(max=ct).mean()).backward()
        c["ref"] = dict(loss_sum=ls.detach(), E=E.detach(), q_l2=q.detach(), t_l2=t.detach(), R_deg=Rd, t_deg=td, sel=sel, gF=Fb.grad)
        c["mix"] = (bF, bq, bt, cq, ct)
        _TAIL_CACHE[key] = c
    return _TAIL_CACHE[key]


def _launch_tail(dfepe, c, v1, v2, t_stride, jac):
    lib = dfepe._lib.lib()
    p = lambda x: None if x is None else x.data_ptr()
    Fl = c["Fl"]
    L, B, M = Fl.shape[0], Fl.shape[1], v1.shape[1]
    Tm = c["T"].contiguous() if t_stride == 0 else c["T"].expand(B, 3, 3).contiguous()
    o = dict(loss_sum=torch.zeros(L, B, device=DEV), E=torch.zeros(L, B, 3, 3, device=DEV), q_l2=torch.zeros(L, B, device=DEV),
             t_l2=torch.zeros(L, B, device=DEV), R_deg=torch.zeros(L, B, device=DEV), t_deg=torch.zeros(L, B, device=DEV),
             sel=torch.zeros(L, B, device=DEV, dtype=torch.int32))
    st = torch.cuda.current_stream().cuda_stream
    if jac:
        o["J"] = torch.zeros(L, B, 27, device=DEV)
        rc = lib.dfepe_loss_tail_jac(p(Fl), L, B, p(Tm), p(Tm), t_stride, p(c["K"]), p(v1), p(v2), M, 0.02, p(c["q"]), p(c["t"]), p(c["R"]), 1,
                                     p(o["loss_sum"]), p(o["E"]), p(o["q_l2"]), p(o["t_l2"]), p(o["R_deg"]), p(o["t_deg"]), p(o["sel"]), p(o["J"]), st)
    else:
        bF, bq, bt, cq, ct = c["mix"]
        o["gF"] = torch.zeros(L, B, 3, 3, device=DEV)
        o["packed"] = torch.zeros(L + 4, device=DEV, dtype=torch.float64)
        o["scalars"] = torch.zeros(L + 4, device=DEV)
        ws = torch.zeros((lib.dfepe_loss_tail_workspace_bytes(B) + 7) // 8, dtype=torch.float64, device=DEV)
        rc = lib.dfepe_loss_tail(p(Fl), L, B, p(Tm), p(Tm), t_stride, p(c["K"]), p(v1), p(v2), M, 0.02, p(c["q"]), p(c["t"]), p(c["R"]), cq, ct,
                                 bF, bq, bt, float(B), p(o["loss_sum"]), p(o["E"]), p(o["q_l2"]), p(o["t_l2"]), p(o["R_deg"]), p(o["t_deg"]),
                                 p(o["sel"]), p(o["gF"]), p(o["packed"]), p(o["scalars"]), p(ws), 0, st)
    torch.cuda.synchronize()
    return rc, o


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x.view(torch.int64) if x.dtype == torch.float64 else x


@pytest.mark.parametrize("jac", [False, True], ids=["tail", "jac"])
@pytest.mark.parametrize("t_stride", [0, 9])
@pytest.mark.parametrize("L,B,M", [(5, 17, 1), (1, 17, 7), (16, 17, 4)])
def test_tail_equals_the_unfused_kernels_wherever_the_points_lie(dfepe, L, B, M, t_stride, jac):
    """M = 1 and 7 (less than a row, no whole 16-byte unit) and M = 4 at L = 16 (F of every layer the tail can take), B = 17 (a second
    workgroup with one pair), T1 / T2 shared by the launch (t_stride 0) and per pair (9), dfepe_loss_tail and dfepe_loss_tail_jac.  At
    M = 4 a launch on point tensors moved by one float (no longer 16-byte aligned) gives every output bit for bit, and all agree with
    dfepe_floss_* / dfepe_pose_* as tests/test_api_path_gpu.py requires (E and sel equal; loss_sum rtol 2e-6, atol 1e-7; q_l2, t_l2 atol
    1e-7; R_deg atol 1e-6; gradients within 2e-5 of the largest entry)."""
    c = _tail_case(dfepe, L, B, M)
    rc, a = _launch_tail(dfepe, c, c["v1"], c["v2"], t_stride, jac)
    assert rc == 0
    runs = [a]
    if M % 4 == 0:
        for w1, w2 in ((_shifted(c["v1"]), _shifted(c["v2"])), (c["v1"], _shifted(c["v2"]))):
            rc, b = _launch_tail(dfepe, c, w1, w2, t_stride, jac)
            assert rc == 0
            for k in a:
                assert torch.equal(_bits(a[k]), _bits(b[k])), (k, "the outputs depend on where the point tensors lie")
            runs.append(b)
    r = c["ref"]
    for o in runs[:2]:
        assert torch.equal(o["E"], r["E"]) and torch.equal(o["sel"], r["sel"])
        np.testing.assert_allclose(o["loss_sum"].cpu().numpy(), r["loss_sum"].cpu().numpy(), rtol=2e-6, atol=1e-7)
        np.testing.assert_allclose(o["q_l2"].cpu().numpy(), r["q_l2"].cpu().numpy(), atol=1e-7)
        np.testing.assert_allclose(o["t_l2"].cpu().numpy(), r["t_l2"].cpu().numpy(), atol=1e-7)
        np.testing.assert_allclose(o["R_deg"].cpu().numpy(), r["R_deg"].cpu().numpy(), atol=1e-6)
        bF, bq, bt, cq, ct = c["mix"]
        if jac:  # the caller's own mixing of the three Jacobians (clamps pass the gradient up to and including the bound)
            J = o["J"].double().view(L, B, 3, 3, 3)
            gq = (bq / (L * B)) * (r["q_l2"] <= cq).double()
            gt = (bt / (L * B)) * (r["t_l2"] <= ct).double()
            gF = (bF / (L * B * M)) * J[:, :, 0] + gq[:, :, None, None] * J[:, :, 1] + gt[:, :, None, None] * J[:, :, 2]
        else:
            gF = o["gF"].double()
        scale = float(r["gF"].abs().max())
        e = float((gF - r["gF"].double()).abs().max())
        print(f"TAIL L={L} B={B} M={M} t_stride={t_stride} jac={jac}: |g_F - unfused| {e:.3e} of {scale:.3e} (bound 2e-5)")
        assert e < 2e-5 * scale
