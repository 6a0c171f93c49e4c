"""The sample-loss branch on the GPU, stage by stage through the checks of tests/sample_loss_cases.py (every stage is fed what the
device wrote before it), then through autograd, then captured in one hipGraph.  Shapes: the smallest at which each kernel can go
wrong (the lists are in sample_loss_cases.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fit_adjoint_cases as fac  # noqa: E402
import sample_loss_cases as sc  # noqa: E402
import sample_loss_ref as slr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _draw(dfepe, case, **over):
    c = dict(case, **over)
    ctr = None if c["counter"] is None else torch.tensor([c["counter"]], dtype=torch.uint32).to(DEV)
    idx, fb = dfepe.ops.sample_multisets(_t(c["weights"]), c["H"], c["K"], seed=c["seed"], offset=c["offset"], counter=ctr, n_valid=_t(c["n_valid"]),
                                         B=c["B"], N=c["N"], device=DEV, want_fallback=True)
    return idx.cpu().numpy(), fb.cpu().numpy()


def test_draw_equals_the_restatement(dfepe):
    chunk = dfepe._lib.lib().dfepe_sampler_scan_chunk()
    for case in sc.draw_cases(chunk):
        sc.check_draw(*_draw(dfepe, case), case)


def test_a_set_is_the_same_in_a_larger_batch_and_from_run_to_run(dfepe):
    w = sc._weights(4, 70, 5)
    base = dict(B=4, N=70, H=100, K=20, weights=w, n_valid=None, seed=9, offset=2, counter=5)
    big, _ = _draw(dfepe, base)
    again, _ = _draw(dfepe, base)
    small, _ = _draw(dfepe, base, B=3, H=65, weights=w[:3].copy())
    assert (big == again).all() and (big[:3, :65] == small).all()
    moved, _ = _draw(dfepe, base, offset=7, counter=None)  # offset + counter is what counts
    assert (moved == big).all()


def test_topk_is_the_rule(dfepe):
    for case in sc.topk_cases():
        idx, values = dfepe.ops.topk_select(_t(case["x"]), case["K"], _t(case["n_valid"]), want_values=True)
        sc.check_topk(idx.cpu().numpy(), case, values.cpu().numpy())


def test_gather_and_accu(dfepe):
    for tag, case in sc.gather_cases():
        out = dfepe.ops.sample_gather(_t(case["pts1"]), _t(case["pts2"]), _t(case["weights"]), _t(case["idx"]))
        sc.check_gather(*(o.cpu().numpy() for o in out), case, tag)


def test_fits_of_the_gathered_sets_and_their_adjoint(dfepe):
    ops = dfepe.ops
    for case in sc.fit_cases():
        tag = f"B={case['B']} N={case['N']} H={case['H']}"
        p1, p2, w = _t(case["pts1"]), _t(case["pts2"]), _t(case["weights"]).requires_grad_(True)
        idx = _t(case["idx"])
        g1, g2, gw, _ = ops.sample_gather(p1, p2, w.detach(), idx)
        F_sel, accu = ops.sample_fits(p1, p2, w, idx)
        # the fit is fed the rows the device gathered: the fp64 fit gets the same rows
        sc.check_fits(F_sel.detach().cpu().numpy(), g1.cpu().numpy(), g2.cpu().numpy(), gw.cpu().numpy(), case, tag)
        GF = torch.randn(F_sel.shape, generator=torch.Generator().manual_seed(case["seed"]))
        (F_sel * GF.to(DEV)).sum().backward()
        sc.check_fit_adjoint(w.grad.cpu().numpy(), F_sel.detach().cpu().numpy(), case, GF.numpy(), tag)
        with pytest.raises(dfepe.DfepeError):
            ops.sample_fits(p1.clone().requires_grad_(True), p2, w, idx)


def test_accu_adjoint_against_float64_autograd(dfepe):
    """d <accu, GA> / d weights.  accu enters the scatter as the float32 the gather wrote (2^-24 each), at most H K = 2000 terms per
    correspondence with cancellation between sets: 1e-5 of the largest entry, about 170 x 2^-24."""
    case = sc.fit_case(2, 64, 100, 20, 3)
    w = _t(case["weights"]).requires_grad_(True)
    _, accu = dfepe.ops.sample_fits(_t(case["pts1"]), _t(case["pts2"]), w, _t(case["idx"]))
    GA = torch.randn(accu.shape, generator=torch.Generator().manual_seed(1))
    (accu * GA.to(DEV)).sum().backward()
    w64 = torch.from_numpy(case["weights"]).double().requires_grad_(True)
    b = torch.arange(2)[:, None, None]
    p = torch.prod(w64[b, torch.from_numpy(case["idx"]).long()] * 1000.0, dim=2, keepdim=True)
    ((p / (p.sum(1, keepdim=True) + 1e-10)) * GA.double()).sum().backward()
    e = fac.relerr(w.grad.cpu().numpy(), w64.grad.numpy())
    print(f"SAMPLE accu adjoint: {e:.3e} (bound 1e-05)")
    assert e < 1e-5


def test_loss_and_its_adjoint(dfepe):
    for case in sc.loss_cases():
        F = _t(case["F_sel"]).requires_grad_(True)
        loss = dfepe.ops.sample_floss(F, _t(case["T1"]), _t(case["T2"]), _t(case["virt1"]), _t(case["virt2"]), case["clamp"])
        (loss * _t(case["g"])).sum().backward()
        sc.check_loss(loss.detach().cpu().numpy(), F.grad.cpu().numpy(), case)


def test_scatter(dfepe):
    ops = dfepe.ops
    chunk = dfepe._lib.lib().dfepe_sample_scatter_chunk()
    for case in sc.scatter_cases(chunk):
        w, idx = _t(case["weights"]), _t(case["idx"])
        B, N = case["weights"].shape
        zero = torch.zeros(B, N, 3, device=DEV)
        accu = ops.sample_gather(zero, zero, w, idx)[3]
        for with_accu in (True, False):
            run = lambda: ops.sample_scatter_bwd(_t(case["g_w_sel"]), _t(case["g_accu"]) if with_accu else None, w, accu, idx).cpu().numpy()
            g_w, again = run(), run()
            assert (g_w.view(np.uint32) == again.view(np.uint32)).all()  # two runs bit-identical
            sc.check_scatter(g_w, case, accu.cpu().numpy(), with_accu)


def _step(dfepe, fit, p1, p2, logits, virt1, virt2, T):
    # the gradient is taken at a fresh view of the leaf, as compat.CapturedStep takes its own: the node it ends at is created here,
    # on the stream of the step, and the leaf's AccumulateGrad node (which lives on whatever stream first used it) stays out of it
    lv = logits.view_as(logits)
    w = torch.softmax(lv, 1)
    sel = fit.selected(p1, p2, w.unsqueeze(1), None)
    F_sel = sel["out_sample_selected_batch"]
    loss = dfepe.ops.sample_floss(F_sel, T, T, virt1, virt2, 0.02).sum() / (F_sel.numel() / 9 * virt1.shape[1])
    return loss, torch.autograd.grad(loss, lv)[0]


def test_captured_step_draws_the_next_sets_on_every_replay(dfepe):
    """Draw (at the device counter), advance, gather, fits, loss and the whole backward in ONE hipGraph: replay r equals the eager step
    at counter c + r.  A linear chain of launches.  The order is that of tests/test_dsac_device_sampler_gpu.py: warm-up on a side
    stream, capture, replays, and only then the eager steps on the default stream."""
    C = dfepe.compat
    case = sc.fit_case(2, 64, 100, 20, 3)
    p1, p2, virt1, virt2 = _t(case["pts1"]), _t(case["pts2"]), _t(case["virt1"]), _t(case["virt2"])
    T = _t(sc.T_HW)
    logits = _t(case["logits"]).requires_grad_(True)
    sampler = C.DeviceSampler(1234, DEV)
    fit = C.DeepFNetSampleLoss.Fit(sampler=sampler)
    c0 = 40
    state = {}

    def step():
        state["loss"], state["g"] = _step(dfepe, fit, p1, p2, logits, virt1, virt2, T)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    loss, g = state["loss"], state["g"]
    sampler.counter.copy_(torch.tensor([c0], dtype=torch.uint32))
    replays = []
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        replays.append((loss.item(), g.cpu().numpy().copy()))
    assert int(sampler.counter.item()) == c0 + 3
    assert replays[0][0] != replays[1][0]  # other sets, another loss
    sampler.counter.copy_(torch.tensor([c0], dtype=torch.uint32))
    for r, (rl, rg) in enumerate(replays):
        step()
        torch.cuda.synchronize()
        assert state["loss"].item() == rl, r
        assert (state["g"].cpu().numpy().view(np.uint32) == rg.view(np.uint32)).all(), r
