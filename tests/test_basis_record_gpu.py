"""The tridiagonalising basis in the fit's `save` record on the GPU (see tests/test_basis_record_cpu.py for the record and the
bounds): the gradients of the backward that applies Q^T and Q as independent sums against float64 autograd of the oracle on every
kernel family, the record the kernels write, the head-riding backward and the seam between the resident and the lean forward build.
GPU box only."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fit_adjoint_cases as fac  # noqa: E402
from test_backward_ladder_gpu import run_device  # noqa: E402
from test_basis_record_cpu import BOUND, MARK_VALUE, S16_MARK, S16_TAG, TAG_VALUE, record_figures  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = float(fac.IMAGE_SIZE[0]), float(fac.IMAGE_SIZE[1])

B_ROW = 37  # two full workgroups of sixteen pairs and five pairs of a third: a partial workgroup and a partial wavefront
# (B, N, row_per_pair): the row kernels IT 1 | 1 | 2 | 2 | 4 | 7 | 7 | 8 | 8, the row kernel that re-reads its correspondences (IT 0,
# forced), the cooperative workgroup
SHAPES = [(B_ROW, n, False) for n in (8, 9, 16, 17, 33, 65, 100, 113, 128)] + [(B_ROW, 129, True), (3, 300, False)]


def shape_seed(N):
    return 500 + N


@pytest.mark.parametrize("variant", ["raw_logits_gF", "raw_logits_all"])
@pytest.mark.parametrize("B,N,rpp", SHAPES)
def test_gradients_through_the_stored_basis_vs_oracle_autograd(dfepe, B, N, rpp, variant):
    """Forward and backward with g_F only (the build without pass A), then with g_residual, g_epi and a gradient on the softmax
    weights as well, against float64 autograd of the oracle: the cases, the reference and the bounds of
    tests/fit_adjoint_cases.py (2e-4 of the largest entry for N >= 20, 2e-3 below); check() prints every figure.
    Measured on an MI355X, largest over all shapes: raw_logits_gF 3.1e-5, raw_logits_all 4.0e-5 (both at the minimal systems)."""
    case = fac.make_case(B, N, shape_seed(N), variant)
    F, grads = run_device(dfepe, case, row_per_pair=rpp)
    assert torch.isfinite(grads["weights"]).all()
    fac.check(case, F, grads, tag="basis")


@pytest.mark.parametrize("B,N,rpp", SHAPES)
def test_record_written_by_the_kernels(dfepe, oracle, B, N, rpp):
    """Q orthogonal, Q^T (M / tr M) Q = T against the oracle's fp64 design matrix, Q z reproduces the returned F, both marks set --
    on the record of every kernel family; a record without the second mark is refused.
    Measured on an MI355X, largest over all shapes: |Q^T Q - I| 8.3e-8, |Q^T M Q - T| 4.2e-8, |F(Q z) - F| 9.6e-8."""
    sc = dfepe.synth.make_scene(B, N, seed=shape_seed(N), outlier_ratio=0.2, noise_px=0.5)
    m = sc["matches_xy_ori"].to(DEV).contiguous()
    logits = sc["logits_layers"][0].to(DEV).contiguous()
    F, _res, _epi, save, wout = dfepe.ops.w8pt_forward(m, None, logits, True, W, H, 0.5, want_epi=True, want_save=True, logits=True,
                                                       row_per_pair=rpp)
    torch.cuda.synchronize()
    orth, tri, dF = record_figures(oracle, m.cpu(), wout.cpu(), F.cpu().reshape(B, 3, 3), save.cpu())
    tolF = 2 * (1e-5 if N < 12 else 1e-6)
    print(f"BASIS B={B} N={N}: |QtQ-I| {orth:.2e} (<= {BOUND}), |QtMQ-T| {tri:.2e} (<= {BOUND}), |F(Qz)-F| {dF:.2e} (< {tolF})")
    assert orth <= BOUND
    assert tri <= BOUND
    assert dF < tolF
    assert (save[:, S16_TAG] == TAG_VALUE).all() and (save[:, S16_MARK] == MARK_VALUE).all()
    bad = save.clone()
    bad[:, S16_MARK] = 0.0
    gF = torch.ones_like(F)
    g = dfepe.ops.w8pt_backward(m, None, wout, True, W, H, 0.5, bad, F, gF, None, None, logits=True, row_per_pair=rpp)
    assert torch.isnan(g).all()
    g = dfepe.ops.w8pt_backward(m, None, wout, True, W, H, 0.5, save, F, gF, None, None, logits=True, row_per_pair=rpp)
    assert torch.isfinite(g).all()


def test_head_riding_backward_equals_the_plain_one(dfepe):
    """hot_path_fused(defer_loss_head=True) -- the backward fit that finishes the loss head beside its first launch, capped at 256
    registers by its 448-thread workgroup -- against defer_loss_head=False at B = 37, N = 100, two layers: gradients bit-identical,
    loss scalars equal after the backward."""
    B, N, depth = B_ROW, 100, 2
    sc = dfepe.pipeline.scene_to_device(dfepe.synth.make_scene(B, N, seed=61, outlier_ratio=0.3, depth_layers=depth), DEV)

    def run(defer):
        logits = sc["logits_layers"][:depth].detach().clone().requires_grad_(True)
        o = dfepe.pipeline.hot_path_fused(sc["matches_xy_ori"], logits, sc["Ks"], sc["pts1_virt_ori"], sc["pts2_virt_ori"], sc["qs_cam"],
                                          sc["ts_cam"], sc["R_gt"], fac.IMAGE_SIZE, 0.02, True, defer_loss_head=defer)
        o["loss"].backward()
        torch.cuda.synchronize()
        return o, logits.grad

    (a, ga), (b, gb) = run(False), run(True)
    assert torch.isfinite(ga).all()
    assert torch.equal(ga.view(torch.int32), gb.view(torch.int32))
    for k in ("loss", "loss_F", "loss_qt", "loss_layers"):
        assert torch.equal(a[k], b[k]), k


def test_batch_seam_whole_record_is_bit_identical(dfepe):
    """One launch of 16384 pairs (the lean forward build) equals four launches of 4096 (the resident build) in every output and in
    every float of the record -- the shape of test_lean_forward_fit_of_large_batches_is_bit_identical, without that test's
    allowance for never-written slots: the record has none any more."""
    B, N = 16384, 100
    sc = dfepe.synth.make_scene(B, N, seed=5, outlier_ratio=0.2, noise_px=0.5)
    m = sc["matches_xy_ori"].to(DEV).contiguous()
    lg = sc["logits_layers"][0].to(DEV).contiguous()
    big = dfepe.ops.w8pt_forward(m, None, lg, True, W, H, 0.5, True, True, logits=True)
    for c in range(0, B, 4096):
        part = dfepe.ops.w8pt_forward(m[c:c + 4096].contiguous(), None, lg[c:c + 4096].contiguous(), True, W, H, 0.5, True, True, logits=True)
        for k, (x, y) in enumerate(zip(big, part)):
            assert torch.equal(x[c:c + 4096].contiguous().view(torch.int32), y.contiguous().view(torch.int32)), k
