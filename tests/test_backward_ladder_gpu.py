"""The backward of the weighted 8-point fit (csrc/w8pt16_bwd_body.h through the launchers of csrc/w8pt16.hip) against float64 autograd
of the oracle at every rung of the N ladder, on both sides of every edge of fit_plan.h and in every kernel family: the row kernels
w8pt16_bwd_kernel<IT, RAW, PGRAD, PLAIN, UP> for IT in 0, 1, 2, 4, 7, 8 and the cooperative w8pt16_coop_bwd_kernel<IT, RAW> for IT in
2, 4, 8.  The cases, the reference and the bounds are those of tests/fit_adjoint_cases.py; tests/test_emu_cpu.py runs the same cases
through the host emulation of the bodies, so a miss here that passes there is a build or launch defect.  GPU box only.

The largest relative errors measured on an MI355X are in the docstrings of the tests; the host emulation of the same cases gives the
same figures to two digits (1.054e-4 against 1.056e-4 at the worst case), i.e. the builds compute what the source says."""
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

ROW_B = 19  # two workgroups of sixteen pairs; the last holds three pairs, all in one wavefront
ROW_N = (8, 16, 17, 32, 33, 64, 65, 112, 113, 128)  # IT 1 | 1 | 2 | 2 | 4 | 4 | 7 | 7 | 8 | 8
ROW_PER_PAIR_N = (129, 257)                          # IT 0, forced (W8PT_ROW_PER_PAIR) where the cooperative workgroup would serve
PAST_COOP = (3, 2049)                                # IT 0 by the plan: N past the cooperative limit
COOP_B = 3
COOP_N = (129, 512, 513, 1024, 1025, 2048)           # IT 2 | 2 | 4 | 4 | 8 | 8
COOP_VARIANTS = ("raw_logits_gF", "raw_logits_all", "homog_gF", "homog_all")  # no point gradients, plain rows: what the plan gives it


def ladder_seed(N):
    return 100 + N


def run_device(dfepe, case, row_per_pair=False, g_scale=None, drop=()):
    """Forward (for the save record) and backward launch of a case through the C ABI.  Returns (F, {"weights", "pts1", "pts2"}).
    drop: names of upstream gradients to leave out of this launch."""
    a = case.launch
    d = lambda t: None if t is None else t.to(DEV).contiguous()
    up = lambda k: None if k in drop else d(a[k])
    pts1, pts2, w = d(a["pts1"]), d(a["pts2"]), d(a["weights"])
    F, _res, _epi, save, w_out = dfepe.ops.w8pt_forward(pts1, pts2, w, a["raw"], W, H, 0.5, want_epi=True, want_save=True, logits=a["logits"],
                                                       row_per_pair=row_per_pair, extra_flags=a["flags"])
    out = dfepe.ops.w8pt_backward(pts1, pts2, w_out if a["logits"] else w, a["raw"], W, H, 0.5, save, F, up("gF"), up("gRes"), up("gEpi"),
                                  logits=a["logits"], gW_extra=up("gW_extra"), want_pts=a["want_pts"], row_per_pair=row_per_pair,
                                  g_scale=None if g_scale is None else torch.tensor([g_scale], device=DEV), extra_flags=a["flags"])
    torch.cuda.synchronize()
    gW, gP1, gP2 = out if a["want_pts"] else (out, None, None)
    return F, {"weights": gW, "pts1": gP1, "pts2": gP2}


@pytest.mark.parametrize("variant", list(fac.VARIANTS))
@pytest.mark.parametrize("B,N", [(ROW_B, n) for n in ROW_N + ROW_PER_PAIR_N] + [PAST_COOP])
def test_row_backward_vs_oracle_autograd(dfepe, B, N, variant):
    """Row kernels: every rung and both sides of every edge (N = 8 .. 128), IT 0 forced at N = 129 / 257 and taken by the plan at
    N = 2049; seven variants, each its own instantiation (tests/fit_adjoint_cases.py: VARIANTS).  Bounds: fit_adjoint_cases.bound.

    Measured on an MI355X, largest error relative to the largest entry over the N >= 20 (in brackets: N = 8, 16, 17), weight / logits
    gradient | point gradients:
        raw_logits_gF    1.7e-6 (1.1e-4)
        raw_logits_all   1.0e-5 (1.0e-4)
        raw_points       4.5e-6 (4.1e-5) | 8.6e-6 (8.1e-4)
        homog_points     8.5e-6 (5.6e-6) | 3.6e-5 (7.2e-4)
        homog_gF         6.6e-7 (6.4e-6)
        homog_all        8.5e-6 (5.6e-6)
        homog_norownorm  2.9e-7 (2.6e-6)
    The bracketed maxima are all at N = 8, the minimal system."""
    case = fac.make_case(B, N, ladder_seed(N), variant)
    F, grads = run_device(dfepe, case, row_per_pair=N in ROW_PER_PAIR_N)
    fac.check(case, F, grads, tag="row")


@pytest.mark.parametrize("variant", COOP_VARIANTS)
@pytest.mark.parametrize("N", COOP_N)
def test_cooperative_backward_vs_oracle_autograd(dfepe, N, variant):
    """w8pt16_coop_bwd_kernel<2 | 4 | 8, RAW> on both sides of its two edges (512 | 513, 1024 | 1025) and at its ends (129, 2048), against
    float64 autograd -- not against the row kernel, as test_cooperative_workgroup_per_pair does.

    Measured on an MI355X, largest over all N: raw_logits_gF 5.1e-7, raw_logits_all 7.4e-6, homog_gF 7.7e-7, homog_all 1.8e-6."""
    case = fac.make_case(COOP_B, N, ladder_seed(N), variant)
    F, grads = run_device(dfepe, case)
    fac.check(case, F, grads, tag="coop")


# The softmax adjoint g_logit_i = w_i (g_w_i - sum_j w_j g_w_j) is formed in fp32: g_w_i is rounded once (2^-24 relative) and the sum runs
# over <= 17 terms per lane and a four-step row reduction, so its error is <= 21 * 2^-24 = 1.3e-6 of sum_j |w_j g_w_j| <= max |g_w|.  Each of
# the two launches therefore carries <= 1.5e-6 w_i max |g_w| per entry, and the largest entry is of the order max_i w_i max |g_w| (the g_w of
# the outliers are far from their weighted mean): 1e-5 of the largest entry is "equal to fp32 rounding" with a factor of three to spare.
G_SCALE_BOUND = 1e-5


@pytest.mark.parametrize("variant", ["raw_logits_gF", "raw_logits_all"])
@pytest.mark.parametrize("N", [16, 32, 64, 112, 128, 257])
def test_g_scale_multiplies_the_gradient(dfepe, N, variant):
    """One N per rung (IT 1, 2, 4, 7, 8 and 0): a launch with a g_scale tensor of -2.5 gives -2.5 times the gradient of the launch
    without, to fp32 rounding, in the build without pass A (g_F only) and in the one with it (g_F, g_residual, g_epi; g_scale does not
    apply to g_weights_extra, which is left out here).  Measured on an MI355X: <= 1.2e-7 of the largest entry."""
    case = fac.make_case(ROW_B, N, ladder_seed(N), variant)
    rpp = N in ROW_PER_PAIR_N
    _, plain = run_device(dfepe, case, row_per_pair=rpp, drop=("gW_extra",))
    _, scaled = run_device(dfepe, case, row_per_pair=rpp, drop=("gW_extra",), g_scale=-2.5)
    e = fac.relerr(scaled["weights"].cpu().numpy(), -2.5 * plain["weights"].double().cpu().numpy())
    print(f"FITADJ g_scale variant={variant} N={N}: {e:.3e} (bound {G_SCALE_BOUND:.0e})")
    assert e < G_SCALE_BOUND


@pytest.mark.parametrize("N", [16, 64, 128])
def test_hot_path_step_matches_oracle_on_the_ladder(dfepe, oracle, N):
    """The whole step (fused tail, the backward fit with and without the deferred head riding on it) at IT 1, 4, 8, the way
    test_hot_path_step_matches_oracle holds it at N = 100 (IT 7): same bounds.  Measured on an MI355X: loss within 1.3e-8, logits
    gradient within 6.4e-7 / 2.9e-7 / 9.1e-7 of its largest entry at N = 16 / 64 / 128."""
    B, depth = 6, 2
    relerr = fac.relerr
    sc = dfepe.synth.make_scene(B, N, seed=21 + N, outlier_ratio=0.2, depth_layers=depth)
    ours = dfepe.pipeline.hot_path_step(dfepe.pipeline.scene_to_device(sc, DEV), fac.IMAGE_SIZE, depth, 0.02, qt=True)
    ref = oracle.hot_path_step({k: v.double() for k, v in sc.items()}, fac.IMAGE_SIZE, depth, 0.02, qt=True, mode="batched")
    e = relerr(ours["grad_logits"].cpu().numpy(), ref["grad_logits"].numpy())
    print(f"FITADJ step N={N}: |loss - ref| {abs(ours['loss'].item() - ref['loss'].item()):.2e}, grad_logits {e:.3e} (bound 5e-4)")
    assert abs(ours["loss"].item() - ref["loss"].item()) < 2e-6 * max(1.0, abs(ref["loss"].item()))
    np.testing.assert_allclose(ours["loss_layers"].detach().cpu().numpy(), torch.stack(ref["losses"]["loss_layers"]).detach().numpy(), rtol=2e-5, atol=1e-8)
    np.testing.assert_allclose(ours["q_l2"].detach().cpu().numpy(), ref["pose"]["q_l2"].detach().numpy(), atol=2e-6, rtol=1e-5)
    np.testing.assert_allclose(ours["t_l2"].detach().cpu().numpy(), ref["pose"]["t_l2"].detach().numpy(), atol=2e-5, rtol=1e-4)
    np.testing.assert_allclose(ours["R_deg"].cpu().numpy(), ref["pose"]["R_deg"], atol=2e-3, rtol=1e-4)
    np.testing.assert_allclose(ours["t_deg"].cpu().numpy(), ref["pose"]["t_deg"], atol=2e-2, rtol=1e-4)
    assert e < 5e-4
    # the head-riding build (w8pt16_bwd_head_kernel<IT, true, false>) against the same truth
    b = dfepe.pipeline.hot_path_step(dfepe.pipeline.scene_to_device(sc, DEV), fac.IMAGE_SIZE, depth, 0.02, qt=True, defer_loss_head=True)
    torch.cuda.synchronize()
    assert relerr(b["grad_logits"].cpu().numpy(), ref["grad_logits"].numpy()) < 5e-4
    assert abs(b["loss"].item() - ref["loss"].item()) < 2e-6 * max(1.0, abs(ref["loss"].item()))
