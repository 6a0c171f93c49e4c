"""Every kernel that computes the clamped symmetric epipolar distance, held to ONE float64 per-point restatement
(tests/epipolar_ref.py) at every launch edge and on every branch, with T1 != T2 everywhere:
  floss_kernel<BWD, CACHED>    ops.floss, dfepe_floss_bwd                 csrc/floss.hip
  tail_floss_row<IT, JAC, KL>  ops.loss_tail_jac, dfepe_loss_tail         csrc/loss_tail_body.h, loss_tail.hip
  epi_residual_kernel<BWD>     ops.epi_residual                           csrc/geom.hip
  epi_metrics_kernel           ops.epi_metrics                            csrc/geom.hip
Inputs and the one check(): tests/epipolar_cases.py.  Bounds: bound_fwd(C_FWD) and bound_grad(C_GRAD, G) of the restatement, the two
constants being 4 x what the reference's own float32 arithmetic needs (tests/test_epipolar_ref_cpu.py); where an entry point adds
roundings of its own (a stored fp32 Jacobian, fp32 coefficients) they are counted and added, each named where it is added.  No bound
comes from a device number: check() prints the largest observed ratio to each bound for the record.  GPU box only.

Largest ratios observed on an MI355X: docstring of test_zz_record."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epipolar_cases as ec  # noqa: E402
import epipolar_ref as er  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U32 = er.U32
U64 = 2.0 ** -50  # a handful of float64 roundings
ERR_UNSUPPORTED = -3  # include/dfepe.h


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def ge_bound(r, g_ref_total, g_E):
    """What the E adjoint A g_E C^T adds: float64 in the kernel (a handful of roundings of the absolute sum) and the one float32
    rounding of the result."""
    absum = np.einsum("bij,lbjk,bmk->lbim", np.abs(r.A2), np.abs(np.asarray(g_E, dtype=np.float64)), np.abs(r.C1))
    return U32 * np.abs(g_ref_total) + U64 * absum


# ---- ops.floss ----------------------------------------------------------------------------------------------------------------------
def run_floss(dfepe, case, clamp, upstream="both"):
    F = dev(case.F).requires_grad_(True)
    ls, E = dfepe.ops.floss(F, dev(case.T1), dev(case.T2), dev(case.K), dev(case.v1), dev(case.v2), clamp)
    terms = []
    if upstream in ("both", "ls"):
        terms.append((ls * dev(case.g_ls)).sum())
    if upstream in ("both", "E"):
        terms.append((E * dev(case.g_E)).sum())
    sum(terms).backward()
    return host(ls), host(E), host(F.grad)


def check_floss(dfepe, case, clamp, upstream="both", tag="floss"):
    r = ec.reference(case, clamp)
    ls, E, g = run_floss(dfepe, case, clamp, upstream)
    g_ls = case.g_ls if upstream in ("both", "ls") else None
    g_E = case.g_E if upstream in ("both", "E") else None
    g_ref = r.g_F(g_loss_sum=g_ls, g_E=g_E)
    bound = r.bound_grad(G=0.0 if g_ls is None else g_ls)
    extra = None if g_E is None else ge_bound(r, g_ref, g_E)
    if case.special == "exact":  # every point sign-uncertain: forward, finiteness and |g_F| <= sum G |contribution| only
        ec.check(f"{tag} exact", r, loss_sum=ls, E=E)
        assert np.isfinite(g).all()
        lim = r.bound_contribution(np.abs(case.g_ls)) * (1 + 64 * U32) + (0.0 if g_E is None else np.abs(r.g_F(g_E=g_E)) + extra)
        assert (np.abs(g) <= lim).all()
        return
    ec.check(f"{tag} {case.L},{case.B},{case.M} {case.tform} clamp {clamp:g} up {upstream}" + (f" {case.special}" if case.special else ""),
             r, loss_sum=ls, g_F=g, g_ref=g_ref, g_bound=bound, E=E, extra_abs=extra)
    if clamp == 0.0 and g_E is None:
        assert (g == 0).all()  # the F-loss part of the gradient at clamp 0 is exactly 0


@pytest.mark.parametrize("L,B,M", ec.FLOSS_SHAPES)
def test_floss_at_every_launch_edge(dfepe, L, B, M):
    """M = 63/64/65: slot 2 of the cached path; 128/129: the step to the re-reading path; L = 9/10/16: lanes 0..8 hold the nine sums,
    lanes < L combine them; B = 4/5/9: partial workgroups of four pairs.  T form and clamp cycle over the shapes."""
    case, clamp = ec.pick(L, B, M)
    check_floss(dfepe, case, clamp)


@pytest.mark.parametrize("clamp", ec.CLAMPS)
@pytest.mark.parametrize("tform", ec.TFORMS)
def test_floss_every_transform_form_and_clamp(dfepe, tform, clamp):
    """[3,3] / [B,3,3] / one of each (the st1 != st2 branch of ops._t_arg), T1 != T2 in all of them; clamp 0.02 (most points gated), 0.5
    (almost none), 1e30 (none), 0 (every sum and the F-loss gradient exactly 0)."""
    case, _ = ec.get(3, 5, 100, tform, clamp)
    for up in ("both", "ls", "E"):
        check_floss(dfepe, case, clamp, up)


@pytest.mark.parametrize("special", ec.SPECIALS)
def test_floss_special_cases(dfepe, special):
    """The unperturbed F (every point sign-uncertain), an all-zero layer among ordinary ones, a virtual point on the epipole of its own
    image."""
    case, clamp = ec.get(3, 5, 100, "pair", 0.02, special)
    check_floss(dfepe, case, clamp, "both")
    check_floss(dfepe, case, clamp, "ls")


def floss_bwd_cabi(dfepe, case, clamp, coef, scale):
    """dfepe_floss_bwd with g_loss_sum = NULL, a g_loss_coef and a one-element g_scale (the captured step's form of the upstream)."""
    lib, ops = dfepe._lib.lib(), dfepe.ops
    B = case.B
    F = dev(case.F)
    T1 = dev(er.per_pair(case.T1, B).astype(np.float32))
    T2 = dev(er.per_pair(case.T2, B).astype(np.float32))
    K, v1, v2 = dev(case.K), dev(case.v1), dev(case.v2)
    gs = torch.tensor([scale], device=DEV, dtype=torch.float32)
    gF = torch.full_like(F, float("nan"))
    with ops._on(F.device):
        rc = lib.dfepe_floss_bwd(F.data_ptr(), case.L, B, T1.data_ptr(), T2.data_ptr(), 9, K.data_ptr(), v1.data_ptr(), v2.data_ptr(), case.M,
                                 float(clamp), None, float(coef), gs.data_ptr(), None, gF.data_ptr(), ops._stream())
    dfepe._lib.check(rc, "dfepe_floss_bwd")
    torch.cuda.synchronize()
    return host(gF)


@pytest.mark.parametrize("M", [65, 129])
def test_floss_bwd_coefficient_times_scale_form(dfepe, M):
    case, clamp = ec.pick(3, 5, M)
    r = ec.reference(case, clamp)
    coef, scale = np.float32(0.37 / (3 * 5 * M)), np.float32(-1.7)
    g = floss_bwd_cabi(dfepe, case, clamp, coef, scale)
    gl = float(coef) * float(scale)  # formed in float64 by the kernel
    ec.check(f"floss_bwd coef x scale M={M}", r, g_F=g, g_ref=r.g_F(g_loss_sum=gl), g_bound=r.bound_grad(G=abs(gl)))


def test_floss_gate_passes_the_gradient_at_the_bound(dfepe):
    """A case whose fp32 evaluation is exact (epipolar_cases.exact_gate_case): d == clamp_at == 1 on every point.  torch.clamp(max=)
    passes the gradient at the bound, so must floss_kernel, tail_floss_row and epi_residual_kernel.  The restatement's float64 d is
    just below 1 (it keeps the 1e-6 that fp32 absorbs), passes the gate too, and is held with the live part of the bound only."""
    c = ec.exact_gate_case()
    r = er.floss_ref(c.F, c.T1, c.T2, c.K, c.v1, c.v2, 1.0)
    assert r.pt.gate.all() and np.abs(r.sums()).max() > 0.01
    live = (er.C_GRAD * U32 * r.pt.mag).sum(2)
    F = dev(c.F).requires_grad_(True)
    ls, _ = dfepe.ops.floss(F, dev(c.T1), dev(c.T2), dev(c.K), dev(c.v1), dev(c.v2), 1.0)
    ls.sum().backward()
    assert (host(ls) == c.M).all()  # exact arithmetic: every point contributes exactly 1
    ec.check("floss on the gate", r, g_F=host(F.grad), g_ref=r.sums(), g_bound=live)
    F2 = dev(c.F).requires_grad_(True)
    t = dfepe.ops.loss_tail_jac(F2, dev(c.T1), dev(c.T2), dev(c.K), dev(c.v1), dev(c.v2), 1.0)
    t["loss_sum"].sum().backward()
    assert (host(t["loss_sum"]) == c.M).all()
    ec.check("loss_tail_jac on the gate", r, g_F=host(F2.grad), g_ref=r.sums(), g_bound=live)
    F3 = dev(c.F[0]).requires_grad_(True)
    out = dfepe.ops.epi_residual(dev(c.v1), dev(c.v2), F3, 1.0)
    out.sum().backward()
    assert (host(out) == 1.0).all()
    # the fp64 adjoint of epi_residual sees d < 1 like the restatement
    ec.check("epi_residual on the gate", r, g_F=host(F3.grad)[None], g_ref=r.sums()[:1], g_bound=live[:1])


# ---- ops.loss_tail_jac --------------------------------------------------------------------------------------------------------------
def run_tail_jac(dfepe, case, clamp, gt, floss_grad=True):
    F = dev(case.F).requires_grad_(True)
    a = (dev(case.q_gt), dev(case.t_gt), dev(case.R_gt)) if gt else (None, None, None)
    r = dfepe.ops.loss_tail_jac(F, dev(case.T1), dev(case.T2), dev(case.K), dev(case.v1), dev(case.v2), clamp, *a, floss_grad=floss_grad)
    return F, r


def check_tail_jac(dfepe, case, clamp, gt, stats=False):
    r = ec.reference(case, clamp)
    L, B, M = case.L, case.B, case.M
    F, t = run_tail_jac(dfepe, case, clamp, gt)
    tag = f"loss_tail_jac {L},{B},{M} {case.tform} clamp {clamp:g}" + (" gt" if gt else "") + (" stats" if stats else "")
    if not stats:
        (t["loss_sum"] * dev(case.g_ls)).sum().backward()
        G = case.g_ls.astype(np.float64)
        n_round = 1  # a (the upstream) times the stored fp32 Jacobian: one more rounding
    else:
        # loss = sum_l w_l m_loss[l] + w_o o_loss; m_loss[l] = mean_b loss_sum[l, b] / M, o_loss = mean_l m_loss[l]
        w = case.g_ls[:, 0].astype(np.float64)
        w_o = 0.83
        ((t["m_loss"] * dev(case.g_ls[:, 0].copy())).sum() + t["o_loss"] * w_o).backward()
        G = np.broadcast_to(((w + np.float64(np.float32(w_o)) / L) / (M * B))[:, None], (L, B))
        # fp32 roundings of dfepe_loss_tail_bwd on the way: 1 / B, 1 / L, o / L, m + o / L, 1 / M, (1 / M) / B, their product, times J
        n_round = 8
    g_ref = r.g_F(g_loss_sum=G)
    ec.check(tag, r, loss_sum=host(t["loss_sum"]), E=host(t["E_layers"]), g_F=host(F.grad), g_ref=g_ref,
             g_bound=r.bound_grad(G=G), extra_abs=n_round * U32 * np.abs(g_ref))
    return t


@pytest.mark.parametrize("gt", [False, True])
@pytest.mark.parametrize("L,B,M", ec.TAIL_SHAPES)
def test_loss_tail_jac_at_every_rung_and_edge(dfepe, L, B, M, gt):
    """M = 1/16/17/32/33/64/65/112: every IT rung of the Jacobian tail and its edges; B = 1/15/16/17/33: partial workgroups of 16
    pairs; L = 1..5, 16: the odd-L remainder of the two-at-a-time walk.  With and without ground truth (the pose lanes run or idle);
    upstream per element."""
    case, clamp = ec.pick(L, B, M)
    check_tail_jac(dfepe, case, clamp, gt)


@pytest.mark.parametrize("gt", [False, True])
def test_loss_tail_jac_upstream_through_the_batch_statistics(dfepe, gt):
    for (L, B, M) in ((3, 17, 33), (5, 17, 37)):
        case, clamp = ec.pick(L, B, M)
        check_tail_jac(dfepe, case, clamp, gt, stats=True)


def test_loss_tail_jac_without_the_floss_jacobian(dfepe):
    """floss_grad = False: the forward values are unchanged, the pose gradient is bit-identical, a gradient on the F-loss is an error."""
    case, clamp = ec.pick(3, 17, 33)
    r = ec.reference(case, clamp)
    F1, t1 = run_tail_jac(dfepe, case, clamp, True, floss_grad=True)
    F0, t0 = run_tail_jac(dfepe, case, clamp, True, floss_grad=False)
    ec.check("loss_tail_jac floss_grad=False", r, loss_sum=host(t0["loss_sum"]), E=host(t0["E_layers"]))
    assert torch.equal(t0["loss_sum"], t1["loss_sum"]) and torch.equal(t0["E_layers"], t1["E_layers"])
    (t1["q_l2"].sum() + 0.5 * t1["t_l2"].sum()).backward()
    (t0["q_l2"].sum() + 0.5 * t0["t_l2"].sum()).backward()
    assert torch.equal(F0.grad, F1.grad) and torch.isfinite(F0.grad).all()
    _, t = run_tail_jac(dfepe, case, clamp, False, floss_grad=False)
    with pytest.raises(dfepe._lib.DfepeError):
        t["loss_sum"].sum().backward()


def test_loss_tail_jac_refuses_more_than_112_points(dfepe):
    case, clamp = ec.pick(3, 17, 113)
    with pytest.raises(dfepe._lib.DfepeError, match=r"not supported.*code -3"):  # DFEPE_ERR_UNSUPPORTED, refused on the host
        run_tail_jac(dfepe, case, clamp, False)


# ---- dfepe_loss_tail through the C ABI ----------------------------------------------------------------------------------------------
def run_one_launch_tail(dfepe, case, clamp, gt, balance_F, defer_head=0, M=None):
    """As tests/test_pose_branches_gpu.py calls it (pipeline.hot_path_fused's arguments), with per-pair T1 != T2."""
    lib, ops = dfepe._lib.lib(), dfepe.ops
    L, B = case.L, case.B
    M = case.M if M is None else M
    F = dev(case.F)
    T1 = dev(er.per_pair(case.T1, B).astype(np.float32))
    T2 = dev(er.per_pair(case.T2, B).astype(np.float32))
    K, v1, v2 = dev(case.K), dev(case.v1), dev(case.v2)
    q_gt, t_gt, R_gt = (dev(case.q_gt), dev(case.t_gt), dev(case.R_gt)) if gt else (None, None, None)
    loss_sum, E = torch.full((L, B), float("nan"), device=DEV), torch.empty(L, B, 3, 3, device=DEV)
    q_l2, t_l2, R_deg, t_deg = (torch.empty(L, B, device=DEV) for _ in range(4))
    sel = torch.empty(L, B, device=DEV, dtype=torch.int32)
    gF = torch.full((L, B, 3, 3), float("nan"), device=DEV)
    packed = torch.empty(L + 4, device=DEV, dtype=torch.float64)
    scalars = torch.empty(4 + L, device=DEV)
    ws = dfepe.pipeline._tail_workspace(torch.device(DEV), B)
    p = lambda t: None if t is None else t.data_ptr()
    with ops._on(F.device):
        rc = lib.dfepe_loss_tail(p(F), L, B, p(T1), p(T2), 9, p(K), p(v1), p(v2), M, float(clamp), p(q_gt), p(t_gt), p(R_gt), 10.0, 10.0,
                                 float(balance_F), 0.7, 1.3, float(B), p(loss_sum), p(E), p(q_l2) if gt else None, p(t_l2) if gt else None,
                                 p(R_deg) if gt else None, p(t_deg) if gt else None, p(sel) if gt else None, p(gF), p(packed), p(scalars),
                                 p(ws), int(defer_head), ops._stream())
    if rc != 0:
        return rc, None, None, None
    torch.cuda.synchronize()
    return rc, host(loss_sum), host(E), host(gF)


@pytest.mark.parametrize("L,B,M", ec.TAIL_SHAPES + ec.TAIL_ABI_SHAPES)
def test_one_launch_loss_tail_at_every_rung_and_edge(dfepe, L, B, M):
    """Without ground truth g_F is coef_F x the restatement's sums, coef_F = float32(balance_F / (L B M)).  With ground truth the
    F-loss part is g_F(balance_F = 1) - g_F(balance_F = 0): the same bound plus one float32 rounding of the larger operand (the fma of
    coef_F x sums onto the pose part rounds once).  defer_head 0 and 1 give the same loss_sum and g_F."""
    case, clamp = ec.pick(L, B, M)
    r = ec.reference(case, clamp)
    bF = 0.9
    coef = float(np.float32(bF / (float(L) * B * M)))
    tag = f"loss_tail {L},{B},{M} {case.tform} clamp {clamp:g}"
    rc, ls, E, g = run_one_launch_tail(dfepe, case, clamp, False, bF)
    assert rc == 0
    ec.check(tag, r, loss_sum=ls, E=E, g_F=g, g_ref=r.g_F(g_loss_sum=coef), g_bound=r.bound_grad(G=coef))
    rc, ls_d, E_d, g_d = run_one_launch_tail(dfepe, case, clamp, False, bF, defer_head=1)
    assert rc == 0 and np.array_equal(ls_d, ls) and np.array_equal(g_d, g) and np.array_equal(E_d, E)
    rc1, ls1, _, g1 = run_one_launch_tail(dfepe, case, clamp, True, bF)
    rc0, ls0, _, g0 = run_one_launch_tail(dfepe, case, clamp, True, 0.0)
    assert rc1 == 0 and rc0 == 0 and np.array_equal(ls1, ls) and np.array_equal(ls0, ls)
    assert np.isfinite(g1).all() and np.isfinite(g0).all()
    ec.check(tag + " gt", r, g_F=g1.astype(np.float64) - g0, g_ref=r.g_F(g_loss_sum=coef), g_bound=r.bound_grad(G=coef),
             extra_abs=U32 * np.maximum(np.abs(g1), np.abs(g0)))


def test_one_launch_loss_tail_refuses_more_than_128_points(dfepe):
    """Refused on the host before any launch: the buffers are those of M = 128, only the argument says 129."""
    case, clamp = ec.pick(3, 17, 128)
    rc, _, _, _ = run_one_launch_tail(dfepe, case, clamp, False, 0.9, M=129)
    assert rc == ERR_UNSUPPORTED


# ---- ops.epi_residual ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def residual_inputs():
    """Transformed points of a shared case with a third coordinate != 1 (each point times 0.5..2), as float32 homogeneous points."""
    case, _ = ec.pick(3, 5, 200)
    r = ec.reference(case, 0.5)
    g = np.random.default_rng(17)
    w1, w2 = g.uniform(0.5, 2.0, r.x1.shape[:2] + (1,)), g.uniform(0.5, 2.0, r.x2.shape[:2] + (1,))
    p1, p2 = (r.x1 * w1).astype(np.float32), (r.x2 * w2).astype(np.float32)
    up = (g.uniform(0.5, 1.5, p1.shape[:2]) * np.where(g.uniform(size=p1.shape[:2]) < 0.5, -1.0, 1.0)).astype(np.float32)
    return p1, p2, case.F[1], up


@pytest.mark.parametrize("clamp", [0.02, 0.5, 0.0])
@pytest.mark.parametrize("B", [1, 4, 5])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 130])
def test_epi_residual_at_every_edge(dfepe, residual_inputs, N, B, clamp):
    """One wavefront per pair, four pairs per workgroup, lanes stride over N.  Forward (fp32) within bound_fwd per point; the adjoint is
    float64 in the kernel: one float32 rounding of the result plus 2^-50 sum G mag, a point flagged only inside the float64 band."""
    P1, P2, Fm, UP = residual_inputs
    p1, p2, F32, up = P1[:B, :N], P2[:B, :N], Fm[:B], UP[:B, :N]
    r = er.residual_ref(p1, p2, F32, clamp)
    F = dev(F32).requires_grad_(True)
    out = dfepe.ops.epi_residual(dev(p1), dev(p2), F, clamp)
    (out * dev(up)).sum().backward()
    o = host(out).astype(np.float64)
    if clamp == 0.0:
        assert (o == 0).all()
    ratio = np.abs(o - r.out) / r.pt.bound_fwd()[0]
    print(f"EPI epi_residual {B},{N} clamp {clamp:g}: forward {ratio.max():.3f} of its bound")
    assert ratio.max() <= 1.0
    g_ref = er.g_F_points(r, up)[None]
    bound = r.bound_grad(c=1.0, G=np.abs(up.astype(np.float64))[None], u=U64, c_flag=1.0, u_flag=U64) + U32 * np.abs(g_ref)
    ec.check(f"epi_residual {B},{N} clamp {clamp:g}", r, g_F=host(F.grad)[None], g_ref=g_ref, g_bound=bound)


# ---- ops.epi_metrics ----------------------------------------------------------------------------------------------------------------
def metric_ref(kind, F, X, Y, homo, clamp, eps):
    if kind == 0:
        return er.sym_epi(F, X, Y, homo, clamp, eps)
    return er.sampson(F, X, Y, homo) if kind == 1 else er.epi_distance(F, X, Y, homo)


def check_metric(dfepe, kind, F, X, Y, clamp=None, eps=0.0, tag=""):
    homo = X.shape[2] == 3
    got = host(dfepe.ops.epi_metrics(kind, dev(F), dev(X), dev(Y), clamp_at=clamp, eps=eps))
    ref = metric_ref(kind, F, X, Y, homo, clamp, eps)
    assert got.shape == ref.shape and got.dtype == np.float32
    # the kernel computes in float64 and writes float32: the result lies between the float32 roundings of ref (1 -+ 1e-12)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{tag}: NaN where the float64 formula has none (or the reverse)"
    assert np.array_equal(np.isinf(got), np.isinf(ref) | (fin & (np.abs(ref) > np.finfo(np.float32).max)))
    with np.errstate(over="ignore"):
        lo, hi = (ref[fin] * (1 - 1e-12)).astype(np.float32), (ref[fin] * (1 + 1e-12)).astype(np.float32)
    ok = (got[fin] >= np.minimum(lo, hi)) & (got[fin] <= np.maximum(lo, hi))
    assert ok.all(), f"{tag}: {int((~ok).sum())} of {ok.size} outside the float32 roundings of the float64 value"


@pytest.fixture(scope="module")
def metric_inputs():
    g = np.random.default_rng(23)
    case, _ = ec.pick(3, 5, 200)
    F = case.F[0, :3]
    r = ec.reference(case, 0.5)
    X2, Y2 = r.x1[:3, :, :2].copy(), r.x2[:3, :, :2].copy()
    w1, w2 = g.uniform(0.5, 2.0, (3, 200, 1)), g.uniform(0.5, 2.0, (3, 200, 1))
    X3, Y3 = (r.x1[:3] * w1).astype(np.float32), (r.x2[:3] * w2).astype(np.float32)
    # one long pair for the B N = 255 / 256 / 257 edges of the one-lane-per-correspondence launch
    XL2, YL2 = np.concatenate((X2[0], X2[1]))[None], np.concatenate((Y2[0], Y2[1]))[None]
    XL3, YL3 = np.concatenate((X3[0], X3[1]))[None], np.concatenate((Y3[0], Y3[1]))[None]
    return F, (X2, Y2), (X3, Y3), (XL2, YL2), (XL3, YL3)


@pytest.mark.parametrize("homo", [False, True])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_epi_metrics_at_every_edge(dfepe, metric_inputs, kind, homo):
    """B N = 1 / 255 / 256 / 257 (the last lane of a workgroup, one past it) and 3 x 100; 2-D and homogeneous points; for the squared
    symmetric distance every clamp_at (None, 0, 0.3) and eps (0, 1e-10)."""
    F, d2, d3, l2, l3 = metric_inputs
    (X, Y), (XL, YL) = (d3, l3) if homo else (d2, l2)
    variants = [(cl, eps) for cl in (None, 0.0, 0.3) for eps in (0.0, 1e-10)] if kind == 0 else [(None, 0.0)]
    for cl, eps in variants:
        for n in (1, 255, 256, 257):
            check_metric(dfepe, kind, F[:1], XL[:, :n], YL[:, :n], cl, eps, tag=f"kind {kind} homo {homo} 1x{n} clamp {cl} eps {eps}")
        check_metric(dfepe, kind, F, X[:, :100], Y[:, :100], cl, eps, tag=f"kind {kind} homo {homo} 3x100 clamp {cl} eps {eps}")


@pytest.mark.parametrize("homo", [False, True])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_epi_metrics_where_F_x_vanishes(dfepe, kind, homo):
    """F = [x]_x with x = (2, 3, 1): F x = 0 exactly, so the squared symmetric distance is 0 * inf, the distance to F x is 0 / 0.  The
    kernel returns what the float64 formula gives, NaN included -- also under a clamp (torch.clamp keeps a NaN)."""
    F = np.array([[[0, -1, 3], [1, 0, -2], [-3, 2, 0]]], dtype=np.float32)
    X = np.array([[[2, 3, 1], [1, 1, 1], [2, 3, 1], [4, 6, 2]]], dtype=np.float32)
    Y = np.array([[[5, 1, 1], [2, 7, 1], [2, 3, 1], [1, 2, 1]]], dtype=np.float32)
    if not homo:
        X, Y = X[..., :2].copy(), Y[..., :2].copy()
        X[0, 3] = (2, 3)
    for cl, eps in ([(None, 0.0), (0.3, 0.0), (0.0, 0.0), (0.3, 1e-10)] if kind == 0 else [(None, 0.0)]):
        check_metric(dfepe, kind, F, X, Y, cl, eps, tag=f"F x = 0, kind {kind} homo {homo} clamp {cl} eps {eps}")


def test_zz_record():
    """Prints the largest ratio to its bound that each entry point reached in this run (nothing is asserted from them).

    Measured on an MI355X (largest ratio to the bound over all cases of an entry point):
      ops.floss          loss_sum 0.066, E 0.000 (bit-identical to float32(E_ref)), g_F 0.039 with the upstream on loss_sum alone; 0.98 where
                         the upstream is on E, whose bound is the one float32 rounding of the result and is reached by construction
      dfepe_floss_bwd    g_F 0.037 (g_loss_coef x g_scale)
      ops.loss_tail_jac  loss_sum 0.074, E 0.000, g_F 0.054
      dfepe_loss_tail    loss_sum 0.074, E 0.000, g_F 0.741 (the difference of two runs with ground truth: one float32 rounding of the
                         larger operand dominates that bound)
      ops.epi_residual   forward 0.176, adjoint 0.962 (float64 in the kernel: again the one float32 rounding of the result)
      the case on the gate: 0.005 for all three kernels."""
    groups = {}
    for tag, d in ec.RECORD.items():
        key = tag.split(" ")[0]
        for k, v in d.items():
            groups.setdefault(key, {})
            groups[key][k] = max(groups[key].get(k, 0.0), v)
    for key, d in sorted(groups.items()):
        print(f"EPI RECORD {key}: " + "  ".join(f"{k} {v:.3f}" for k, v in sorted(d.items())))
