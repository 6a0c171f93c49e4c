"""The fp64 restatement of the estimator's GEMM kernels (tests/est_gemm_ref.py) and the checks of tests/est_gemm_cases.py, on the host:
the restatement against torch float64 autograd of leaky_relu(instance_norm(X W^T)); a plain torch fp32 evaluation of each kernel's
chain on host-built planes through every check() (the bounds hold for a correct fp32 evaluation); seven mutations of that evaluation,
each rejected on its own (the checks notice a wrong one); the cap on undecided elements over the whole matrix."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import est_gemm_cases as cs  # noqa: E402
import est_gemm_ref as ref  # noqa: E402

F = torch.nn.functional
KPTS = ref.KPTS
EPS = 1e-5


# ---- the restatement against autograd ------------------------------------------------------------------------------------------------
def _exact_planes(x, dtype):
    """Planes of values that need no second plane (x already rounded to `dtype`): the product of the planes IS the product."""
    return ref.block(torch.stack([x.to(dtype), torch.zeros_like(x).to(dtype)]))


@pytest.mark.parametrize("M,pairs,K,slope", [(32, 3, 32, 0.01), (64, 2, 96, 0.01), (32, 2, 64, 2.0)])
def test_restatement_against_float64_autograd(M, pairs, K, slope):
    g = torch.Generator().manual_seed(M + K)
    ncols = pairs * KPTS
    W = (torch.randn(M, K, generator=g) / K ** 0.5).half().float()
    X = torch.randn(ncols, K, generator=g).half().float()
    gamma = (1 + 0.2 * torch.randn(M, generator=g)).double()
    beta = (0.3 * torch.randn(M, generator=g)).double()
    gamma[5] = 0.0
    Wp, Xp = _exact_planes(W * 8.0, torch.float16), _exact_planes(X, torch.float16)
    r = ref.layer_forward(Wp, Xp, 8.0, gamma, beta, EPS, slope)
    Wd, Xd = W.double().requires_grad_(True), X.double()
    gm, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    Y = (Xd @ Wd.t()).view(pairs, KPTS, M).permute(0, 2, 1)  # [pairs, M, N]
    Y.retain_grad()
    a = F.leaky_relu(F.instance_norm(Y, weight=gm, bias=bt, eps=EPS), slope)
    a_cm = a.permute(0, 2, 1).reshape(ncols, M)
    rel = lambda x, y: float((x - y).abs().max() / y.abs().max())
    assert rel(r["a"], a_cm.detach()) < 1e-12
    rstd = 1.0 / torch.sqrt(Y.detach().var(2, unbiased=False) + EPS)
    assert rel(r["rstd"], rstd) < 1e-12
    # the adjoint on the same activation (float64: no plane quantisation) and an arbitrary upstream gradient
    G = torch.randn(ncols, M, generator=g, dtype=torch.float64)
    (a_cm * G).sum().backward()
    ad = ref.adjoint(G, torch.zeros_like(G), a_cm.detach(), rstd, gamma, beta, slope)
    live = gamma != 0
    ref_dY = Y.grad.permute(0, 2, 1).reshape(ncols, M)
    assert rel(ad["dY"][:, live], ref_dY[:, live]) < 1e-12
    assert float(ad["dY"][:, ~live].abs().max()) == 0.0 and float(ref_dY[:, ~live].abs().max()) < 1e-12
    assert rel(ad["dbeta"].sum(0), bt.grad) < 1e-12
    assert rel(ad["dgamma"].sum(0)[live], gm.grad[live]) < 1e-12
    assert float(ad["dgamma"][:, ~live].abs().max()) == 0.0  # the kernels' definition; dfepe_est_dgamma_zero supplies the true value


def test_product_takes_the_terms_the_kernel_multiplies():
    g = torch.Generator().manual_seed(3)
    A, B = torch.randn(40, 64, generator=g), torch.randn(17, 64, generator=g)
    for planes, order, host in ((2, 1, lambda x: ref.host_planes_bf16(x, 2)), (3, 2, lambda x: ref.host_planes_bf16(x, 3)), (2, 1, ref.host_planes_f16)):
        Ap, Bp = host(A), host(B)
        a, b = ref.unblock(Ap), ref.unblock(Bp)
        assert torch.equal(ref.unblock(ref.block(a)), a)
        full = b.sum(0) @ a.sum(0).t()
        dropped = sum(b[j] @ a[i].t() for i in range(planes) for j in range(planes) if i + j > order)
        value, bound = ref.product(Ap, Bp, order)
        assert float((value - (full - dropped)).abs().max()) < 1e-13 * float(full.abs().max())
        terms = sum(1 for i in range(planes) for j in range(planes) if i + j <= order)
        assert terms == (3 if planes == 2 else 6)
        mag = sum(b[j].abs() @ a[i].abs().t() for i in range(planes) for j in range(planes) if i + j <= order)
        assert torch.allclose(bound, ref.SLACK * terms * 64 * 2.0 ** -23 * mag, rtol=1e-12, atol=0)
    v2, b2 = ref.product(Ap, Bp, 1, scale=4.0, ksteps=(1, 2))
    v1, b1 = ref.product(ref.host_planes_f16(A[:, 32:]), ref.host_planes_f16(B[:, 32:]), 1)
    assert torch.equal(v2 * 4.0, v1) and torch.equal(b2 * 4.0, b1)
    assert ref.split_ksteps(160, 3) == [(0, 1), (1, 3), (3, 5)] and ref.tn_slices(100, 8)[3:5] == [(96, 100), (128, 100)]
    assert ref.weight_scale(0.02) * 0.02 >= 8.0 and ref.weight_scale(0.02) * 0.02 < 16.0


# ---- a plain fp32 evaluation of each chain on the planes' values ---------------------------------------------------------------------
def f32(P):
    return ref.unblock(P).float()


def emu_product(Ap, Bp, order, scale=1.0, ksteps=None, mut=None):
    A, B = f32(Ap), f32(Bp)
    if ksteps is not None:
        A, B = A[..., 32 * ksteps[0]:32 * ksteps[1]], B[..., 32 * ksteps[0]:32 * ksteps[1]]
    if mut == "k_step_left_out":
        A = A.clone()
        A[..., :32] = 0.0
    acc = torch.zeros(B.shape[1], A.shape[1])
    for i in range(A.shape[0]):
        for j in range(B.shape[0]):
            if i + j <= order:
                term = B[j] @ A[i].t()
                if mut == "hi_lo_left_out" and (i, j) == (0, 1):
                    term[16:32] = 0.0
                acc += term
    return acc * torch.tensor(1.0 / scale)


def emu_plain(case, Ap, Bp, scale, mut=None):
    name, M, ncols, K, S, pad, _ = case
    buf = torch.full((S, ncols + 2, M + pad), float("nan"))
    for z, ks in enumerate(ref.split_ksteps(K, S)):
        m = mut if (mut == "hi_lo_left_out" or (mut == "k_step_left_out" and z == S - 1)) else None
        buf[z, 1:-1, :M] = emu_product(Ap, Bp, 2 if name == "gemm_nt3" else 1, scale, ks if S > 1 else None, m)
    if mut == "ldc_padding_written":
        buf[0, 1 + ncols // 2, M] = 1.0
    return buf


def emu_gx(case, Ap, Bp):
    C0, N, pairs, layout, K = case
    y = emu_product(Ap, Bp, 1).view(pairs, N, 32)[:, :, :C0]
    flat = torch.full((pairs * C0 * N + 2 * N,), float("nan"))
    flat[N:-N] = (y.permute(0, 2, 1) if layout == "dense" else y.permute(2, 0, 1)).reshape(-1)
    return flat


def _fill(buf, planes):
    for p in range(buf.n):
        buf.flat[cs.MARGIN + p * buf.stride:cs.MARGIN + p * buf.stride + buf.count] = planes[p].reshape(-1)


def emu_layer_fwd(case, Wp, Xp, scale, gamma, beta, slope, mut=None):
    """est_gemm_nt_kernel's EPI_IN epilogue in torch fp32: sums, the difference first, the biased variance, one fused multiply-add's worth of z."""
    _, M, pairs, K, absmax, keep = case
    ncols = pairs * KPTS
    y = emu_product(Wp, Xp, 1, scale)
    inv_n = torch.tensor(1.0 / KPTS)
    spans = [(p * KPTS, (p + 1) * KPTS) for p in range(pairs)]
    if mut == "next_block_in_pair_1":
        spans[1] = (100, 208)
    if mut == "lane_boundary_moved":
        spans[0], spans[1] = (0, 99), (99, 200)
    a = torch.empty(ncols, M)
    rstd = torch.empty(pairs, M)
    for p, (c0, c1) in enumerate(spans):
        mu = y[c0:c1].sum(0) * inv_n
        q = ((y[c0:c1] - mu) ** 2).sum(0)
        rstd[p] = 1.0 / torch.sqrt(q * inv_n + EPS)
        z = (y[p * KPTS:(p + 1) * KPTS] - mu) * (rstd[p] * gamma) + beta
        a[p * KPTS:(p + 1) * KPTS] = torch.where(z > 0, z, z * slope)
    out = cs.PlaneBuf(2, ncols, M, torch.float16, "cpu")
    out_b = cs.PlaneBuf(2, ncols, M, torch.bfloat16, "cpu")
    _fill(out, ref.host_planes_f16(a))
    if keep:
        _fill(out_b, ref.host_planes_bf16(a, 2))
    rb = cs.row_buf(pairs, M, "cpu")
    rb[1:-1] = rstd
    return out, out_b, rb


def emu_dgrad(case, WTp, dYnp, ap, rstd, gamma, beta, mut=None):
    """est_gemm_nt_kernel's EPI_INBWD epilogue in torch fp32."""
    _, M, pairs, K, slope = case
    ncols = pairs * KPTS
    dA = emu_product(WTp, dYnp, 1)
    a = ref.unblock((ap[0].float() + ap[1].float()).view(1, ncols, M))[0].float()
    islope = torch.tensor(1.0) / torch.tensor(slope)
    z = torch.where(a > 0, a, a * islope).view(pairs, KPTS, M)
    e = torch.where(a > 0, dA, dA * slope).view(pairs, KPTS, M)
    s1, S = e.sum(1), (e * z).sum(1)
    live = gamma.abs() > 1e-30
    ig = torch.where(live, 1.0 / torch.where(live, gamma, torch.ones_like(gamma)), torch.zeros_like(gamma))
    s2 = (S if mut == "no_beta_correction" else S - beta * s1) * ig
    inv_n = torch.tensor(1.0 / KPTS)
    k = rstd * gamma
    m1, m2g = s1 * inv_n, s2 * inv_n * ig
    c1, c0 = -k * m2g, k * (m2g * beta - m1)
    y = k[:, None, :] * e + (c1[:, None, :] * z + c0[:, None, :])
    dY = cs.PlaneBuf(2, ncols, M, torch.bfloat16, "cpu")
    _fill(dY, ref.host_planes_bf16(y.reshape(ncols, M), 2))
    dg, db = cs.row_buf(pairs, M, "cpu"), cs.row_buf(pairs, M, "cpu")
    dg[1:-1], db[1:-1] = s2, s1
    return dY, dg, db


def emu_tn(case, dYp, Xp, mut=None):
    Cout, Cin, ncols, slices = case
    A, B = f32(dYp), f32(Xp)
    part = torch.full((slices + 2, Cout, Cin), float("nan"))
    for s, (k0, k1) in enumerate(ref.tn_slices(ncols, slices)):
        if k1 <= k0:
            if mut != "empty_slice_left":
                part[1 + s] = 0.0
            continue
        part[1 + s] = (A[1, k0:k1].t() @ B[0, k0:k1] + A[0, k0:k1].t() @ B[1, k0:k1]) + A[0, k0:k1].t() @ B[0, k0:k1]
    return part


# ---- host planes of a case -----------------------------------------------------------------------------------------------------------
def plain_planes(case):
    A, B = cs.plain_inputs(case)
    if case[0] == "gemm_nt_f16":
        scale = ref.weight_scale(A.abs().max()) if case[6] else 1.0
        return ref.host_planes_f16(A, scale), ref.host_planes_f16(B), scale
    n = 3 if case[0] == "gemm_nt3" else 2
    return ref.host_planes_bf16(A, n), ref.host_planes_bf16(B, n), 1.0


def layer_planes(case):
    W, X, gamma, beta = cs.layer_fwd_inputs(case)
    scale = ref.weight_scale(W.abs().max()) if case[4] else 1.0
    return ref.host_planes_f16(W, scale), ref.host_planes_f16(X), scale, gamma, beta


def dgrad_planes(case):
    WT, dYn, a, rstd, gamma, beta = cs.dgrad_inputs(case)
    return ref.host_planes_bf16(WT, 2), ref.host_planes_bf16(dYn, 2), ref.host_planes_bf16(a, 2), rstd, gamma, beta


def run_plain(case, mut=None):
    Ap, Bp, scale = plain_planes(case)
    return cs.check_plain(case, Ap, Bp, scale, emu_plain(case, Ap, Bp, scale, mut))


def run_layer(case, mut=None):
    Wp, Xp, scale, gamma, beta = layer_planes(case)
    out, out_b, rb = emu_layer_fwd(case, Wp, Xp, scale, gamma, beta, 0.01, mut)
    return cs.check_layer_fwd(case, Wp, Xp, scale, gamma, beta, EPS, 0.01, out, out_b, rb)


def run_dgrad(case, mut=None):
    WTp, dYnp, ap, rstd, gamma, beta = dgrad_planes(case)
    dY, dg, db = emu_dgrad(case, WTp, dYnp, ap, rstd, gamma, beta, mut)
    return cs.check_dgrad(case, WTp, dYnp, ap, rstd, gamma, beta, dY, dg, db)[0]


def run_tn(case, mut=None):
    dYf, Xf = cs.tn_inputs(*case[:3])
    dYp, Xp = ref.host_planes_bf16(dYf, 2), ref.host_planes_bf16(Xf, 3)
    return cs.check_tn(case, dYp, Xp, emu_tn(case, dYp, Xp, mut))


# three shapes per entry point, a half-empty block (an odd pair count) and an M = 8 row block among them
HOST_PLAIN = [c for c in cs.PLAIN if c[1:4] in ((8, 200, 96), (40, 201, 160), (136, 208, 64))]
HOST_LAYER = [c for c in cs.LAYER_FWD if c[1:4] in ((32, 1, 32), (96, 2, 96), (128, 3, 32))]
HOST_DGRAD = [c for c in cs.DGRAD if c[1:4] in ((32, 1, 32), (128, 3, 32), (96, 3, 64))]
HOST_TN = [(96, 160, 31, 3), (32, 128, 100, 8), (160, 32, 33, 3)]


@pytest.mark.parametrize("case", HOST_PLAIN, ids=cs.case_id)
def test_fp32_evaluation_passes_plain(case):
    assert run_plain(case) <= ref.TOL


@pytest.mark.parametrize("case", cs.GX[:3], ids=cs.case_id)
def test_fp32_evaluation_passes_gx(case):
    A, B = cs.gx_inputs(case)
    Ap, Bp = ref.host_planes_bf16(A, 2), ref.host_planes_bf16(B, 2)
    assert cs.check_gx(case, Ap, Bp, emu_gx(case, Ap, Bp)) <= ref.TOL


@pytest.mark.parametrize("case", HOST_LAYER, ids=cs.case_id)
def test_fp32_evaluation_passes_layer_fwd(case):
    assert max(run_layer(case).values()) <= ref.TOL


@pytest.mark.parametrize("case", HOST_DGRAD, ids=cs.case_id)
def test_fp32_evaluation_passes_dgrad_in_bwd(case):
    assert max(run_dgrad(case).values()) <= ref.TOL


@pytest.mark.parametrize("case", HOST_TN, ids=cs.case_id)
def test_fp32_evaluation_passes_tn(case):
    assert run_tn(case) <= ref.TOL


def test_host_shapes_are_there():
    # three shapes for each two-plane product (the two split ones have no three-plane launch) and for each fused epilogue
    assert [sum(1 for c in HOST_PLAIN if c[0] == n) for n in ("gemm_nt_f16", "gemm_nt2", "gemm_nt3")] == [3, 3, 1]
    assert len(HOST_LAYER) == 3 and len(HOST_DGRAD) == 3


# ---- the mutations: each one alone is rejected -----------------------------------------------------------------------------------------
def _first(cases, name, kw):
    return next(c for c in cases if c[0] == name and all(c[i] == v for i, v in kw.items()))


MUTATIONS = [
    ("hi_lo_left_out", lambda m: run_plain(_first(cs.PLAIN, "gemm_nt2", {1: 136, 2: 208}), m)),
    ("k_step_left_out", lambda m: run_plain(_first(cs.PLAIN, "gemm_nt2", {1: 40, 2: 201}), m)),
    ("next_block_in_pair_1", lambda m: run_layer(_first(cs.LAYER_FWD, "layer_fwd", {1: 128, 2: 3}), m)),
    ("lane_boundary_moved", lambda m: run_layer(_first(cs.LAYER_FWD, "layer_fwd", {1: 96, 2: 2}), m)),
    ("no_beta_correction", lambda m: run_dgrad(_first(cs.DGRAD, "dgrad_in_bwd", {1: 128, 2: 3}), m)),
    ("ldc_padding_written", lambda m: run_plain(_first(cs.PLAIN, "gemm_nt_f16", {1: 8, 2: 200}), m)),
    ("empty_slice_left", lambda m: run_tn((32, 128, 100, 8), m)),
]


@pytest.mark.parametrize("name,run", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_each_mutation_is_rejected(name, run):
    run(None)  # the evaluation itself passes
    with pytest.raises(AssertionError):
        run(name)


# ---- the cap on undecided elements, over the whole matrix (the device test asserts it again on the device's planes) --------------------
@pytest.mark.parametrize("case", cs.LAYER_FWD, ids=cs.case_id)
def test_undecided_cap_layer_fwd(case):
    Wp, Xp, scale, gamma, beta = layer_planes(case)
    if not case[4]:
        cs.assert_planes_normal(Wp)
    cs.assert_planes_normal(Xp)
    cs.assert_undecided_cap(ref.layer_forward(Wp, Xp, scale, gamma, beta, EPS, 0.01)["undecided"], cs.case_id(case))


@pytest.mark.parametrize("case", cs.DGRAD, ids=cs.case_id)
def test_undecided_cap_dgrad_in_bwd(case):
    WTp, dYnp, ap, rstd, gamma, beta = dgrad_planes(case)
    cs.assert_undecided_cap(ref.fused_adjoint(WTp, dYnp, ap, rstd, gamma, beta, case[4])["undecided"], cs.case_id(case))


def test_matrix_reaches_both_builds_and_both_remap_states():
    """What est_gemm_cases asserts at import, once more where a report shows it."""
    for name, cases in (("gemm_nt_f16", cs.PLAIN), ("gemm_nt2", cs.PLAIN), ("layer_fwd", cs.LAYER_FWD), ("dgrad_in_bwd", cs.DGRAD)):
        assert {cs.geometry(c) for c in cases if c[0] == name} == {("small", False), ("small", True), ("full", False), ("full", True)}
    assert cs.workgroups(1024, 6400) == 256 and cs.build_of(1024, 6400) == "small" and cs.workgroups(1024, 6600) == 264
    assert cs.build_of(1024, 6600) == "full" and cs.remapped(6400) and not cs.remapped(6600)
    assert "DFEPE_EST_SMALL_GRID" not in os.environ
