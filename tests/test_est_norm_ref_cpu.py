"""The fp64 restatement of the estimator's any-N normalisation, adjoint, head and reduction kernels (tests/est_norm_ref.py) and the
checks of tests/est_norm_cases.py, on the host: the restatement against torch float64 instance_norm + leaky_relu and their autograd;
a torch fp32 evaluation of each kernel's chain (partials added in slice order, row sums of the kernel's depth, the Chan merge) through
every check_*() of the matrix -- the bounds admit a correct implementation --; mutations of that evaluation, each rejected on its own;
the cap on undecided elements over every forward case."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import est_norm_cases as cs  # noqa: E402
import est_norm_ref as ref  # noqa: E402

F = torch.nn.functional
EPS = cs.EPS
WORST = {}


def _note(entry, worst):
    WORST[entry] = max(WORST.get(entry, 0.0), worst)
    print(f"ESTNORM host {entry} worst={worst:.3f} (so far {WORST[entry]:.3f})")
    assert worst <= ref.TOL


# ---- the restatement against torch float64 ----------------------------------------------------------------------------------------
def _close(x, y):
    """Two float64 evaluations of O(1) quantities, element by element: 1e-12 of the element, or of one where it is smaller."""
    return bool(((x - y).abs() <= 1e-12 * (y.abs() + 1.0)).all())


@pytest.mark.parametrize("N,C,pairs,S,mode,slope", [(1, 32, 2, 1, "two_pass", 0.01), (37, 32, 3, 2, "two_pass", 0.01), (129, 64, 2, 5, ("chan", 7), 0.01),
                                                    (33, 32, 1, 1, ("chan", 64), 2.0), (257, 32, 2, 3, ("chan", 3), 0.01)])
def test_restatement_against_float64_torch(N, C, pairs, S, mode, slope):
    g = torch.Generator().manual_seed(N + C)
    ncols = pairs * N
    parts = torch.randn(S, ncols, C, generator=g) + 1.5
    gamma = ((1 + 0.2 * torch.randn(C, generator=g)) * cs._sign((C,), g)).double()
    beta = (0.3 * torch.randn(C, generator=g)).double()
    gamma[5] = 0.0
    r = ref.norm_forward(parts, N, gamma, beta, EPS, slope, mode)
    Y = parts.double().sum(0).view(pairs, N, C).permute(0, 2, 1).clone().requires_grad_(True)  # [pairs, C, N]
    gm, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    if N > 1:
        a = F.leaky_relu(F.instance_norm(Y, weight=gm, bias=bt, eps=EPS), slope)
        rstd = 1.0 / torch.sqrt(Y.detach().var(2, unbiased=False) + EPS)
    else:  # instance_norm refuses one point: the explicit formula (mean = y, variance 0)
        rstd = torch.full((pairs, C), EPS ** -0.5, dtype=torch.float64)
        a = F.leaky_relu((Y - Y.mean(2, keepdim=True)) * rstd[..., None] * gm[None, :, None] + bt[None, :, None], slope)
    a_cm = a.permute(0, 2, 1).reshape(ncols, C)
    assert not bool(r["undecided"].any())
    assert _close(r["a"], a_cm.detach()) and _close(r["rstd"], rstd)
    # the adjoint of the same activation (float64: nothing lost in planes) under an arbitrary upstream gradient, in S partials
    Gp = torch.randn(S, ncols, C, generator=g, dtype=torch.float64)
    G = Gp.sum(0)
    (a_cm * G).sum().backward()
    ad = ref.adjoint_n(Gp, a_cm.detach(), rstd, gamma, beta, slope, N)
    assert not bool(ad["undecided"].any())
    live = gamma != 0
    want = Y.grad.permute(0, 2, 1).reshape(ncols, C)
    if N > 1:
        assert _close(ad["dY"][:, live], want[:, live])
    else:  # one point: e - s1 / N - x^ s2 / N is 0 up to float64 rounding
        assert float(ad["dY"].abs().max()) < 1e-12 * float(G.abs().max()) and float(want.abs().max()) < 1e-12 * float(G.abs().max())
    assert float(ad["dY"][:, ~live].abs().max()) == 0.0 and float(want[:, ~live].abs().max()) < 1e-12
    assert _close(ad["dbeta_part"].sum(0), bt.grad)  # (the reference has no per-pair rows: the sum here, row by row in the checks)
    if N > 1:
        assert _close(ad["dgamma_part"].sum(0)[live], gm.grad[live])
    assert float(ad["dgamma_part"][:, ~live].abs().max()) == 0.0
    # per pair: each pair alone through autograd gives that pair's row
    if N > 1:
        p = pairs - 1
        Yp = Y.detach()[p:p + 1].clone()
        gp, bp = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        ap = F.leaky_relu(F.instance_norm(Yp, weight=gp, bias=bp, eps=EPS), slope)
        (ap.permute(0, 2, 1).reshape(N, C) * G[p * N:(p + 1) * N]).sum().backward()
        assert _close(ad["dgamma_part"][p][live], gp.grad[live]) and _close(ad["dbeta_part"][p], bp.grad)
    # the head's rank-one form is the same adjoint of dl w^T
    dl, wh = torch.randn(ncols, generator=g).double(), torch.randn(C, generator=g).double()
    h1 = ref.adjoint_n((dl, wh), a_cm.detach(), rstd, gamma, beta, slope, N)
    h2 = ref.adjoint_n((dl[:, None] * wh[None, :])[None], a_cm.detach(), rstd, gamma, beta, slope, N)
    assert torch.equal(h1["dY"], h2["dY"]) and torch.equal(h1["dgamma_part"], h2["dgamma_part"])
    # dgamma_zero: where gamma is 0 its value is the true d gamma of that channel, pair by pair
    x = torch.randn(ncols, 32, generator=g)
    W = torch.randn(C, 32, generator=g)
    xp = ref.host_planes_bf16(x, 2)
    yv = ref.stored_activation(xp) @ W.double().t()
    Yz = yv.view(pairs, N, C)
    rs = 1.0 / torch.sqrt(Yz.var(1, unbiased=False) + EPS) if N > 1 else torch.full((pairs, C), EPS ** -0.5, dtype=torch.float64)
    az = torch.randn(ncols, C, generator=g)
    value, _ = ref.dgamma_zero(("dA", G), ref.host_planes_bf16(az, 2), xp, W, rs, slope, N)
    xh = (Yz - Yz.mean(1, keepdim=True)) * rs[:, None, :]
    e = torch.where(ref.stored_activation(ref.host_planes_bf16(az, 2)) > 0, G, G * slope).view(pairs, N, C)
    assert _close(value, (e * xh).sum(1)) or N == 1


def test_plain_sums_are_the_sums():
    g = torch.Generator().manual_seed(1)
    a = torch.randn(17, 96, generator=g)
    w, bias, dl = torch.randn(96, generator=g), torch.randn(1, generator=g), torch.randn(17, generator=g)
    v, _ = ref.head_forward(ref.host_planes_f16(a), w, bias)
    assert _close(v, ref.f16_activation(ref.host_planes_f16(a)) @ w.double() + bias.double())
    ab = ref.stored_activation(ref.host_planes_bf16(a, 2))
    part, dpart, b, db = ref.head_dw(ref.host_planes_bf16(a, 2), dl, 20)
    assert ref.head_blocks(17, 20)[16:18] == [(16, 17), (17, 17)] and _close(part[:17], ab * dl.double()[:, None])
    assert float(part[17:].abs().max()) == 0.0 and float(dpart[17:].abs().max()) == 0.0 and float(db[17:].abs().max()) == 0.0
    assert _close(b[:17], dl.double())
    v, bd = ref.colsum(torch.randn(0, 5))
    assert float(v.abs().max()) == 0.0 and float(bd.abs().max()) == 0.0
    assert ref.split_rows(257, 64)[51:53] == [(255, 257), (260, 257)] and ref.split_rows(5, 7)[4:6] == [(4, 5), (5, 5)]
    assert cs.chain_r(128) == 19 and cs.chain_r(2048) == 34 and cs.chain_n(2500, 1) == 111 and cs.chain_n(33, 64) == 33


# ---- a torch fp32 evaluation of each chain ----------------------------------------------------------------------------------------
def ksum(T, rg, lds):
    """Sum over dim 1 of T [pairs, rows, C] as a workgroup of `rg` row groups does it: group g adds rows g, g + rg, ... in order, the
    rg / lds groups of a wavefront are added pairwise, the lds partials in order."""
    pairs, rows, C = T.shape
    chunks = -(-rows // rg)
    P = torch.zeros(pairs, chunks * rg, C)
    P[:, :rows] = T
    P = P.view(pairs, chunks, rg, C)
    acc = torch.zeros(pairs, rg, C)
    for c in range(chunks):
        acc = acc + P[:, c]
    acc = acc.view(pairs, lds, rg // lds, C)
    while acc.shape[2] > 1:
        acc = acc[:, :, 0::2] + acc[:, :, 1::2]
    out = torch.zeros(pairs, C)
    for q in range(lds):
        out = out + acc[:, q, 0]
    return out


def _geometry(case):
    if case[0] in ("norm_fwd_r", "in_bwd_r"):
        return 1024 // cs.template_r(case[1])[1], 16
    return (32, 32) if case[0] in ("norm_fwd", "in_bwd_n") else (8, 8)


def _fill(buf, planes):
    for p in range(buf.n):
        buf.flat[cs.MARGIN + p * buf.stride:cs.MARGIN + p * buf.stride + buf.count] = planes[p].reshape(-1)


def _slices(parts):
    y = parts[0].clone()
    for s in range(1, parts.shape[0]):
        y = y + parts[s]
    return y


def emu_norm_fwd(case, parts, gamma, beta, slope=0.01, mut=None):
    name, N, C, pairs = case[:4]
    keep = case[-1]
    splits = 1 if name == "norm_fwd_r" else case[4]
    rg, lds = _geometry(case)
    ncols = pairs * N
    Y = _slices(parts)[:, :C].reshape(pairs, N, C)
    inv_N = torch.tensor(1.0 / N)
    part_buf = None
    if splits == 1:
        mu = ksum(Y, rg, lds) * inv_N
        if mut == "one_pass_variance":
            q = ksum(Y * Y, rg, lds) - N * mu * mu
        else:
            q = ksum((Y - mu[:, None]) ** 2, rg, lds)
    else:
        live = [(a, b) for a, b in ref.split_rows(N, splits) if b > a]
        part_buf = cs.flat_buf(pairs * splits * 2 * C, "cpu")
        ws = torch.zeros(pairs, splits, 2, C)
        for t, (a, b) in enumerate(live):
            m = ksum(Y[:, a:b], rg, lds) * torch.tensor(1.0 / (b - a))
            ws[:, t, 0], ws[:, t, 1] = m, ksum((Y[:, a:b] - m[:, None]) ** 2, rg, lds)
        acc = torch.zeros(pairs, C)
        for t, (a, b) in enumerate(live):
            if not (mut == "last_split_dropped" and t == len(live) - 1):
                acc = acc + float(b - a) * ws[:, t, 0]
        mu = acc / float(N)
        q = torch.zeros(pairs, C)
        for t, (a, b) in enumerate(live):
            dm = ws[:, t, 0] - mu
            q = q + (ws[:, t, 1] + float(b - a) * dm * dm)
        cs.inside(part_buf)[:] = ws.reshape(-1)
        if mut == "workspace_cell_unwritten":
            cs.inside(part_buf)[-1] = float("nan")
    rstd = 1.0 / torch.sqrt(q * inv_N + EPS)
    z = (Y - mu[:, None]) * (rstd * gamma)[:, None] + beta
    a = torch.where(z > 0, z, z if mut == "no_slope" else z * slope).reshape(ncols, C)
    if mut == "ragged_group_unwritten":
        assert N % rg
        a.view(pairs, N, C)[:, N // rg * rg:] = float("nan")
    out, out_b = cs.PlaneBuf(2, ncols, C, torch.float16, "cpu"), cs.PlaneBuf(2, ncols, C, torch.bfloat16, "cpu")
    _fill(out, ref.host_planes_f16(a))
    if keep:
        _fill(out_b, ref.host_planes_bf16(a, 2))
    if mut == "margin_written":
        out.flat[cs.MARGIN + out.count + 3] = 1.0
    rb = cs.row_buf(pairs, C, "cpu")
    rb[1:-1] = rstd
    return out, out_b, rb, part_buf


def emu_in_bwd(case, up, ap, rstd, gamma, beta, mut=None):
    name = case[0]
    N, C = (case[1], case[2]) if name != "in_bwd" else (cs.KPTS, case[1])
    slope = case[-1]
    splits = case[4] if name == "in_bwd_n" else 1
    rg, lds = _geometry(case)
    ncols = ap.shape[1]
    pairs = ncols // N
    d = up[0][:, None] * up[1][None, :] if isinstance(up, tuple) else _slices(up)[:, :C]
    a = ref.unblock((ap[0].float() + ap[1].float()).view(1, ncols, C))[0].float()
    islope = torch.tensor(1.0) / torch.tensor(slope)
    z = torch.where(a > 0, a, a * islope)
    e = torch.where(a > 0, d, d * slope).view(pairs, N, C)
    livec = gamma.abs() > 1e-30
    ig = torch.where(livec, 1.0 / torch.where(livec, gamma, torch.ones_like(gamma)), torch.ones_like(gamma) if mut == "xhat_at_gamma_zero" else torch.zeros_like(gamma))
    x = ((z - beta) * ig).view(pairs, N, C)
    part_buf = None
    if splits == 1:
        s1, s2 = ksum(e, rg, lds), ksum(e * x, rg, lds)
    else:
        part_buf = cs.flat_buf(pairs * splits * 2 * C, "cpu")
        ws = torch.zeros(pairs, splits, 2, C)
        for t, (r0, r1) in enumerate(ref.split_rows(N, splits)):
            if r1 > r0:
                ws[:, t, 0], ws[:, t, 1] = ksum(e[:, r0:r1], rg, lds), ksum((e * x)[:, r0:r1], rg, lds)
        s1, s2 = torch.zeros(pairs, C), torch.zeros(pairs, C)
        for t in range(splits):
            s1, s2 = s1 + ws[:, t, 0], s2 + ws[:, t, 1]
        cs.inside(part_buf)[:] = ws.reshape(-1)
    inv_n = torch.tensor(1.0 / N)
    k = rstd * gamma
    y = k[:, None] * (e - (s1 * inv_n)[:, None] - x * (s2 * inv_n)[:, None])
    if mut == "ragged_group_unwritten":
        assert N % rg
        y[:, N // rg * rg:] = float("nan")
    dY = cs.PlaneBuf(2, ncols, C, torch.bfloat16, "cpu")
    _fill(dY, ref.host_planes_bf16(y.reshape(ncols, C), 2))
    if mut == "margin_written":
        dY.flat[3] = 0.5
    dg, db = cs.row_buf(pairs, C, "cpu"), cs.row_buf(pairs, C, "cpu")
    dg[1:-1], db[1:-1] = s2, s1
    if mut == "dgamma_rows_swapped":
        dg[1], dg[2] = s2[1], s2[0]
    return dY, dg, db, part_buf


def emu_head_fwd(case, ap, w, bias, mut=None):
    _, C, cols, _ = case
    t = ref.f16_activation(ap).float() * w[None, :]
    lanes = t.view(cols, C // 32, 16, 2)
    s = torch.zeros(cols, 16)
    for kb in range(C // 32):
        s = (s + lanes[:, kb, :, 0]) + lanes[:, kb, :, 1]
    while s.shape[1] > 1:
        s = s[:, 0::2] + s[:, 1::2]
    out = cs.flat_buf(cols, "cpu")
    cs.inside(out)[:] = s[:, 0] + (bias[0] if (bias is not None and mut != "bias_left_out") else 0.0)
    if mut == "last_column_unwritten":
        cs.inside(out)[-1] = float("nan")
    return out


def emu_head_dw(case, ap, dl, mut=None):
    _, C, cols, blocks, want_bias = case
    a = ref.stored_activation(ap).float()
    part, bias = cs.row_buf(blocks, C, "cpu"), cs.flat_buf(blocks, "cpu")
    for i, (c0, c1) in enumerate(ref.head_blocks(cols, blocks)):
        if c1 <= c0:
            if mut != "empty_block_nan":
                part[1 + i] = 0.0
            if want_bias:
                cs.inside(bias)[i] = 0.0
            continue
        part[1 + i] = ksum((a[c0:c1] * dl[c0:c1, None])[None], 8, 8)[0]
        if want_bias:
            hi = c1 - 1 if (mut == "bias_missing_column" and i == 0) else c1
            cs.inside(bias)[i] = ksum(dl[c0:hi].reshape(1, -1, 1), 8, 8)[0, 0] if hi > c0 else 0.0
    return part, bias


def emu_colsum(launch, srcs, mut=None):
    dsts = []
    for (rows, cols), src in zip(launch, srcs):
        if mut == "last_row_left_out" and rows > 32:
            src = src[:-1]
        dst = cs.flat_buf(cols, "cpu")
        if rows <= 32:
            s = torch.zeros(cols)
            for r in range(rows):
                s = s + src[r]
        else:
            s = ksum(src[None], 16, 16)[0]
        cs.inside(dst)[:] = s
        dsts.append(dst)
    return dsts


def emu_dgamma_zero(case, up, ap_out, ap_in, W, rstd, gamma, Ci=cs.ZERO_CI, mut=None):
    _, N, pairs, form = case
    a, x = ref.stored_activation(ap_out).float(), ref.stored_activation(ap_in).float()
    C = a.shape[1]
    y = (x[:, :Ci] @ W[:, :Ci].t()).view(pairs, N, C)
    mean = ksum(y, 256, 4) / float(N)
    xh = (y - mean[:, None]) * rstd[:, None]
    if form == "dA":
        d = up[1]
    elif form == "head":
        d = up[1][:, None] * up[2][None, :]
    else:
        d = ref.stored_activation(up[1]).float() @ up[2]
    e = torch.where(a > 0, d, d * 0.01).view(pairs, N, C)
    dg = cs.row_buf(pairs, C, "cpu")
    dead = gamma.abs() <= (1e-28 if mut == "threshold_moved" else 1e-30)
    if mut == "mean_left_in":
        xh = y * rstd[:, None]
    dg[1:-1][:, dead] = ksum(e * xh, 256, 4)[:, dead]
    return dg


# ---- every case of the matrix through its check ------------------------------------------------------------------------------------
def run_norm(case, mut=None):
    parts, gamma, beta = cs.fwd_inputs(case)
    out, out_b, rb, pb = emu_norm_fwd(case, parts, gamma, beta, 0.01, mut)
    return cs.check_norm_fwd(case, parts, gamma, beta, 0.01, out, out_b, rb, pb)


def run_bwd(case, mut=None):
    up, a, rstd, gamma, beta = cs.bwd_inputs(case)
    ap = ref.host_planes_bf16(a, 2)
    dY, dg, db, pb = emu_in_bwd(case, up, ap, rstd, gamma, beta, mut)
    return cs.check_in_bwd(case, up, ap, rstd, gamma, beta, dY, dg, db, pb)


def run_head_dw(case, mut=None):
    a, _, _, dl = cs.head_inputs(case)
    ap = ref.host_planes_bf16(a, 2)
    part, bias = emu_head_dw(case, ap, dl, mut)
    return cs.check_head_dw(case, ap, dl, part, bias)


@pytest.mark.parametrize("case", cs.NORM_R + cs.NORM_N, ids=cs.case_id)
def test_fp32_evaluation_passes_norm_forward(case):
    _note(case[0], max(run_norm(case).values()))


@pytest.mark.parametrize("case", cs.INBWD_R + cs.INBWD_N + cs.INBWD_100, ids=cs.case_id)
def test_fp32_evaluation_passes_adjoint(case):
    _note(case[0], max(run_bwd(case).values()))


def run_head_fwd(case, mut=None):
    a, w, bias, _ = cs.head_inputs(case)
    ap = ref.host_planes_f16(a)
    bias = bias if case[3] else None
    return cs.check_head_fwd(case, ap, w, bias, emu_head_fwd(case, ap, w, bias, mut))


@pytest.mark.parametrize("case", cs.HEAD_FWD, ids=cs.case_id)
def test_fp32_evaluation_passes_head_fwd(case):
    _note("head_fwd", run_head_fwd(case))


@pytest.mark.parametrize("case", cs.HEAD_DW, ids=cs.case_id)
def test_fp32_evaluation_passes_head_dw(case):
    _note("head_dw", max(run_head_dw(case).values()))


def run_colsum(launch, mut=None):
    srcs = cs.colsum_inputs(launch)
    return cs.check_colsum(launch, srcs, emu_colsum(launch, srcs, mut))


@pytest.mark.parametrize("launch", cs.COLSUM, ids=lambda l: f"{len(l)}seg")
def test_fp32_evaluation_passes_colsum(launch):
    _note("colsum", run_colsum(launch))


def run_zero(case, mut=None):
    up, a, x, W, rstd, gamma = cs.zero_inputs(case)
    ap_out, ap_in = ref.host_planes_bf16(a, 2), ref.host_planes_bf16(x, 2)
    if case[3] == "next":
        up = ("next", ref.host_planes_bf16(up[1], 2), up[2])
    return cs.check_dgamma_zero(case, up, ap_out, ap_in, W, rstd, gamma, emu_dgamma_zero(case, up, ap_out, ap_in, W, rstd, gamma, mut=mut))


@pytest.mark.parametrize("case", cs.DGAMMA_ZERO, ids=cs.case_id)
def test_fp32_evaluation_passes_dgamma_zero(case):
    _note("dgamma_zero", run_zero(case))


# ---- the mutations: each one alone is rejected -------------------------------------------------------------------------------------
def _pick(cases, **kw):
    idx = {"N": 1, "C": 2, "pairs": 3, "splits": 4}
    return next(c for c in cases if all(c[idx[k]] == v for k, v in kw.items()))


MUTATIONS = [
    ("dgamma_rows_swapped", lambda m: run_bwd(_pick(cs.INBWD_R, N=1024, pairs=3), m)),
    ("dgamma_rows_swapped", lambda m: run_bwd(_pick(cs.INBWD_N, N=2500, splits=64), m)),
    ("ragged_group_unwritten", lambda m: run_norm(_pick(cs.NORM_R, N=65), m)),
    ("ragged_group_unwritten", lambda m: run_bwd(_pick(cs.INBWD_R, N=1025), m)),
    ("ragged_group_unwritten", lambda m: run_norm(_pick(cs.NORM_N, N=33, splits=2), m)),
    ("last_split_dropped", lambda m: run_norm(_pick(cs.NORM_N, N=257, splits=64), m)),
    ("workspace_cell_unwritten", lambda m: run_norm(_pick(cs.NORM_N, N=129, splits=3), m)),
    ("one_pass_variance", lambda m: run_norm(_pick(cs.NORM_R, N=63), m)),
    ("one_pass_variance", lambda m: run_norm(_pick(cs.NORM_N, N=32, splits=1), m)),
    ("no_slope", lambda m: run_norm(_pick(cs.NORM_R, N=512), m)),
    ("xhat_at_gamma_zero", lambda m: run_bwd(_pick(cs.INBWD_R, N=64), m)),
    ("xhat_at_gamma_zero", lambda m: run_bwd(cs.INBWD_100[1], m)),
    ("margin_written", lambda m: run_norm(_pick(cs.NORM_R, N=2), m)),
    ("margin_written", lambda m: run_bwd(_pick(cs.INBWD_N, N=5), m)),
    ("empty_block_nan", lambda m: run_head_dw(next(c for c in cs.HEAD_DW if c[3] == c[2] + 3 and c[2] == 17), m)),
    ("bias_missing_column", lambda m: run_head_dw(next(c for c in cs.HEAD_DW if c[4] and c[2] == 700 and c[3] == 8), m)),
    ("bias_left_out", lambda m: run_head_fwd(next(c for c in cs.HEAD_FWD if c[3] and c[2] == 17), m)),
    ("last_column_unwritten", lambda m: run_head_fwd(next(c for c in cs.HEAD_FWD if c[2] == 17), m)),
    ("last_row_left_out", lambda m: run_colsum(cs.COLSUM[1], m)),
    ("threshold_moved", lambda m: run_zero(cs.DGAMMA_ZERO[3], m)),
    ("mean_left_in", lambda m: run_zero(cs.DGAMMA_ZERO[5], m)),
]


@pytest.mark.parametrize("name,run", MUTATIONS, ids=[f"{m[0]}-{i}" for i, m in enumerate(MUTATIONS)])
def test_each_mutation_is_rejected(name, run):
    run(None)  # the evaluation itself passes
    with pytest.raises(AssertionError):
        run(name)


# ---- the cap on undecided elements, over every forward case (the device test asserts it again) ----------------------------------------
@pytest.mark.parametrize("case", cs.NORM_R + cs.NORM_N, ids=cs.case_id)
def test_undecided_cap_forward(case):
    name, N, C, pairs = case[:4]
    parts, gamma, beta = cs.fwd_inputs(case)
    mode = "two_pass" if name == "norm_fwd_r" or case[4] == 1 else ("chan", case[4])
    r = ref.norm_forward(parts[:, :, :C], N, gamma, beta, EPS, 0.01, mode, cs.chain_of(case))
    cs.assert_undecided_cap(r["undecided"], cs.case_id(case))
    # the inputs are what the matrix promises: a pair close to eps, a constant channel, the rest 40 +- 3
    y = parts.double().sum(0)[:, :C].view(pairs, N, C)
    if N > 1:
        var = y.var(1, unbiased=False)
        assert float(var[0, 7]) == 0.0
        near = var[pairs - 1, C // 2:]
        assert bool(((near > EPS / 4) & (near < EPS * 4)).all()) or N < 8
        assert float(y.mean()) > 39.0


# ---- inorm_lrelu: an fp32 evaluation of inorm.hip's two kernels through check_inorm ------------------------------------------------------
def emu_inorm(case, Y, gamma, beta, G, slope=0.01, mut=None):
    _, N, C, R = case
    rows = C * R
    y, gA = Y.reshape(rows, N), G.reshape(rows, N)
    gm, bt = gamma.view(C, 1).expand(C, R).reshape(rows, 1), beta.view(C, 1).expand(C, R).reshape(rows, 1)
    rsum = lambda t: ksum(t.t().reshape(1, N, rows), 16, 16)[0][:, None]  # sixteen lanes per row
    mean = rsum(y) / float(N)
    var = (rsum(y * y) / float(N) - mean * mean) if mut == "one_pass_variance" else rsum((y - mean) ** 2) / float(N)
    rstd = 1.0 / torch.sqrt(var + EPS)
    z = (y - mean) * (gm * rstd) + bt
    A = torch.where(z > 0, z, z * slope)
    xh = (y - mean) * rstd
    e = torch.where(xh * gm + bt > 0, gA, gA * slope)
    s1, s2 = rsum(e), rsum(e * xh)
    gY = (gm * rstd) * (e - s1 / float(N) - xh * (s2 / float(N)))
    gg, gb = s2.view(C, R), s1.view(C, R)
    if mut == "rows_of_next_channel" and C > 1:
        gg = gg.roll(1, 0)
    return A.view(C, R, N), torch.cat([mean, rstd], 1), gY.view(C, R, N), gg.sum(1), gb.sum(1)


def run_inorm(case, mut=None):
    Y, gamma, beta, G = cs.inorm_inputs(case)
    A, stats, gY, gg, gb = emu_inorm(case, Y, gamma, beta, G, 0.01, mut)
    return cs.check_inorm(case, Y, gamma, beta, 0.01, A, stats, G, gY, gg, gb)


@pytest.mark.parametrize("case", cs.INORM, ids=cs.case_id)
def test_fp32_evaluation_passes_inorm(case):
    _note("inorm_lrelu", max(run_inorm(case).values()))


@pytest.mark.parametrize("mut,case", [("one_pass_variance", ("inorm", 8, 17, 1)), ("rows_of_next_channel", ("inorm", 132, 3, 5))])
def test_inorm_mutations_are_rejected(mut, case):
    assert case in cs.INORM
    run_inorm(case)
    with pytest.raises(AssertionError):
        run_inorm(case, mut)
