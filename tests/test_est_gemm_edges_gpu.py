"""Every entry point of csrc/est_gemm.hip's matrix-core kernels on the device, over the case matrix of tests/est_gemm_cases.py
and through its check(): each element against the fp64 restatement of tests/est_gemm_ref.py (evaluated on the device's own
planes, read back after dfepe_est_split / dfepe_est_split_f16 / dfepe_est_absmax), within TOL times its own first-order bound; NaN
pre-filled outputs with margins; a second call on the same inputs bit for bit.  The matrix holds both builds of every two-plane
entry point (AHEAD = 2 up to 256 workgroups, the default build above), with and without the XCD remap in each.  Each test prints the
worst |got - value| / bound it saw; DESIGN.md's table is taken from those lines."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import est_gemm_cases as cs  # noqa: E402
import est_gemm_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KPTS = ref.KPTS
EPS = 1e-5


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _split(dfepe, src, n_planes):
    src = src.to(DEV).contiguous()
    return dfepe.estimator._split(src, src.shape[0], src.shape[1], src.shape[1], n_planes)


def _split_f16(dfepe, src, scaled):
    """(planes, absmax word or None, scale): the weights' path when scaled (dfepe_est_absmax + dfepe_est_split_f16)."""
    src = src.to(DEV).contiguous()
    word, scale = None, 1.0
    if scaled:
        word = torch.zeros(1, device=DEV, dtype=torch.int32)
        assert dfepe._lib.lib().dfepe_est_absmax(src.data_ptr(), src.numel(), word.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert word.view(torch.float32).item() == src.abs().max().item()
        scale = ref.weight_scale(word.view(torch.float32).item())
    return dfepe.estimator._split_f16(src, src.shape[0], src.shape[1], src.shape[1], word), word, scale


def _wp(word):
    return None if word is None else word.data_ptr()


def _report(entry, case, geometry, worst):
    build, remap = geometry
    print(f"ESTGEMM {entry} build={build} remapped={int(remap)} case={cs.case_id(case)} worst={worst:.3f}")
    assert worst <= ref.TOL


def test_host_planes_are_the_device_planes(dfepe):
    """The host test (tests/test_est_gemm_ref_cpu.py) builds its planes with est_gemm_ref.host_planes_*: the same bits as the device
    splits leave, so what it establishes about the matrix (the cap on undecided elements, no subnormal plane) holds here too."""
    case = cs.LAYER_FWD[0]
    W, X, _, _ = cs.layer_fwd_inputs(case)
    Wp, _, scale = _split_f16(dfepe, W, True)
    assert torch.equal(_bits(Wp.cpu()), _bits(ref.host_planes_f16(W, scale)))
    assert torch.equal(_bits(_split_f16(dfepe, X, False)[0].cpu()), _bits(ref.host_planes_f16(X)))
    a = cs.dgrad_inputs(cs.DGRAD[0])[2]
    for n in (2, 3):
        assert torch.equal(_bits(_split(dfepe, a, n).cpu()), _bits(ref.host_planes_bf16(a, n)))


# ---- plain products --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cs.PLAIN, ids=cs.case_id)
def test_plain_products(dfepe, case):
    lib = dfepe._lib.lib()
    name, M, ncols, K, S, pad, scaled = case
    A, B = cs.plain_inputs(case)
    if name == "gemm_nt_f16":
        (Ap, word, scale), (Bp, _, _) = _split_f16(dfepe, A, scaled), _split_f16(dfepe, B, False)
        if not scaled:
            cs.assert_planes_normal(Ap)
        cs.assert_planes_normal(Bp)
    else:
        n = 3 if name == "gemm_nt3" else 2
        Ap, Bp, word, scale = _split(dfepe, A, n), _split(dfepe, B, n), None, 1.0
    ldc, stride = M + pad, (ncols + 2) * (M + pad)

    def call():
        buf = torch.full((S, ncols + 2, ldc), float("nan"), device=DEV)
        out = buf[0, 1].data_ptr()
        a = (Ap.data_ptr(), M * K, Bp.data_ptr(), ncols * K, M, ncols, K)
        if name == "gemm_nt_f16":
            rc = lib.dfepe_est_gemm_nt_f16(*a, _wp(word), out, ldc, None) if S == 1 else \
                lib.dfepe_est_gemm_nt_f16_splitk(*a, _wp(word), out, ldc, S, stride, None)
        elif S == 1:
            rc = lib.dfepe_est_gemm_nt(*a, 3 if name == "gemm_nt3" else 2, out, ldc, None)
        else:
            rc = lib.dfepe_est_gemm_nt_splitk(*a, out, ldc, S, stride, None)
        assert rc == 0
        torch.cuda.synchronize()
        return buf

    buf = call()
    worst = cs.check_plain(case, Ap, Bp, scale, buf)
    assert torch.equal(_bits(call()), _bits(buf))
    geometry = ("one", cs.remapped(ncols)) if name == "gemm_nt3" else cs.geometry(case)
    _report(name, case, geometry, worst)


@pytest.mark.parametrize("case", cs.GX, ids=cs.case_id)
def test_input_gradient_store(dfepe, case):
    lib = dfepe._lib.lib()
    C0, N, pairs, layout, K = case
    ncols = pairs * N
    A, B = cs.gx_inputs(case)
    Ap, Bp = _split(dfepe, A, 2), _split(dfepe, B, 2)
    sb, sc = cs.gx_strides(case)

    def call():
        flat = torch.full((pairs * C0 * N + 2 * N,), float("nan"), device=DEV)
        assert lib.dfepe_est_gemm_nt_gx(Ap.data_ptr(), 32 * K, Bp.data_ptr(), ncols * K, 32, ncols, K, flat[N:].data_ptr(), C0, N, sb, sc, None) == 0
        torch.cuda.synchronize()
        return flat

    flat = call()
    worst = cs.check_gx(case, Ap, Bp, flat)
    assert torch.equal(_bits(call()), _bits(flat))
    _report("gemm_nt_gx", case, (cs.build_of(32, ncols), cs.remapped(ncols)), worst)


# ---- the fused epilogues -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cs.LAYER_FWD, ids=cs.case_id)
def test_layer_forward(dfepe, case):
    lib = dfepe._lib.lib()
    _, M, pairs, K, absmax, keep = case
    ncols, slope = pairs * KPTS, 0.01
    W, X, gamma, beta = cs.layer_fwd_inputs(case)
    (Wp, word, scale), (Xp, _, _) = _split_f16(dfepe, W, absmax), _split_f16(dfepe, X, False)
    gd, bd = gamma.to(DEV), beta.to(DEV)

    def call():
        out = cs.PlaneBuf(2, ncols, M, torch.float16, DEV)
        out_b = cs.PlaneBuf(2, ncols, M, torch.bfloat16, DEV)
        rb = cs.row_buf(pairs, M, DEV)
        rc = lib.dfepe_est_layer_fwd(Wp.data_ptr(), M * K, Xp.data_ptr(), ncols * K, M, ncols, K, _wp(word), gd.data_ptr(), bd.data_ptr(), EPS, slope,
                                     out.first().data_ptr(), out.stride, out_b.first().data_ptr() if keep else None, out_b.stride,
                                     rb[1].data_ptr(), None)
        assert rc == 0
        torch.cuda.synchronize()
        return out, out_b, rb

    out, out_b, rb = call()
    worst = cs.check_layer_fwd(case, Wp, Xp, scale, gd, bd, EPS, slope, out, out_b, rb)
    out2, out_b2, rb2 = call()
    assert torch.equal(_bits(out2.flat), _bits(out.flat)) and torch.equal(_bits(out_b2.flat), _bits(out_b.flat)) and torch.equal(_bits(rb2), _bits(rb))
    print("ESTGEMM layer_fwd parts", {k: round(v, 3) for k, v in worst.items()})
    _report("layer_fwd", case, cs.geometry(case), max(worst.values()))


@pytest.mark.parametrize("case", cs.DGRAD, ids=cs.case_id)
def test_fused_data_gradient_and_adjoint(dfepe, case):
    lib = dfepe._lib.lib()
    _, M, pairs, K, slope = case
    ncols = pairs * KPTS
    WT, dYn, a, rstd, gamma, beta = cs.dgrad_inputs(case)
    WTp, dYnp, ap = _split(dfepe, WT, 2), _split(dfepe, dYn, 2), _split(dfepe, a, 2)
    rd, gd, bd = rstd.to(DEV), gamma.to(DEV), beta.to(DEV)

    def call():
        dY = cs.PlaneBuf(2, ncols, M, torch.bfloat16, DEV)
        dg, db = cs.row_buf(pairs, M, DEV), cs.row_buf(pairs, M, DEV)
        rc = lib.dfepe_est_dgrad_in_bwd(WTp.data_ptr(), M * K, dYnp.data_ptr(), ncols * K, M, ncols, K, ap.data_ptr(), ncols * M, rd.data_ptr(),
                                        gd.data_ptr(), bd.data_ptr(), slope, dY.first().data_ptr(), dY.stride, dg[1].data_ptr(), db[1].data_ptr(), None)
        assert rc == 0
        torch.cuda.synchronize()
        return dY, dg, db

    dY, dg, db = call()
    worst, r = cs.check_dgrad(case, WTp, dYnp, ap, rd, gd, bd, dY, dg, db)
    dY2, dg2, db2 = call()
    assert torch.equal(_bits(dY2.flat), _bits(dY.flat)) and torch.equal(_bits(dg2), _bits(dg)) and torch.equal(_bits(db2), _bits(db))
    # and against the two launches it replaces, on the same planes: both are held by the same bounds, so they differ by at most their sum
    dA = torch.full((ncols, M), float("nan"), device=DEV)
    assert lib.dfepe_est_gemm_nt(WTp.data_ptr(), M * K, dYnp.data_ptr(), ncols * K, M, ncols, K, 2, dA.data_ptr(), M, None) == 0
    tY = cs.PlaneBuf(2, ncols, M, torch.bfloat16, DEV)
    tg, tb = cs.row_buf(pairs, M, DEV), cs.row_buf(pairs, M, DEV)
    assert lib.dfepe_est_in_bwd(dA.data_ptr(), None, None, ap.data_ptr(), ncols * M, rd.data_ptr(), gd.data_ptr(), bd.data_ptr(), slope, M, ncols,
                                tY.first().data_ptr(), tY.stride, tg[1].data_ptr(), tb[1].data_ptr(), None) == 0
    torch.cuda.synchronize()
    ref.compare(dA, r["dA"], r["dA_bound"], "dA of the two launches")
    two = {"dY": ref.compare(cs.planes_value(dY.planes()), cs.planes_value(tY.planes()), 2 * r["dY_bound"], "dY against the two launches"),
           "dgamma": ref.compare(dg[1:-1], tg[1:-1], 2 * r["dgamma_bound"], "d gamma against the two launches"),
           "dbeta": ref.compare(db[1:-1], tb[1:-1], 2 * r["dbeta_bound"], "d beta against the two launches")}
    print("ESTGEMM dgrad_in_bwd parts", {k: round(v, 3) for k, v in worst.items()}, "two launches (of the summed bound)", {k: round(v, 3) for k, v in two.items()})
    _report("dgrad_in_bwd", case, cs.geometry(case), max(worst.values()))


# ---- the weight gradient -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cs.TN, ids=cs.case_id)
def test_weight_gradient_partials(dfepe, case):
    lib = dfepe._lib.lib()
    Cout, Cin, ncols, slices = case
    dYf, Xf = cs.tn_inputs(Cout, Cin, ncols)
    dYp, Xp = _split(dfepe, dYf, 2), _split(dfepe, Xf, 3)

    def call():
        part = torch.full((slices + 2, Cout, Cin), float("nan"), device=DEV)
        assert lib.dfepe_est_gemm_tn(dYp.data_ptr(), ncols * Cout, Cout, Xp.data_ptr(), ncols * Cin, Cin, ncols, slices, part[1].data_ptr(), None) == 0
        torch.cuda.synchronize()
        return part

    part = call()
    worst = cs.check_tn(case, dYp, Xp, part)
    assert torch.equal(_bits(call()), _bits(part))
    _report("gemm_tn", case, ("one", slices % 8 == 0), worst)


@pytest.mark.parametrize("ncols,layers", cs.TN_MULTI, ids=lambda v: str(v) if isinstance(v, int) else "x".join(str(s) for _, _, s in v))
def test_weight_gradient_table(dfepe, ncols, layers):
    """Layers of different slice counts in one launch: their block counts are padded to multiples of eight, differently each."""
    lib = dfepe._lib.lib()
    n = len(layers)
    planes = []
    for i, (Cout, Cin, slices) in enumerate(layers):
        dYf, Xf = cs.tn_inputs(Cout, Cin, ncols, salt=i)
        planes.append((_split(dfepe, dYf, 2), _split(dfepe, Xf, 3)))
    blocks = [-(-co // 128) * -(-ci // 128) * s for co, ci, s in layers]
    assert len({-b % 8 for b in blocks}) > 1  # the padding differs between the layers

    def call():
        parts = [torch.full((s + 2, co, ci), float("nan"), device=DEV) for co, ci, s in layers]
        ptrs = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
        sizes = lambda vs: (ctypes.c_size_t * n)(*vs)
        ints = lambda vs: (ctypes.c_int * n)(*vs)
        rc = lib.dfepe_est_gemm_tn_multi(n, ptrs([p[0] for p in planes]), sizes([ncols * co for co, _, _ in layers]), ints([co for co, _, _ in layers]),
                                         ptrs([p[1] for p in planes]), sizes([ncols * ci for _, ci, _ in layers]), ints([ci for _, ci, _ in layers]),
                                         ncols, ints([s for _, _, s in layers]), ptrs([p[1] for p in parts]), None)
        assert rc == 0
        torch.cuda.synchronize()
        return parts

    parts = call()
    worst = max(cs.check_tn((co, ci, ncols, s), dYp, Xp, part) for (co, ci, s), (dYp, Xp), part in zip(layers, planes, parts))
    for p, q in zip(call(), parts):
        assert torch.equal(_bits(p), _bits(q))
    _report("gemm_tn_multi", (ncols,) + tuple(s for _, _, s in layers), ("one", False), worst)
