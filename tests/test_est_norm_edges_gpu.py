"""The estimator's any-N normalisation, adjoint, head and reduction entry points (csrc/est_norm.hip, est_planes.hip) on the device, over the case matrix
of tests/est_norm_cases.py and through its check_*(): each element against the fp64 restatement of tests/est_norm_ref.py, within TOL
times its own first-order bound; NaN pre-filled outputs and `part` workspaces with margins; per-pair and per-block partials row by row;
a second call on the same inputs bit for bit; refused arguments leave the outputs untouched.  Each test prints
`ESTNORM <entry> case=<id> worst=<ratio>`; DESIGN.md's table is taken from those lines."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import est_norm_cases as cs  # noqa: E402
import est_norm_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = cs.EPS
SLOPE = 0.01
INVALID = -1  # DFEPE_ERR_INVALID_ARG


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    """Two runs' buffers (PlaneBuf, tensor or None), bit for bit."""
    for x, y in zip(a, b):
        if x is None:
            assert y is None
            continue
        x, y = (x.flat, y.flat) if isinstance(x, cs.PlaneBuf) else (x, y)
        assert torch.equal(_bits(x), _bits(y))


def _split(dfepe, src, n_planes=2):
    src = src.to(DEV).contiguous()
    return dfepe.estimator._split(src, src.shape[0], src.shape[1], src.shape[1], n_planes)


def _split_f16(dfepe, src):
    src = src.to(DEV).contiguous()
    return dfepe.estimator._split_f16(src, src.shape[0], src.shape[1], src.shape[1], None)


def _p(t):
    return None if t is None else t.data_ptr()


def _report(entry, case, worst):
    worst = max(worst.values()) if isinstance(worst, dict) else worst
    print(f"ESTNORM {entry} case={cs.case_id(case) if isinstance(case, tuple) else case} worst={worst:.3f}")
    assert worst <= ref.TOL


def test_host_planes_are_the_device_planes(dfepe):
    """The host test builds the adjoints' planes with host_planes_bf16 and the head's with host_planes_f16: the bits the device splits
    leave, tiny and zero activations included."""
    _, a, _, _, _ = cs.bwd_inputs(cs.INBWD_R[3])
    assert torch.equal(_bits(_split(dfepe, a).cpu()), _bits(ref.host_planes_bf16(a, 2)))
    a = cs.head_inputs(cs.HEAD_FWD[3])[0]
    assert torch.equal(_bits(_split_f16(dfepe, a).cpu()), _bits(ref.host_planes_f16(a)))


# ---- forward ---------------------------------------------------------------------------------------------------------------------
def _forward(dfepe, case, N=None, splits=None, with_part=True):
    """One call of the case's forward entry point on fresh NaN buffers; N / splits override the case's (refusals).  Returns rc and buffers."""
    lib = dfepe._lib.lib()
    name, N0, C, pairs = case[:4]
    keep = case[-1]
    parts, gamma, beta = (t.to(DEV) for t in cs.fwd_inputs(case))
    ncols, ld = pairs * N0, parts.shape[2]
    out, out_b = cs.PlaneBuf(2, ncols, C, torch.float16, DEV), cs.PlaneBuf(2, ncols, C, torch.bfloat16, DEV)
    rb = cs.row_buf(pairs, C, DEV)
    pb = None
    if name == "norm_fwd_r":
        rc = lib.dfepe_est_norm_fwd_r(parts.data_ptr(), ld, case[4], ncols * ld, C, pairs, N0 if N is None else N, gamma.data_ptr(), beta.data_ptr(), EPS,
                                      SLOPE, out.first().data_ptr(), out.stride, out_b.first().data_ptr() if keep else None, out_b.stride,
                                      rb[1].data_ptr(), None)
    else:
        S = case[4] if splits is None else splits
        pb = cs.flat_buf(pairs * max(case[4], 1) * 2 * C, DEV) if case[4] > 1 or splits is not None else None
        rc = lib.dfepe_est_norm_fwd(parts.data_ptr(), ld, C, pairs, N0, gamma.data_ptr(), beta.data_ptr(), EPS, SLOPE, out.first().data_ptr(), out.stride,
                                    out_b.first().data_ptr() if keep else None, out_b.stride, rb[1].data_ptr(), S,
                                    cs.inside(pb).data_ptr() if (pb is not None and with_part) else None, None)
    torch.cuda.synchronize()
    return rc, (parts, gamma, beta), (out, out_b, rb, pb)


@pytest.mark.parametrize("case", cs.NORM_R + cs.NORM_N, ids=cs.case_id)
def test_norm_forward(dfepe, case):
    rc, (parts, gamma, beta), bufs = _forward(dfepe, case)
    assert rc == 0
    worst = cs.check_norm_fwd(case, parts, gamma, beta, SLOPE, *bufs)
    rc2, _, bufs2 = _forward(dfepe, case)
    assert rc2 == 0
    _same(bufs2, bufs)
    print("ESTNORM", case[0], "parts", {k: round(v, 3) for k, v in worst.items()})
    _report(case[0], case, worst)


def _untouched(bufs):
    for b in bufs:
        if isinstance(b, cs.PlaneBuf):
            b.assert_untouched("a refused call")
        elif b is not None:
            assert bool(torch.isnan(b).all()), "a refused call wrote"


def test_norm_forward_refusals(dfepe):
    """N = 0 and N = 2049 (register-resident), splits = 0, 65 and splits > 1 without `part` (strided): refused, every output still NaN."""
    case = next(c for c in cs.NORM_R if c[1] == 64)
    for N in cs.R_REFUSED:
        rc, _, bufs = _forward(dfepe, case, N=N)
        assert rc == INVALID
        _untouched(bufs)
    case = next(c for c in cs.NORM_N if c[1] == 129)
    for splits, with_part in [(s, True) for s in cs.N_REFUSED_SPLITS] + [(3, False)]:
        rc, _, bufs = _forward(dfepe, case, splits=splits, with_part=with_part)
        assert rc == INVALID
        _untouched(bufs)


# ---- the adjoints ----------------------------------------------------------------------------------------------------------------
def _backward(dfepe, case, N=None, splits=None, with_part=True):
    lib = dfepe._lib.lib()
    name = case[0]
    up, a, rstd, gamma, beta = cs.bwd_inputs(case)
    ncols, C = a.shape
    head, slope = isinstance(up, tuple), case[-1]
    ap = _split(dfepe, a)
    up = tuple(t.to(DEV) for t in up) if head else up.to(DEV)
    rstd, gamma, beta = rstd.to(DEV), gamma.to(DEV), beta.to(DEV)
    dA, dl, wh = (None, up[0], up[1]) if head else (up, None, None)
    dY = cs.PlaneBuf(2, ncols, C, torch.bfloat16, DEV)
    pairs = rstd.shape[0]
    dg, db = cs.row_buf(pairs, C, DEV), cs.row_buf(pairs, C, DEV)
    pb = None
    tail = (ap.data_ptr(), ncols * C, rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), slope, C)
    outs = (dY.first().data_ptr(), dY.stride, dg[1].data_ptr(), db[1].data_ptr())
    if name == "in_bwd_r":
        _, N0, _, _, S, pad = case[:6]
        rc = lib.dfepe_est_in_bwd_r(_p(dA), C + pad, S, ncols * (C + pad), _p(dl), _p(wh), *tail, pairs, N0 if N is None else N, *outs, None)
    elif name == "in_bwd_n":
        S = case[4] if splits is None else splits
        pb = cs.flat_buf(pairs * max(case[4], 1) * 2 * C, DEV) if case[4] > 1 or splits is not None else None
        rc = lib.dfepe_est_in_bwd_n(_p(dA[0]) if dA is not None else None, _p(dl), _p(wh), *tail, pairs, case[1], *outs, S,
                                    cs.inside(pb).data_ptr() if (pb is not None and with_part) else None, None)
    else:
        rc = lib.dfepe_est_in_bwd(_p(dA[0]) if dA is not None else None, _p(dl), _p(wh), *tail, ncols, *outs, None)
    torch.cuda.synchronize()
    return rc, (up, ap, rstd, gamma, beta), (dY, dg, db, pb)


@pytest.mark.parametrize("case", cs.INBWD_R + cs.INBWD_N + cs.INBWD_100, ids=cs.case_id)
def test_adjoint(dfepe, case):
    rc, ins, bufs = _backward(dfepe, case)
    assert rc == 0
    worst = cs.check_in_bwd(case, *ins, *bufs)
    rc2, _, bufs2 = _backward(dfepe, case)
    assert rc2 == 0
    _same(bufs2, bufs)
    print("ESTNORM", case[0], "parts", {k: round(v, 3) for k, v in worst.items()})
    _report(case[0], case, worst)


def test_adjoint_refusals(dfepe):
    case = next(c for c in cs.INBWD_R if c[1] == 64)
    for N in cs.R_REFUSED:
        rc, _, bufs = _backward(dfepe, case, N=N)
        assert rc == INVALID
        _untouched(bufs)
    case = next(c for c in cs.INBWD_N if c[1] == 129)
    for splits, with_part in [(s, True) for s in cs.N_REFUSED_SPLITS] + [(3, False)]:
        rc, _, bufs = _backward(dfepe, case, splits=splits, with_part=with_part)
        assert rc == INVALID
        _untouched(bufs)


# ---- the head --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cs.HEAD_FWD, ids=cs.case_id)
def test_head_forward(dfepe, case):
    lib = dfepe._lib.lib()
    _, C, cols, with_bias = case
    a, w, bias, _ = cs.head_inputs(case)
    ap, w = _split_f16(dfepe, a), w.to(DEV)
    bias = bias.to(DEV) if with_bias else None

    def call():
        logits = cs.flat_buf(cols, DEV)
        assert lib.dfepe_est_head_fwd(ap.data_ptr(), cols * C, C, cols, w.data_ptr(), _p(bias), cs.inside(logits).data_ptr(), None) == 0
        torch.cuda.synchronize()
        return logits

    logits = call()
    worst = cs.check_head_fwd(case, ap, w, bias, logits)
    _same([call()], [logits])
    _report("head_fwd", case, worst)


@pytest.mark.parametrize("case", cs.HEAD_DW, ids=cs.case_id)
def test_head_weight_gradient_partials(dfepe, case):
    lib = dfepe._lib.lib()
    _, C, cols, blocks, want_bias = case
    a, _, _, dl = cs.head_inputs(case)
    ap, dl = _split(dfepe, a), dl.to(DEV)

    def call():
        part, bias = cs.row_buf(blocks, C, DEV), cs.flat_buf(blocks, DEV)
        assert lib.dfepe_est_head_dw(ap.data_ptr(), cols * C, C, cols, blocks, dl.data_ptr(), part[1].data_ptr(),
                                     cs.inside(bias).data_ptr() if want_bias else None, None) == 0
        torch.cuda.synchronize()
        return part, bias

    part, bias = call()
    worst = cs.check_head_dw(case, ap, dl, part, bias)
    _same(call(), (part, bias))
    _report("head_dw", case, worst)


# ---- the reductions --------------------------------------------------------------------------------------------------------------
def _colsum(dfepe, launch, srcs):
    n = len(launch)
    dsts = [cs.flat_buf(c, DEV) for _, c in launch]
    rc = dfepe._lib.lib().dfepe_est_colsum(n, (ctypes.c_void_p * n)(*[(s.data_ptr() if s.numel() else None) for s in srcs]),
                                           (ctypes.c_int * n)(*[r for r, _ in launch]), (ctypes.c_int * n)(*[c for _, c in launch]),
                                           (ctypes.c_void_p * n)(*[cs.inside(d).data_ptr() for d in dsts]), None)
    torch.cuda.synchronize()
    return rc, dsts


@pytest.mark.parametrize("launch", cs.COLSUM, ids=lambda l: f"{len(l)}seg")
def test_column_sums(dfepe, launch):
    srcs = [s.to(DEV).contiguous() for s in cs.colsum_inputs(launch)]
    rc, dsts = _colsum(dfepe, launch, srcs)
    assert rc == 0
    worst = cs.check_colsum(launch, srcs, dsts)
    rc2, dsts2 = _colsum(dfepe, launch, srcs)
    assert rc2 == 0
    _same(dsts2, dsts)
    _report("colsum", f"{len(launch)}seg", worst)


def test_column_sums_beyond_the_segment_limit(dfepe):
    launch = cs.COLSUM[-1] + [(33, 64)]
    assert len(launch) == cs.SEG_MAX + 1
    rc, dsts = _colsum(dfepe, launch, [s.to(DEV).contiguous() for s in cs.colsum_inputs(launch)])
    assert rc == INVALID
    _untouched(dsts)


def _zero_args(dfepe, case, **kw):
    """Device arguments of one layer of dfepe_est_dgamma_zero[_multi] and what check_dgamma_zero needs of them."""
    up, a, x, W, rstd, gamma = cs.zero_inputs(case, **kw)
    ap_out, ap_in = _split(dfepe, a), _split(dfepe, x)
    W, rstd, gamma = W.to(DEV).contiguous(), rstd.to(DEV), gamma.to(DEV)
    if up[0] == "next":
        up = ("next", _split(dfepe, up[1]), up[2].to(DEV).contiguous())
    else:
        up = (up[0],) + tuple(t.to(DEV).contiguous() for t in up[1:])
    return up, ap_out, ap_in, W, rstd, gamma


@pytest.mark.parametrize("case", cs.DGAMMA_ZERO, ids=cs.case_id)
def test_dgamma_of_dead_channels(dfepe, case):
    lib = dfepe._lib.lib()
    _, N, pairs, form = case
    C, Ci, ldw, Cn = cs.ZERO_C, cs.ZERO_CI, cs.ZERO_LDW, cs.ZERO_CN
    up, ap_out, ap_in, W, rstd, gamma = _zero_args(dfepe, case)
    ncols = pairs * N
    dA, dl, wh, dYn, Wn = (_p(up[1]) if form == "dA" else None, _p(up[1]) if form == "head" else None, _p(up[2]) if form == "head" else None,
                           _p(up[1]) if form == "next" else None, _p(up[2]) if form == "next" else None)

    def call(n=N):
        dg = cs.row_buf(pairs, C, DEV)
        rc = lib.dfepe_est_dgamma_zero(dA, dl, wh, ap_out.data_ptr(), ncols * C, ap_in.data_ptr(), ncols * 32, W.data_ptr(), ldw, Ci, rstd.data_ptr(),
                                       gamma.data_ptr(), SLOPE, C, n, pairs, dg[1].data_ptr(), dYn, ncols * Cn, Wn, C, Cn if form == "next" else 0, None)
        torch.cuda.synchronize()
        return rc, dg

    rc, dg = call()
    assert rc == 0
    worst = cs.check_dgamma_zero(case, up, ap_out, ap_in, W, rstd, gamma, dg)
    _same([call()[1]], [dg])
    rc, untouched = call(cs.FIX_MAX_N + 1)
    assert rc == INVALID
    _untouched([untouched])
    _report("dgamma_zero", case, worst)


def test_dgamma_of_dead_channels_two_layers_in_one_launch(dfepe):
    """dfepe_est_dgamma_zero_multi: two layers of different C (and forms) in one launch; ld = Ci / C there."""
    lib = dfepe._lib.lib()
    N, pairs = 100, 3
    ncols = pairs * N
    layers = [(("dgamma_zero", N, pairs, "next"), dict(C=32, Ci=20, ldw=20, Cn=64)), (("dgamma_zero", N, pairs, "head"), dict(C=64, Ci=32, ldw=32, salt=1))]
    args = [_zero_args(dfepe, case, **kw) for case, kw in layers]
    n = len(layers)
    ptrs = lambda vs: (ctypes.c_void_p * n)(*vs)
    sizes = lambda vs: (ctypes.c_size_t * n)(*vs)
    ints = lambda vs: (ctypes.c_int * n)(*vs)
    Cs, Cis = [kw["C"] for _, kw in layers], [kw["Ci"] for _, kw in layers]

    def call():
        dgs = [cs.row_buf(pairs, C, DEV) for C in Cs]
        rc = lib.dfepe_est_dgamma_zero_multi(
            n, ptrs([None, None]), ptrs([None, _p(args[1][0][1])]), ptrs([None, _p(args[1][0][2])]), ptrs([_p(a[1]) for a in args]), sizes([ncols * C for C in Cs]),
            ptrs([_p(a[2]) for a in args]), sizes([ncols * 32] * n), ptrs([_p(a[3]) for a in args]), ints(Cis), ptrs([_p(a[4]) for a in args]),
            ptrs([_p(a[5]) for a in args]), ints(Cs), ptrs([d[1].data_ptr() for d in dgs]), ptrs([_p(args[0][0][1]), None]), sizes([ncols * 64, 0]),
            ptrs([_p(args[0][0][2]), None]), ints([64, 0]), SLOPE, N, pairs, None)
        assert rc == 0
        torch.cuda.synchronize()
        return dgs

    dgs = call()
    worst = max(cs.check_dgamma_zero(case, a[0], a[1], a[2], a[3], a[4], a[5], dg, Ci=kw["Ci"]) for (case, kw), a, dg in zip(layers, args, dgs))
    _same(call(), dgs)
    _report("dgamma_zero_multi", "two-layers", worst)
