"""The case matrix of the estimator's any-N normalisation, adjoint, head and reduction kernels (csrc/est_norm.hip, est_colsum in csrc/est_planes.hip) and one check_*() per
entry point, shared by the host test (tests/test_est_norm_ref_cpu.py: an fp32 evaluation in torch and mutations of it) and the device
test (tests/test_est_norm_edges_gpu.py).  The reference and every bound are tests/est_norm_ref.py's; the buffers (PlaneBuf, row_buf,
MARGIN), the undecided cap and affine() are tests/est_gemm_cases.py's.

Launch geometry, restated once from est_norm.hip:
  register-resident pair (the N ladders of dfepe_est_norm_fwd_r / dfepe_est_in_bwd_r): template (RPT, CP) = (2, 16) N <= 128, (8, 16)
      N <= 512, (16, 16) N <= 1024, (16, 8) N <= 2048; 1024 / CP row groups, thread (cp, rg) owns rows rg, rg + RG, ...; a row sum is
      RPT additions in the thread, log2(64 / CP) cross-lane, 15 through LDS (rg_all_sum)
  strided pair (dfepe_est_norm_fwd / _in_bwd_n): 32 row groups x 4 rows in flight, splits = 1..64 workgroups per pair, split t owns rows
      [t R, min((t + 1) R, N)), R = ceil(N / splits); a split's sum is ceil(R / 32) additions in the thread and 32 through LDS
      (pair_reduce2); the adjoint adds the `splits` partial sums in order
  dfepe_est_in_bwd (N = 100): 8 row groups of 13 rows, 8 partials through LDS
Every output and the `part` workspace carry margins and are NaN throughout before the call: check_*() asserts that the margins are
still NaN and that everything inside is finite and within TOL * bound of the restatement.  Per-pair d gamma / d beta rows and per-block
head partials are compared row by row, never after a sum."""
import torch

import est_norm_ref as ref
from est_gemm_cases import MARGIN, UNDECIDED_CAP, PlaneBuf, affine, assert_undecided_cap, case_id, hash_of, row_buf  # noqa: F401

KPTS = 100
EPS = 1e-5
SEG_MAX = 40    # include/dfepe.h: dfepe_est_colsum takes n_seg <= 40 segments per launch
PLANTED_ZEROS = 5  # stored activations of exactly 0 per adjoint case
FIX_MAX_N = 4096  # dfepe_est_dgamma_zero: the LDS array of one pair's points


def template_r(N):
    """(RPT, CP) of est_norm_fwd_r_kernel / est_in_bwd_r_kernel at N."""
    return (2, 16) if N <= 128 else (8, 16) if N <= 512 else (16, 16) if N <= 1024 else (16, 8)


def chain_r(N):
    rpt, cp = template_r(N)
    return rpt + (2 if cp == 16 else 3) + 15


def chain_n(N, splits):
    return -(-(-(-N // splits)) // 32) + 32


def chain_of(case):
    name = case[0]
    if name in ("norm_fwd_r", "in_bwd_r"):
        return chain_r(case[1])
    if name == "norm_fwd":
        return chain_n(case[1], case[4])
    if name == "in_bwd_n":
        return chain_n(case[1], case[4]) + (case[4] if case[4] > 1 else 0)
    return 13 + 8  # in_bwd


# ---- the matrix ---------------------------------------------------------------------------------------------------------------
R_NS = [1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 2047, 2048]
_by_template = {}
for _N in R_NS:
    _by_template.setdefault(template_r(_N), []).append(_N)
NORM_R, INBWD_R = [], []   # (name, N, C, pairs, S, ld - C, planes_bwd) / (name, N, C, pairs, S, ld - C, head, slope)
for _Ns in _by_template.values():
    for _i, _N in enumerate(_Ns):
        _C, _pairs, _S, _pad = (32, 96)[_i % 2], (1, 3)[(_i + _i // 2) % 2], (1, 2, 5)[_i % 3], (0, 8)[(_i // 2) % 2]
        NORM_R.append(("norm_fwd_r", _N, _C, _pairs, _S, _pad, _i % 2 == 0))
        # the head form is given the case's S and ld all the same: a null dA has to make the kernel ignore both
        INBWD_R.append(("in_bwd_r", _N, _C, _pairs, _S, _pad, _i % 3 == 1, 2.0 if _i % 4 == 3 else 0.01))
INBWD_R += [("in_bwd_r", 2048, 32, 1, 1, 0, False, 2.0), ("in_bwd_r", 1024, 96, 3, 2, 8, True, 2.0)]  # slope 2 where x^ is re-read / kept at RPT 16
R_REFUSED = [0, 2049]
# strided pair: (N, C, pairs, splits); splits > N, splits not dividing N (empty splits), 64 of them
_N_CASES = [(1, 32, 1, 1), (1, 64, 3, 2), (5, 96, 3, 7), (31, 32, 1, 3), (32, 64, 3, 1), (33, 96, 1, 2), (33, 32, 3, 64), (127, 64, 3, 64),
            (128, 32, 1, 7), (129, 96, 3, 3), (257, 64, 1, 64), (257, 32, 3, 1), (2500, 96, 3, 1), (2500, 32, 1, 7), (2500, 64, 3, 64)]
NORM_N = [("norm_fwd",) + c + (i % 2 == 0,) for i, c in enumerate(_N_CASES)]                                  # (..., planes_bwd)
INBWD_N = [("in_bwd_n",) + c + (i % 3 == 1, 2.0 if i % 4 == 3 else 0.01) for i, c in enumerate(_N_CASES)]     # (..., head, slope)
N_REFUSED_SPLITS = [0, 65]
INBWD_100 = [("in_bwd", 32, 1, False, 0.01), ("in_bwd", 96, 3, True, 0.01), ("in_bwd", 64, 2, True, 2.0), ("in_bwd", 96, 2, False, 2.0)]
# head: (C, columns, bias) / (C, columns, blocks, bias_part); 700 columns in 1 block, 15 in 8 (2), 17 in 8 (3): columns per block off 8
HEAD_FWD = [("head_fwd", C, cols, (i + j) % 2 == 0) for i, C in enumerate((32, 96, 256)) for j, cols in enumerate((1, 15, 16, 17, 700))]
HEAD_DW = [("head_dw", (32, 96, 256)[(i + j) % 3], cols, blocks(cols), (i + j) % 2 == 0)
           for i, cols in enumerate((1, 15, 16, 17, 700)) for j, blocks in enumerate((lambda c: 1, lambda c: 8, lambda c: c + 3))]
HEAD_DW += [("head_dw", 256, 700, 8, True), ("head_dw", 32, 700, 703, False)]
# colsum: launches of (rows, columns) segments; rows <= 32: wide, rows > 32: tall with four loads in flight from 49 rows on
COLSUM = [[(1, 1), (32, 63), (33, 64), (48, 65)], [(49, 1023), (64, 1024), (65, 1025), (200, 1)],
          [(1, 1025), (200, 63), (32, 1024), (33, 1023), (0, 5), (64, 65), (49, 1), (48, 1024)],
          [((1, 32, 33, 48, 49, 64, 65, 200)[i % 8], (1, 63, 64, 65, 1023, 1024, 1025)[i % 7]) for i in range(SEG_MAX)]]
# dgamma_zero: (N, pairs, upstream form)
DGAMMA_ZERO = [("dgamma_zero", 1, 1, "dA"), ("dgamma_zero", 100, 3, "head"), ("dgamma_zero", 255, 1, "next"), ("dgamma_zero", 256, 3, "dA"),
               ("dgamma_zero", 257, 1, "head"), ("dgamma_zero", 4096, 3, "next"), ("dgamma_zero", 100, 1, "next"), ("dgamma_zero", 4096, 1, "dA"),
               ("dgamma_zero", 1, 3, "head")]
ZERO_C, ZERO_CI, ZERO_LDW, ZERO_CN = 32, 20, 24, 64
ZERO_GAMMA = {3: 0.0, 4: 1e-31, 5: -1e-31, 6: 1e-29, 7: -1e-29}   # overwritten: 3, 4, 5; kept: 6, 7 and every O(1) channel

# every template on each side of its boundary, both kernels
for _cases in (NORM_R, INBWD_R):
    assert {c[1] for c in _cases} >= set(R_NS)
    for _t in ((2, 16), (8, 16), (16, 16), (16, 8)):
        _sub = [c for c in _cases if template_r(c[1]) == _t]
        assert {c[2] for c in _sub} == {32, 96} and {c[3] for c in _sub} == {1, 3} and {c[4] for c in _sub} == {1, 2, 5} and {c[5] for c in _sub} == {0, 8}, _t
        assert {c[6] for c in _sub} == {False, True}, _t
assert any(c[6] and c[4] > 1 for c in INBWD_R) and any(c[6] and c[5] > 0 for c in INBWD_R)
for _cases in (NORM_N, INBWD_N):
    assert {c[1] for c in _cases} == {1, 5, 31, 32, 33, 127, 128, 129, 257, 2500} and {c[2] for c in _cases} == {32, 64, 96}
    assert {c[4] for c in _cases} == {1, 2, 3, 7, 64} and any(c[4] > c[1] for c in _cases)
    assert any(b <= a for c in _cases for a, b in ref.split_rows(c[1], c[4]))  # an empty split
assert any(-(-c[2] // c[3]) % 8 for c in HEAD_DW if c[3] == 8)


def _gen(case, salt=0):
    return torch.Generator().manual_seed(hash_of(tuple(case)) + salt)


def _sign(shape, g):
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()


def _weights(S, g):
    w = torch.rand(S, generator=g) + 0.5
    return w / w.sum()


# ---- inputs (host, fp32, deterministic) ------------------------------------------------------------------------------------------
def fwd_inputs(case):
    """(parts [S, pairs * N, ld], gamma, beta): the product 40 +- 3 as S partials; the last pair (half the channels of the only one) is
    40 + 3.16e-3 t[n] s[c] with |t| in [0.9, 1.1] -- its variance is within a factor of four of eps, and its normalised values stay near
    +-0.7, away from the kink --; channel 7 of pair 0 is the same in every row (variance 0); gamma[5] = 0; beta = +-(2..3) |gamma|."""
    name, N, C, pairs = case[:4]
    S, pad = (case[4], case[5]) if name == "norm_fwd_r" else (1, 0)
    g = _gen(case)
    ncols, ld = pairs * N, C + pad
    Y = 40.0 + 3.0 * torch.randn(ncols, ld, generator=g)
    t = (0.9 + 0.2 * torch.rand(N, generator=g)) * _sign((N,), g)
    near = 40.0 + 3.16e-3 * t[:, None] * _sign((C,), g)[None, :]
    c0 = C // 2 if pairs == 1 else 0
    Y[(pairs - 1) * N:, c0:C] = near[:, c0:]
    w = _weights(S, g)
    parts = (Y[None] * w[:, None, None]).contiguous()
    parts[:, :N, 7] = (40.0 * w)[:, None]
    gamma, beta = affine(C, g)
    return parts, gamma, beta


def bwd_inputs(case):
    """(up, a [ncols, C], rstd [pairs, C], gamma, beta); up: dA partials [S, ncols, ld] or (dlogit [ncols], w_head [C]).  a = lrelu(gamma
    x^ + beta) of a random x^, a few of them exactly 0; gamma of both signs, gamma[5] = 0, [6] = 1e-31, [7] = -1e-29, [8] = -1e-31,
    [9] = 1e-29 with beta = 0 at 6..9 (a forward-sized activation: est_gemm_cases.dgrad_inputs); rstd arbitrary positive."""
    name = case[0]
    if name == "in_bwd_r":
        _, N, C, pairs, S, pad, head, slope = case
    elif name == "in_bwd_n":
        (_, N, C, pairs, _, head, slope), S, pad = case, 1, 0
    else:
        (_, C, pairs, head, slope), N, S, pad = case, KPTS, 1, 0
    g = _gen(case)
    ncols = pairs * N
    gamma = (1 + 0.2 * torch.randn(C, generator=g)) * _sign((C,), g)
    beta = 0.3 * torch.randn(C, generator=g)
    for ch, v in ((5, 0.0), (6, 1e-31), (7, -1e-29), (8, -1e-31), (9, 1e-29)):
        gamma[ch] = v
    beta[6:10] = 0.0
    z = torch.randn(ncols, C, generator=g) * gamma[None, :] + beta[None, :]
    a = torch.where(z > 0, z, z * slope)
    a.view(-1)[::97][:PLANTED_ZEROS] = 0.0
    rstd = 0.5 + torch.rand(pairs, C, generator=g)
    if head:
        up = (torch.randn(ncols, generator=g), torch.randn(C, generator=g))
    else:
        up = (torch.randn(ncols, C + pad, generator=g)[None] * _weights(S, g)[:, None, None]).contiguous()
    return up, a, rstd, gamma.float(), beta.float()


def head_inputs(case):
    """(a [cols, C], w [C], bias [1], dlogit [cols])."""
    C, cols = case[1], case[2]
    g = _gen(case)
    return torch.randn(cols, C, generator=g), torch.randn(C, generator=g), torch.randn(1, generator=g), torch.randn(cols, generator=g)


def colsum_inputs(launch, salt=0):
    g = _gen(("colsum", len(launch), salt))
    return [torch.randn(r, c, generator=g) + 0.5 for r, c in launch]


def zero_inputs(case, C=ZERO_C, Ci=ZERO_CI, ldw=ZERO_LDW, Cn=ZERO_CN, salt=0):
    """(up, a [ncols, C], x [ncols, 32], W [C, ldw], rstd [pairs, C], gamma): up = ("dA", dA), ("head", dlogit, w_head) or ("next", dYn
    [ncols, Cn], W_next [Cn, C]); x has Ci live channels."""
    _, N, pairs, form = case
    g = _gen(case, salt)
    ncols = pairs * N
    gamma = 1 + 0.2 * torch.randn(C, generator=g)
    for ch, v in ZERO_GAMMA.items():
        gamma[ch] = v
    a = torch.randn(ncols, C, generator=g)
    a.view(-1)[::89][:3] = 0.0
    x = torch.zeros(ncols, 32)
    x[:, :Ci] = torch.randn(ncols, Ci, generator=g)
    W = torch.randn(C, ldw, generator=g)
    rstd = 0.5 + torch.rand(pairs, C, generator=g)
    if form == "dA":
        up = ("dA", torch.randn(ncols, C, generator=g))
    elif form == "head":
        up = ("head", torch.randn(ncols, generator=g), torch.randn(C, generator=g))
    else:
        up = ("next", torch.randn(ncols, Cn, generator=g), torch.randn(Cn, C, generator=g))
    return up, a, x, W, rstd, gamma.float()


# ---- buffers ---------------------------------------------------------------------------------------------------------------------
def flat_buf(count, device, dtype=torch.float32):
    """`count` elements with a margin in front and behind, NaN throughout (inside(): the elements)."""
    return PlaneBuf(1, 1, count, dtype, device)


def inside(buf):
    """The elements of a flat_buf, as a view."""
    return buf.flat[MARGIN:MARGIN + buf.count]


def _nan(t, what):
    assert bool(torch.isnan(t).all()), f"{what}: written"


def _rows(buf, what):
    _nan(buf[0], what + ": the row in front")
    _nan(buf[-1], what + ": the row behind")
    return buf[1:-1].cpu()


def _workspace(part_buf, what):
    part_buf.assert_margins(what + " part")
    w = inside(part_buf)
    assert bool(torch.isfinite(w).all()), f"{what}: {int((~torch.isfinite(w)).sum())} cells of the part workspace were not written"


def planes_value(P):
    return ref.unblock(P.cpu()).sum(0)


# ---- one check per entry point: they return the worst |got - value| / bound per output ---------------------------------------------
def check_norm_fwd(case, parts, gamma, beta, slope, out, out_bwd, rstd_buf, part_buf=None):
    """dfepe_est_norm_fwd_r / dfepe_est_norm_fwd.  out / out_bwd: PlaneBuf of two fp16 / two bf16 planes (out_bwd untouched when the case
    keeps none), rstd_buf: row_buf, part_buf: flat_buf of pairs * splits * 2 * C (strided pair with splits > 1)."""
    name, N, C, pairs = case[:4]
    keep, what = case[-1], case_id(case)
    mode = "two_pass" if name == "norm_fwd_r" or case[4] == 1 else ("chan", case[4])
    r = ref.norm_forward(parts.cpu()[:, :, :C], N, gamma.cpu(), beta.cpu(), EPS, slope, mode, chain_of(case))
    assert_undecided_cap(r["undecided"], what)  # before the output is looked at
    out.assert_margins(what + " planes")
    worst = {"a": ref.compare(planes_value(out.planes()), r["a"], r["bound_f16"], what + " planes")}
    if keep:
        out_bwd.assert_margins(what + " planes_bwd")
        worst["a_bwd"] = ref.compare(planes_value(out_bwd.planes()), r["a"], r["bound_bf16"], what + " planes_bwd")
    else:
        out_bwd.assert_untouched(what + " planes_bwd")
    worst["rstd"] = ref.compare(_rows(rstd_buf, what + " rstd"), r["rstd"], r["rstd_bound"], what + " rstd")
    if part_buf is not None:
        _workspace(part_buf, what)
    return worst


def check_in_bwd(case, up, ap, rstd, gamma, beta, dY, dg_buf, db_buf, part_buf=None):
    """dfepe_est_in_bwd_r / _in_bwd_n / _in_bwd.  ap: the layer's output planes [2, ncols, C] bf16 as the kernel was given them; dY:
    PlaneBuf of two bf16 planes; dg_buf / db_buf: row_buf, one row per PAIR, compared row by row."""
    name = case[0]
    N, C = (case[1], case[2]) if name != "in_bwd" else (KPTS, case[1])
    slope, what = case[-1], case_id(case)
    up = (up[0].cpu(), up[1].cpu()) if isinstance(up, tuple) else up.cpu()[:, :, :C]
    stored = ref.stored_activation(ap.cpu())
    r = ref.adjoint_n(up, stored, rstd.cpu(), gamma.cpu(), beta.cpu(), slope, N, chain_of(case))
    # the planes decide the branch: undecided are the planted zeros and, in a channel below the threshold, an activation below 2^-120
    odd = r["undecided"] & (stored != 0) & (gamma.cpu().double().abs() > ref.GAMMA_MIN)[None, :]
    assert int((stored == 0).sum()) <= PLANTED_ZEROS and not bool(odd.any()), what
    dY.assert_margins(what + " dY")
    worst = {"dY": ref.compare(planes_value(dY.planes()), r["dY"], r["dY_bound"], what + " dY"),
             "dgamma": ref.compare(_rows(dg_buf, what + " d gamma"), r["dgamma_part"], r["dgamma_bound"], what + " d gamma"),
             "dbeta": ref.compare(_rows(db_buf, what + " d beta"), r["dbeta_part"], r["dbeta_bound"], what + " d beta")}
    if part_buf is not None:
        _workspace(part_buf, what)
    return worst


def check_head_fwd(case, ap, w, bias, logits):
    """ap: the forward's two fp16 planes [2, cols, C]; bias: [1] or None; logits: flat_buf(cols)."""
    what = case_id(case)
    value, bound = ref.head_forward(ap.cpu(), w.cpu(), None if bias is None else bias.cpu())
    logits.assert_margins(what)
    return ref.compare(inside(logits).cpu(), value, bound, what)


def check_head_dw(case, ap, dlogit, part, bias_part):
    """ap: the backward's two bf16 planes; part: row_buf(blocks, C), one row per BLOCK; bias_part: flat_buf(blocks), untouched when the
    case asks for none.  A block without columns reads exactly 0 (its bound is 0)."""
    _, C, cols, blocks, want_bias = case
    what = case_id(case)
    v, dv, b, db = ref.head_dw(ap.cpu(), dlogit.cpu(), blocks)
    got = _rows(part, what + " part")
    worst = {"part": ref.compare(got, v, dv, what + " part")}
    if want_bias:
        bias_part.assert_margins(what + " bias_part")
        worst["bias_part"] = ref.compare(inside(bias_part).cpu(), b, db, what + " bias_part")
    else:
        bias_part.assert_untouched(what + " bias_part")
    return worst


def check_colsum(launch, srcs, dsts):
    """dsts: one flat_buf(cols) per segment."""
    worst = 0.0
    for i, ((rows, cols), src, dst) in enumerate(zip(launch, srcs, dsts)):
        what = f"colsum segment {i} ({rows} x {cols})"
        value, bound = ref.colsum(src.cpu().reshape(rows, cols))
        dst.assert_margins(what)
        worst = max(worst, ref.compare(inside(dst).cpu(), value, bound, what))
    return worst


def check_dgamma_zero(case, up, ap_out, ap_in, W, rstd, gamma, dg_buf, Ci=ZERO_CI):
    """up: as zero_inputs' with the planes of dY_next in place of its fp32 values; dg_buf: row_buf(pairs, C), NaN before the call: the
    channels with |gamma| <= 1e-30 hold the recomputed d gamma of each pair, every other one still its NaN."""
    _, N, pairs, form = case
    what = case_id(case)
    up = tuple(t.cpu() if torch.is_tensor(t) else t for t in up)
    value, bound = ref.dgamma_zero(up, ap_out.cpu(), ap_in.cpu(), W.cpu()[:, :Ci], rstd.cpu(), 0.01, N)
    got = _rows(dg_buf, what)
    dead = gamma.cpu().double().abs() <= ref.GAMMA_MIN
    assert int(dead.sum()) == 3
    _nan(got[:, ~dead], what + ": a live channel's d gamma")
    return ref.compare(got[:, dead], value[:, dead], bound[:, dead], what)


# ---- inorm_lrelu (csrc/inorm.hip): fp32 rows, no planes -------------------------------------------------------------------------------
# (N, C, R): templates NV = 2 / 4 / 8 float4 per lane at N <= 128 / 256 / 512; C R = 1, 15, 16, 17, 35 rows against the 16 rows of a workgroup
INORM = [("inorm", N) + rc for N, rcs in ((4, [(1, 1), (5, 7)]), (8, [(3, 5), (17, 1)]), (128, [(4, 4)]), (132, [(1, 1), (3, 5), (5, 7)]),
                                          (256, [(4, 4), (17, 1)]), (260, [(1, 1), (4, 4), (5, 7)]), (512, [(3, 5), (17, 1)])) for rc in rcs]
INORM_REFUSED = [516, 10]
for _lo, _hi in ((1, 128), (129, 256), (257, 512)):
    assert {c[2] * c[3] for c in INORM if _lo <= c[1] <= _hi} == {1, 15, 16, 17, 35}


def chain_inorm(N):
    """inorm.hip:41-46: a lane adds NV float4 (two levels inside each, one addition per float4), four cross-lane additions."""
    return (2 if N <= 128 else 4 if N <= 256 else 8) + 2 + 4


def inorm_inputs(case):
    """(Y [C, R, N], gamma, beta [C], G [C, R, N]); beta = +-(2..3) |gamma|, one gamma exactly 0 where there are more than three channels."""
    _, N, C, R = case
    g = _gen(case)
    Y = torch.randn(C, R, N, generator=g) * 3 + 40  # a mean far above the deviation
    gamma, beta = affine(C, g, zero=(C - 1,) if C > 3 else ())
    return Y, gamma, beta, torch.randn(C, R, N, generator=g)


def check_inorm(case, Y, gamma, beta, slope, A, stats, G, gY, ggamma, gbeta):
    """ops.inorm_lrelu's output A [C, R, N] and gradients (gY [C, R, N], ggamma, gbeta [C]: the rows' sums, added by torch) and the stats
    [C R, 2] (mean, rstd) its forward kernel left -- the backward's inputs as given."""
    _, N, C, R = case
    what = case_id(case)
    Y, A, G, gY, stats = Y.cpu(), A.cpu(), G.cpu(), gY.cpu(), stats.cpu()
    cm = lambda t: t.permute(1, 2, 0).reshape(R * N, C)  # (pair = r, point) x channel
    r = ref.norm_forward(cm(Y)[None], N, gamma.cpu(), beta.cpu(), EPS, slope, "two_pass", chain_inorm(N))
    assert_undecided_cap(r["undecided"], what)
    worst = {"a": ref.compare(cm(A), r["a"], r["bound_f32"], what + " A"),
             "mean": ref.compare(stats[:, 0].view(C, R).t(), r["mean"], r["mean_bound"], what + " mean"),
             "rstd": ref.compare(stats[:, 1].view(C, R).t(), r["rstd"], r["rstd_bound"], what + " rstd")}
    rows = C * R
    per_row = lambda t: t.cpu().double().view(C, 1).expand(C, R).reshape(rows)
    b = ref.adjoint_f32(G.reshape(rows, N), Y.reshape(rows, N), stats[:, 0], stats[:, 1], per_row(gamma), per_row(beta), slope, chain_inorm(N))
    worst["gY"] = ref.compare(gY.reshape(rows, N), b["gY"], b["gY_bound"], what + " gY")
    for name, got in (("row_ggamma", ggamma), ("row_gbeta", gbeta)):
        v, dv = b[name].view(C, R), b[name + "_bound"].view(C, R)
        worst[name] = ref.compare(got.cpu(), v.sum(1), dv.sum(1) + ref.SLACK * R * ref.U * v.abs().sum(1), what + " " + name)
    return worst
