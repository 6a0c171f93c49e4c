"""The case matrix of the estimator's GEMM kernels (csrc/est_gemm.hip, constants in csrc/est_common.h) and one check() per entry point, shared by the host test of
the restatement (tests/test_est_gemm_ref_cpu.py: an fp32 evaluation on host-built planes, and mutations of it) and the device test
(tests/test_est_gemm_edges_gpu.py).  The reference and every bound are tests/est_gemm_ref.py's.

Launch geometry, restated once from the sources (est_common.h's constants BM = 128 channels and BSTEP = 200 owned columns per
workgroup; est_gemm.hip: the grid every entry point hands to launch_nt(); small_grid(): the AHEAD = 2 build at up to 256 workgroups,
the default build above; the XCD remap at the top of est_gemm_nt_kernel: taken when gridDim.x % 8 == 0):
    workgroups(M, ncols, S) = ceil(ncols / 200) * ceil(M / 128) * S
    build    = "small" if workgroups <= 256 else "full"
    remapped = ceil(ncols / 200) % 8 == 0
At import the module asserts that DFEPE_EST_SMALL_GRID does not override that choice, that each of the four two-plane entry points
has cases in both builds, with and without the remap in each, and that the 256 / 264 boundary pair (M = 1024 at 32 and 33 column
blocks) is there.

Every output buffer carries a margin in front and behind (and between planes) and is NaN throughout before the call: check()
asserts that the margins and the ldc - M padding are still NaN and -- through compare() -- that every element inside is finite and
within TOL * bound of the restatement."""
import os

import torch

import est_gemm_ref as ref

KPTS = ref.KPTS
MARGIN = 64  # elements around and between planes
UNDECIDED_CAP = 1e-4


def workgroups(M, ncols, S=1):
    return -(-ncols // 200) * -(-M // 128) * S


def build_of(M, ncols, S=1):
    return "small" if workgroups(M, ncols, S) <= 256 else "full"


def remapped(ncols):
    return (-(-ncols // 200)) % 8 == 0


# ---- the matrix ---------------------------------------------------------------------------------------------------------------
# plain products: (M, ncols, K, S, ldc - M); S > 1 only where the entry point splits
_PLAIN = [(8, 1, 32, 1, 0), (32, 15, 64, 1, 4), (40, 16, 96, 1, 0), (128, 17, 32, 1, 4), (136, 199, 64, 2, 0), (8, 200, 96, 3, 4),
          (40, 201, 160, 3, 0), (32, 207, 32, 1, 0), (136, 208, 64, 1, 4), (128, 209, 96, 1, 0), (40, 1600, 32, 1, 4),
          (136, 1800, 64, 1, 0), (32, 209, 1024, 1, 0), (128, 201, 1024, 32, 4), (1024, 6400, 32, 1, 0), (1024, 6600, 32, 1, 4),
          (136, 3401, 256, 8, 0),
          (136, 3200, 288, 9, 4)]  # full AND remapped (16 column blocks x 2 x 9 = 288), one K step per slice
PLAIN = ([("gemm_nt_f16",) + c + (i % 2 == 0,) for i, c in enumerate(_PLAIN)]        # (..., scaled)
         + [("gemm_nt2",) + c + (False,) for c in _PLAIN]
         + [("gemm_nt3",) + c + (False,) for c in _PLAIN if c[3] == 1])
# dfepe_est_gemm_nt_gx: (C0, N, pairs, layout, K) at M = 32
GX = [(4, 37, 3, "dense", 32), (7, 37, 3, "channel", 64), (7, 100, 5, "dense", 32), (4, 100, 16, "channel", 64), (4, 1970, 2, "dense", 32),
      (7, 1970, 26, "channel", 32)]  # 26 x 1970 = 51220 columns = 257 column blocks: the default build
# fused epilogues: (M, pairs, K); M = 1024 at 64 / 66 pairs is the 256 / 264 boundary, 1056 at 57 the half-empty last block of a full
# grid (29 x 9 = 261), 1056 at 64 the remapped full grid (288), 160 at 16 the remapped small one
_FUSED = [(32, 1, 32), (96, 2, 96), (128, 3, 32), (160, 16, 96), (1056, 3, 32), (1056, 1, 96), (1024, 64, 32), (1024, 66, 32),
          (1056, 57, 32), (1056, 64, 32), (160, 80, 96)]  # 160 at 80 pairs: 40 blocks x 2 = small and remapped beyond one XCD round
LAYER_FWD = [("layer_fwd", M, p, K, i % 2 == 0, i % 3 != 2) for i, (M, p, K) in enumerate(_FUSED)]   # (..., absmax, planes_bwd)
DGRAD = [("dgrad_in_bwd", M, p, K, 0.01) for M, p, K in _FUSED] + [("dgrad_in_bwd", 96, 3, 64, 2.0)]  # slope 2: unrelu's +inf branch
# weight gradient: (Cout, Cin, ncols, slices)
TN = [(32, 32, 1, 1), (96, 160, 31, 3), (128, 96, 32, 1), (160, 32, 33, 3), (32, 128, 100, 8), (96, 96, 700, 16), (160, 160, 700, 8),
      (128, 128, 100, 16), (160, 96, 1, 3), (128, 160, 700, 1)]
TN_MULTI = [(100, [(32, 32, 3), (160, 96, 8), (96, 128, 1)]), (700, [(160, 160, 8), (32, 96, 3), (128, 32, 16), (96, 32, 1)])]


def geometry(case):
    """(build, remapped) of a case of a two-plane entry point."""
    if case[0] in ("gemm_nt_f16", "gemm_nt2"):
        _, M, ncols, K, S, pad, _ = case
        return build_of(M, ncols, S), remapped(ncols)
    _, M, pairs = case[:3]
    return build_of(M, pairs * KPTS), remapped(pairs * KPTS)


assert "DFEPE_EST_SMALL_GRID" not in os.environ, "DFEPE_EST_SMALL_GRID forces one build: the matrix would not reach the other"
for _name, _cases in (("gemm_nt_f16", PLAIN), ("gemm_nt2", PLAIN), ("layer_fwd", LAYER_FWD), ("dgrad_in_bwd", DGRAD)):
    _have = {geometry(c) for c in _cases if c[0] == _name}
    assert _have == {(b, r) for b in ("small", "full") for r in (False, True)}, (_name, _have)
    _wg = {workgroups(c[1], c[2] if _name.startswith("gemm") else c[2] * KPTS, c[4] if _name.startswith("gemm") else 1)
           for c in _cases if c[0] == _name and c[1] == 1024}
    assert {256, 264} <= _wg, (_name, _wg)


def case_id(case):
    return "-".join(str(x) for x in case)


# ---- inputs (host, fp32, deterministic) ------------------------------------------------------------------------------------------
def _gen(case, salt=0):
    return torch.Generator().manual_seed(hash_of(case) + salt)


def hash_of(case):
    h = 17
    for ch in case_id(case if isinstance(case, tuple) else tuple(case)):
        h = (h * 131 + ord(ch)) % (2 ** 31 - 1)
    return h


def f16_operand(shape, g):
    """fp32 values of magnitude [0.25, 3.75) whose two fp16 planes are BOTH normal or zero (no nonzero plane element below 2^-14:
    subnormal planes stay with the looser test of tests/test_estimator_mfma_gpu.py): a low plane that would be subnormal is moved to
    +-2^-14, less than half an ulp of its high plane, so the split returns exactly (high, low)."""
    x = (0.25 + 3.5 * torch.rand(shape, generator=g)) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)
    return f16_safe(x)


def f16_safe(x):
    h = x.half()
    lo = (x - h.float()).half()
    small = (lo != 0) & (lo.float().abs() < 2.0 ** -14)
    lo = torch.where(small, torch.copysign(torch.full_like(lo, 2.0 ** -14), lo), lo)
    return h.float() + lo.float()


def assert_planes_normal(P):
    v = P.float().abs()
    assert not bool(((v > 0) & (v < 2.0 ** -14)).any()), "an fp16 plane element is subnormal"


def plain_inputs(case):
    """(A [M, K], B [ncols, K]) fp32."""
    name, M, ncols, K, S, pad, scaled = case
    g = _gen(case)
    if name == "gemm_nt_f16":
        A = f16_operand((M, K), g)
        return (A * 2.0 ** -5 if scaled else A), f16_operand((ncols, K), g)
    return torch.randn(M, K, generator=g), torch.randn(ncols, K, generator=g)


def gx_inputs(case):
    C0, N, pairs, layout, K = case
    g = _gen(("gx",) + case)
    return torch.randn(32, K, generator=g), torch.randn(pairs * N, K, generator=g)


def affine(M, g, zero=(5,)):
    """gamma, beta with beta = +-(2 .. 3) |gamma|: the pre-activation's density at the kink is a twentieth of a centred one's (the cap
    on undecided elements), both branches are still taken within most (pair, channel)s, and the channels' signs differ."""
    gamma = (1 + 0.2 * torch.randn(M, generator=g)) * (torch.randint(0, 2, (M,), generator=g) * 2 - 1)
    beta = gamma.abs() * (2 + torch.rand(M, generator=g)) * (torch.randint(0, 2, (M,), generator=g) * 2 - 1)
    for ch in zero:
        gamma[ch] = 0.0
    return gamma.float(), beta.float()


def layer_fwd_inputs(case):
    """(W [M, K], X [ncols, K], gamma, beta).  One pair (the second, or the only one) is a constant column plus noise of 1e-3 -- its
    variance is close to eps, the cancellation est_gemm_nt_kernel's EPI_IN epilogue speaks of ("the difference first"); the noise is t[col] v[k] with |t| in [0.9, 1.1], so that the pair's normalised
    values stay near +-1 and away from the kink however wide the bound is there.  gamma[5] = 0."""
    _, M, pairs, K, absmax, keep = case
    g = _gen(case)
    W = f16_operand((M, K), g)
    if absmax:
        W = W * 2.0 ** -2
    X = f16_operand((pairs * KPTS, K), g)
    lv = min(1, pairs - 1)
    # eight channels of magnitude [0.26, 0.49), the others zero: the product's bound (n 2^-23 sum|w||x|, n = 3 K) then stays a few
    # percent of the noise's 1e-3 sqrt(8) |w|, and the variance, 8e-6 |w|^2, within a factor of four of eps = 1e-5
    c, v = torch.zeros(K), torch.zeros(K)
    c[:8] = (0.26 + 0.23 * torch.rand(8, generator=g)) * (torch.randint(0, 2, (8,), generator=g) * 2 - 1)
    v[:8] = (torch.randint(0, 2, (8,), generator=g) * 2 - 1).float()
    t = (0.9 + 0.2 * torch.rand(KPTS, generator=g)) * (torch.randint(0, 2, (KPTS,), generator=g) * 2 - 1)
    X[lv * KPTS:(lv + 1) * KPTS] = f16_safe(c[None, :] + 1e-3 * t[:, None] * v[None, :])
    gamma, beta = affine(M, g)
    return W, X, gamma, beta


def dgrad_inputs(case):
    """(WT [M, K], dYn [ncols, K], a [ncols, M], rstd [pairs, M], gamma, beta): a = lrelu(gamma x^ + beta) of a random x^, as a
    forward leaves it.  gamma[5] = 0, gamma[6] = 1e-31 (below the 1e-30 at which the kernel gives x^ up), gamma[7] = -1e-29 (above);
    beta[6] = beta[7] = 0: with a beta of O(1) an activation stored to 16 bits keeps nothing of a 1e-29 x^."""
    _, M, pairs, K, slope = case
    g = _gen(case)
    ncols = pairs * KPTS
    WT = torch.randn(M, K, generator=g) / K ** 0.5
    dYn = torch.randn(ncols, K, generator=g)
    gamma = 1 + 0.2 * torch.randn(M, generator=g)
    beta = 0.3 * torch.randn(M, generator=g)
    gamma[5], gamma[6], gamma[7] = 0.0, 1e-31, -1e-29
    beta[6] = beta[7] = 0.0
    z = torch.randn(ncols, M, generator=g) * gamma[None, :] + beta[None, :]
    a = torch.where(z > 0, z, z * slope)
    rstd = 0.5 + torch.rand(pairs, M, generator=g)
    return WT, dYn, a, rstd, gamma, beta


def tn_inputs(Cout, Cin, ncols, salt=0):
    g = _gen(("tn", Cout, Cin, ncols), salt)
    return torch.randn(ncols, Cout, generator=g), torch.randn(ncols, Cin, generator=g)


# ---- NaN pre-filled buffers with margins ------------------------------------------------------------------------------------------
class PlaneBuf:
    """n planes of `count` elements, MARGIN elements in front, between and behind; NaN throughout."""

    def __init__(self, n, rows, C, dtype, device):
        self.n, self.rows, self.C, self.count = n, rows, C, rows * C
        self.stride = self.count + MARGIN
        self.flat = torch.full((MARGIN + n * self.stride,), float("nan"), dtype=dtype, device=device)

    def first(self):
        return self.flat[MARGIN:]

    def planes(self):
        return torch.stack([self.flat[MARGIN + p * self.stride:MARGIN + p * self.stride + self.count] for p in range(self.n)]).view(self.n, self.rows, self.C)

    def assert_margins(self, what):
        m = torch.ones_like(self.flat, dtype=torch.bool)
        for p in range(self.n):
            m[MARGIN + p * self.stride:MARGIN + p * self.stride + self.count] = False
        assert bool(torch.isnan(self.flat[m]).all()), f"{what}: a margin was written"

    def assert_untouched(self, what):
        assert bool(torch.isnan(self.flat).all()), f"{what}: written"


def row_buf(rows, M, device):
    """[rows + 2, M] fp32, NaN: the first and last row are margins."""
    return torch.full((rows + 2, M), float("nan"), device=device)


def _nan(t, what):
    assert bool(torch.isnan(t).all()), f"{what}: written"


def assert_undecided_cap(und, what):
    n = int(und.sum())
    assert n <= UNDECIDED_CAP * und.numel(), f"{what}: {n} of {und.numel()} elements undecided by the restatement alone"


# ---- one check() per entry point: they return the worst |got - value| / bound ---------------------------------------------------
def check_plain(case, Ap, Bp, scale, buf):
    """buf [S, ncols + 2, ldc] (slice z of a split launch split_stride = (ncols + 2) * ldc floats behind slice z - 1), out = buf[0, 1]."""
    name, M, ncols, K, S, pad, _ = case
    order = 2 if name == "gemm_nt3" else 1
    assert buf.shape == (S, ncols + 2, M + pad)
    worst = 0.0
    for z, ks in enumerate(ref.split_ksteps(K, S)):
        value, bound = ref.product(Ap, Bp, order, scale, ks if S > 1 else None)
        _nan(buf[z, 0], f"{case_id(case)} slice {z}: the row in front")
        _nan(buf[z, -1], f"{case_id(case)} slice {z}: the row behind")
        _nan(buf[z, 1:-1, M:], f"{case_id(case)} slice {z}: the ldc padding")
        worst = max(worst, ref.compare(buf[z, 1:-1, :M], value, bound, f"{case_id(case)} slice {z}"))
    return worst


def gx_strides(case):
    C0, N, pairs, layout, K = case
    return (C0 * N, N) if layout == "dense" else (N, pairs * N)


def check_gx(case, Ap, Bp, flat):
    """flat: N margin elements, pairs * C0 * N of the destination, N margin elements."""
    C0, N, pairs, layout, K = case
    value, bound = ref.product(Ap, Bp, 1)
    pick = (lambda t: t.view(pairs, N, 32)[:, :, :C0].permute(0, 2, 1)) if layout == "dense" else (lambda t: t.view(pairs, N, 32)[:, :, :C0].permute(2, 0, 1))
    _nan(flat[:N], f"gx {case_id(case)}: the margin in front")
    _nan(flat[-N:], f"gx {case_id(case)}: the margin behind")
    inside = flat[N:-N].view((pairs, C0, N) if layout == "dense" else (C0, pairs, N))
    return ref.compare(inside, pick(value), pick(bound), f"gx {case_id(case)}")


def planes_value(P):
    return ref.unblock(P).sum(0)


def check_layer_fwd(case, Wp, Xp, scale, gamma, beta, eps, slope, out, out_bwd, rstd_buf):
    """out / out_bwd: PlaneBuf of two fp16 / two bf16 planes (out_bwd untouched when the case keeps none), rstd_buf: row_buf."""
    _, M, pairs, K, absmax, keep = case
    what = case_id(case)
    if not absmax:
        assert_planes_normal(Wp)
    assert_planes_normal(Xp)
    r = ref.layer_forward(Wp, Xp, scale, gamma, beta, eps, slope)
    assert_undecided_cap(r["undecided"], what)
    out.assert_margins(what + " planes")
    worst = {"a": ref.compare(planes_value(out.planes()), r["a"], r["bound_f16"], what + " planes")}
    if keep:
        out_bwd.assert_margins(what + " planes_bwd")
        worst["a_bwd"] = ref.compare(planes_value(out_bwd.planes()), r["a"], r["bound_bf16"], what + " planes_bwd")
    else:
        out_bwd.assert_untouched(what + " planes_bwd")
    _nan(rstd_buf[0], what + " rstd: the row in front")
    _nan(rstd_buf[-1], what + " rstd: the row behind")
    worst["rstd"] = ref.compare(rstd_buf[1:-1], r["rstd"], r["rstd_bound"], what + " rstd")
    return worst


def check_dgrad(case, WTp, dYnp, ap, rstd, gamma, beta, dY, dg_buf, db_buf):
    """dY: PlaneBuf of two bf16 planes, dg_buf / db_buf: row_buf.  Returns (worst ratios, the restatement)."""
    _, M, pairs, K, slope = case
    what = case_id(case)
    r = ref.fused_adjoint(WTp, dYnp, ap, rstd, gamma, beta, slope)
    assert_undecided_cap(r["undecided"], what)
    dY.assert_margins(what + " dY")
    for b, n in ((dg_buf, "d gamma"), (db_buf, "d beta")):
        _nan(b[0], f"{what} {n}: the row in front")
        _nan(b[-1], f"{what} {n}: the row behind")
    worst = {"dY": ref.compare(planes_value(dY.planes()), r["dY"], r["dY_bound"], what + " dY"),
             "dgamma": ref.compare(dg_buf[1:-1], r["dgamma"], r["dgamma_bound"], what + " d gamma"),
             "dbeta": ref.compare(db_buf[1:-1], r["dbeta"], r["dbeta_bound"], what + " d beta")}
    return worst, r


def check_tn(case, dYp, Xp, part):
    """part [slices + 2, Cout, Cin]: the first and last are margins; an empty slice's bound is 0, so it must read exactly 0."""
    Cout, Cin, ncols, slices = case
    what = "tn " + case_id(case)
    value, bound = ref.tn_product(dYp, Xp, slices)
    _nan(part[0], what + ": the slice in front")
    _nan(part[-1], what + ": the slice behind")
    for s, (k0, k1) in enumerate(ref.tn_slices(ncols, slices)):
        if k1 <= k0:
            assert bool((part[1 + s] == 0).all()), f"{what}: empty slice {s} is not zero"
    return ref.compare(part[1:-1], value, bound, what)
