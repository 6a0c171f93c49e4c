"""fp64 restatement of the estimator's GEMM kernels (csrc/est_gemm.hip: est_gemm_nt_kernel with its three epilogues, est_gemm_tn_body)
that tests/est_gemm_cases.py holds them to, element by element.  torch float64, no GPU needed (it runs wherever its arguments live).

It works from the PLANES' values -- read back after the device split, or built on the host (host_planes_*) -- in the K-blocked
layout of est_common.h's kb_index, [planes][C/32][rows][32]: what an operand lost when it was split is not the kernels' error and is
not in the reference; what remains is fp32 accumulation and the epilogues' fp32 arithmetic.

Bounds (u = 2^-24; first order, SLACK = 1 + 2^-10 on every final bound for the second-order terms; each bound is on
|an fp32 evaluation - the exact value of the same expression of the planes|)
------------------------------------------------------------------------------------------------------------------------------
product   The kernel multiplies exactly the terms A_i B_j^T with i + j <= order (16-bit x 16-bit products are exact in fp32) and
          accumulates the n = terms * K products in fp32, in an order that is the matrix core's business: n u sum|a||b| for any
          order, DOUBLED because the matrix core's internal rounding is not specified:  n 2^-23 sum_terms |A_i| |B_j|^T.
          A split-K slice is the same over its own K steps.  The scaled fp16 path divides value and bound by the power-of-two scale
          (exact).
EPI_IN    est_gemm_nt_kernel, EPI_IN epilogue, per (pair, channel) over the pair's 100 columns, y = the product, dy its bound:
            mean      99 additions, the rounded 1 / 100, one product:           dmu   = mean(dy) + 101 u mean|y|
            d = y - mu                                                          dd    = dy + dmu + u |d|
            q = sum d^2 (100 fused multiply-adds, one row sum)                  dq    = sum 2 |d| dd + 101 u q
            var = q * (1 / 100) [scaled back by an exact power of two]          dvar  = dq / 100 + 2 u var
            v = var + eps                                                       dv    = dvar + u v
            rstd = 1 / sqrt(v) (a root and a quotient, correctly rounded)       drstd = rstd (dv / (2 v) + 2 u)
            k = rstd * (gamma * unscale) (the inner product is exact)           dk    = |gamma| drstd + u |k|
            z = fma(d, k, beta)                                                 dz    = |k| dd + |d| dk + u |z|
            a = z > 0 ? z : z * slope                                           da    = dz, or slope dz + u |a|
          and the output planes: two fp16 planes keep max(2^-22 |a|, 2^-25) (the low plane of a small a is subnormal: half its
          spacing 2^-24), two bf16 planes 2^-16 |a|.
          undecided: |z| <= dz (TOL dz for a slope above one) -- the two LeakyReLU branches differ by less than that there; such an
          element is still compared, with the bound widened by |z|.
EPI_INBWD est_gemm_nt_kernel, EPI_INBWD epilogue.  dA = the product (bound ddA); a = the fp32 sum of the two stored bf16 planes (exact: both sides
          read the same bits, so the branch is decided except at a == 0, where the bound is widened by |dA| |1 - slope|).
            z = a, or a * fl(1 / slope)                                         dzz   = 0, or 2 u |z|
            e = dz = dA, or dA * slope                                          de    = ddA, or slope ddA + u |e|
            s1 = sum e (d beta)                                                 ds1   = sum de + 100 u sum|e|
            S = sum fma(e, z)                                                   dS    = sum (de |z| + |e| dzz) + 101 u sum|e z|
            Sx = S - beta * s1                                                  dSx   = dS + |beta| ds1 + u |beta s1| + u |Sx|
            d gamma = Sx * fl(1 / gamma), 0 where |gamma| <= 1e-30             ddg   = dSx / |gamma| + 2 u |d gamma|
            k = rstd * gamma; m1 = s1 / 100; g = d gamma / 100 / gamma          dk = u |k|; dm1 = ds1 / 100 + 2 u |m1|; dg = ddg / (100 |gamma|) + 3 u |g|
            c1 = -k g; w = g beta - m1; c0 = k w                                each product and sum one u on top of its operands' bounds
            dY = fma(k, e, fma(c1, z, c0))                                      |k| de + |e| dk + dc1 |z| + |c1| dzz + dc0 + u |c1 z + c0| + u |dY|
          and 2^-16 |dY| for the two bf16 output planes.  The VALUE is not that chain but rstd gamma (dz - mean dz - x^ mean(dz x^)),
          x^ = (z - beta) / gamma.
tn        est_gemm_tn_body's three terms hi.hi, hi.lo, lo.hi over a slice's columns: 3 * columns * 2^-23 sum|dY||X|; a slice
          without columns is exactly zero.

TOL = 2, with the meaning of tests/detector_eval_ref.py: two correct evaluations differ by at most twice the first-order bound.
Every comparison is |got - value| <= TOL * bound, element by element (compare()); no global norm anywhere.
"""
import torch

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10
TOL = 2.0
KPTS = 100       # est_common.h: kPts
GAMMA_MIN = 1e-30  # the `ig` of the EPI_INBWD epilogue and of est_norm.hip's adjoints: below it they take x^ = 0


def unblock(P):
    """K-blocked planes [planes, rows, C] (each plane stored [C/32][rows][32]) -> float64 [planes, rows, C]."""
    n, rows, C = P.shape
    return P.double().reshape(n, C // 32, rows, 32).permute(0, 2, 1, 3).reshape(n, rows, C)


def block(x):
    """[planes, rows, C] -> the K-blocked storage of the same shape (the inverse of unblock, any dtype)."""
    n, rows, C = x.shape
    return x.reshape(n, rows, C // 32, 32).permute(0, 2, 1, 3).reshape(n, rows, C).contiguous()


def host_planes_bf16(x, n_planes):
    """What dfepe_est_split leaves: round-to-nearest bf16 planes, each the remainder of the ones before it (exact in fp32)."""
    r, out = x.float().clone(), []
    for _ in range(n_planes):
        p = r.bfloat16()
        out.append(p)
        r = r - p.float()
    return block(torch.stack(out))


def weight_scale(absmax):
    """The power of two that brings max |W| into [8, 16) (est_common.h: wscale, exponent clamped like there)."""
    eb = int(torch.tensor(float(absmax), dtype=torch.float32).view(torch.int32).item() >> 23) & 255
    return 2.0 ** (130 - min(max(eb, 100), 150))


def host_planes_f16(x, scale=1.0):
    """What dfepe_est_split_f16 leaves: two fp16 planes of x * scale."""
    r = x.float() * scale
    h = r.half()
    return block(torch.stack([h, (r - h.float()).half()]))


def product(Ap, Bp, order, scale=1.0, ksteps=None):
    """(value, bound) [ncols, M] float64 of out[col][m] = sum_{i + j <= order} A_i[m] . B_j[col] over the K steps `ksteps`
    (begin, end; None: all) of the planes Ap [NPA, M, K], Bp [NPB, ncols, K]."""
    A, B = unblock(Ap), unblock(Bp)
    if ksteps is not None:
        A, B = A[..., 32 * ksteps[0]:32 * ksteps[1]], B[..., 32 * ksteps[0]:32 * ksteps[1]]
    value = torch.zeros(B.shape[1], A.shape[1], dtype=torch.float64, device=A.device)
    mag, terms = torch.zeros_like(value), 0
    for i in range(A.shape[0]):
        for j in range(B.shape[0]):
            if i + j <= order:
                value += B[j] @ A[i].t()
                mag += B[j].abs() @ A[i].abs().t()
                terms += 1
    n = terms * A.shape[2]
    return value / scale, SLACK * n * 2.0 ** -23 * mag / scale


def split_ksteps(K, S):
    """The K steps of each of S slices, as est_gemm_nt_kernel divides them (its ks_begin and nk)."""
    nk = K // 32
    return [((nk * z) // S, (nk * (z + 1)) // S) for z in range(S)]


def layer_forward(Wp, Xp, scale, gamma, beta, eps, slope):
    """EPI_IN on the planes Wp [2, M, K] (split scaled by `scale`), Xp [2, pairs * 100, K].  Returns a dict of float64 tensors:
    a, bound_f16, bound_bf16 [ncols, M] (the activation and its bounds as two fp16 / two bf16 planes), rstd, rstd_bound [pairs, M],
    undecided [ncols, M] bool."""
    y, dy = product(Wp, Xp, 1, scale)
    ncols, M = y.shape
    pairs = ncols // KPTS
    g, b = gamma.double().view(1, 1, M), beta.double().view(1, 1, M)
    Y, DY = y.view(pairs, KPTS, M), dy.view(pairs, KPTS, M)
    mu = Y.mean(1, keepdim=True)
    dmu = DY.mean(1, keepdim=True) + 101 * U * Y.abs().mean(1, keepdim=True)
    d = Y - mu
    dd = DY + dmu + U * d.abs()
    q = (d * d).sum(1, keepdim=True)
    dq = (2 * d.abs() * dd).sum(1, keepdim=True) + 101 * U * q
    var = q / KPTS
    dvar = dq / KPTS + 2 * U * var
    v = var + eps
    dv = dvar + U * v
    rstd = v ** -0.5
    drstd = rstd * (dv / (2 * v) + 2 * U)
    k = rstd * g
    dk = g.abs() * drstd + U * k.abs()
    z = d * k + b
    dz = k.abs() * dd + d.abs() * dk + U * z.abs()
    pos = z > 0
    a = torch.where(pos, z, z * slope)
    da = torch.where(pos, dz, slope * dz + U * a.abs())
    und = z.abs() <= (dz if slope <= 1.0 else TOL * dz)
    da = torch.where(und, max(1.0, slope) * dz + U * a.abs() + z.abs(), da)
    a, da, und = a.reshape(ncols, M), da.reshape(ncols, M), und.reshape(ncols, M)
    return {"a": a, "bound_f16": SLACK * (da + torch.clamp(2.0 ** -22 * a.abs(), min=2.0 ** -25)),
            "bound_bf16": SLACK * (da + 2.0 ** -16 * a.abs()), "rstd": rstd.reshape(pairs, M),
            "rstd_bound": SLACK * drstd.reshape(pairs, M), "undecided": und}


def stored_activation(ap):
    """a as the adjoint kernels read it: the fp32 sum of the two leading bf16 planes (`unpack` in the EPI_INBWD epilogue), float64 [ncols, M]."""
    n, rows, C = ap.shape
    f = ap[0].float() + ap[1].float()
    return unblock(f.view(1, rows, C))[0]


def adjoint(dA, ddA, a, rstd, gamma, beta, slope):
    """The InstanceNorm + LeakyReLU adjoint of EPI_INBWD / est_in_bwd_kernel on an upstream gradient dA [ncols, M] known to ddA and
    the layer's output a [ncols, M] (float64: stored_activation() of its planes).
    Returns a dict: dY, dY_bound [ncols, M], dgamma, dgamma_bound, dbeta, dbeta_bound [pairs, M], undecided [ncols, M]."""
    ncols, M = dA.shape
    pairs = ncols // KPTS
    g, b = gamma.double().view(1, 1, M), beta.double().view(1, 1, M)
    pos = a > 0
    z = torch.where(pos, a, a / slope)
    dzz = torch.where(pos, torch.zeros_like(z), 2 * U * z.abs())
    e = torch.where(pos, dA, dA * slope)
    de = torch.where(pos, ddA, slope * ddA + U * e.abs())
    und = a.abs() < 2.0 ** -120
    de = torch.where(und, de + dA.abs() * abs(1.0 - slope), de)
    Z, DZZ, E, DE = (t.view(pairs, KPTS, M) for t in (z, dzz, e, de))
    s1 = E.sum(1, keepdim=True)
    ds1 = DE.sum(1, keepdim=True) + 100 * U * E.abs().sum(1, keepdim=True)
    S = (E * Z).sum(1, keepdim=True)
    dS = (DE * Z.abs() + E.abs() * DZZ).sum(1, keepdim=True) + 101 * U * (E * Z).abs().sum(1, keepdim=True)
    live = g.abs() > GAMMA_MIN
    ig = torch.where(live, 1.0 / torch.where(live, g, torch.ones_like(g)), torch.zeros_like(g))
    Sx = S - b * s1
    dSx = dS + b.abs() * ds1 + U * (b * s1).abs() + U * Sx.abs()
    dgam = Sx * ig
    ddgam = dSx * ig.abs() + 2 * U * dgam.abs()
    R = rstd.double().view(pairs, 1, M)
    k = R * g
    dk = U * k.abs()
    m1 = s1 / KPTS
    dm1 = ds1 / KPTS + 2 * U * m1.abs()
    gg = dgam / KPTS * ig
    dgg = ddgam / KPTS * ig.abs() + 3 * U * gg.abs()
    c1 = -k * gg
    dc1 = k.abs() * dgg + gg.abs() * dk + U * c1.abs()
    w = gg * b - m1
    dw = dgg * b.abs() + U * (gg * b).abs() + dm1 + U * w.abs()
    c0 = k * w
    dc0 = k.abs() * dw + w.abs() * dk + U * c0.abs()
    xh = (Z - b) * ig
    dY = k * (E - m1 - xh * (dgam / KPTS))
    dYb = (k.abs() * DE + E.abs() * dk + dc1 * Z.abs() + c1.abs() * DZZ + dc0 + U * (c1 * Z + c0).abs() + U * dY.abs()
           + 2.0 ** -16 * dY.abs())
    return {"dY": dY.reshape(ncols, M), "dY_bound": SLACK * dYb.reshape(ncols, M), "dgamma": dgam.reshape(pairs, M),
            "dgamma_bound": SLACK * ddgam.reshape(pairs, M), "dbeta": s1.reshape(pairs, M), "dbeta_bound": SLACK * ds1.reshape(pairs, M),
            "undecided": und}


def fused_adjoint(WTp, dYnp, ap, rstd, gamma, beta, slope):
    """EPI_INBWD: dA = the two-plane product of WTp [2, M, K] and dYnp [2, ncols, K], straight through adjoint()."""
    dA, ddA = product(WTp, dYnp, 1)
    out = adjoint(dA, ddA, stored_activation(ap), rstd, gamma, beta, slope)
    out["dA"], out["dA_bound"] = dA, ddA
    return out


def tn_slices(ncols, slices):
    """(begin, end) columns of each slice of dfepe_est_gemm_tn (its cps; kbeg, kend of est_gemm_tn_body); end <= begin: empty."""
    cps = ((ncols + slices - 1) // slices + 31) // 32 * 32
    return [(s * cps, min(s * cps + cps, ncols)) for s in range(slices)]


def tn_product(dYp, Xp, slices):
    """(value, bound) [slices, Cout, Cin] of part[s][co][ci] = sum over the slice's columns of dY[col][co] X[col][ci] in the three
    terms hi.hi, hi.lo, lo.hi of dYp [2, ncols, Cout], Xp [>= 2, ncols, Cin]."""
    A, B = unblock(dYp), unblock(Xp)
    vals, bnds = [], []
    for k0, k1 in tn_slices(A.shape[1], slices):
        v = torch.zeros(A.shape[2], B.shape[2], dtype=torch.float64, device=A.device)
        m = torch.zeros_like(v)
        if k1 > k0:
            for i, j in ((0, 0), (0, 1), (1, 0)):
                v += A[i, k0:k1].t() @ B[j, k0:k1]
                m += A[i, k0:k1].abs().t() @ B[j, k0:k1].abs()
        vals.append(v)
        bnds.append(SLACK * 3 * max(k1 - k0, 0) * 2.0 ** -23 * m)
    return torch.stack(vals), torch.stack(bnds)


def compare(got, value, bound, what):
    """Assert |got - value| <= TOL * bound for every element (a bound of 0: equality) and that got is finite; returns the worst
    |got - value| / bound (0 / 0 = 0)."""
    got, value, bound = got.double(), value.double().to(got.device), bound.double().to(got.device)
    assert got.shape == value.shape == bound.shape, (what, got.shape, value.shape, bound.shape)
    finite = torch.isfinite(got)
    assert bool(finite.all()), f"{what}: {int((~finite).sum())} of {got.numel()} elements are not finite, first at {_first(~finite)}"
    err = (got - value).abs()
    bad = err > TOL * bound
    if bool(bad.any()):
        at = _first(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements beyond TOL * bound, first at {at}: got {got[at].item()!r}, "
                             f"value {value[at].item()!r}, bound {bound[at].item():.3e}")
    ratio = torch.where(err > 0, err / torch.clamp(bound, min=1e-300), torch.zeros_like(err))
    return float(ratio.max()) if ratio.numel() else 0.0


def _first(mask):
    return tuple(int(i) for i in mask.nonzero()[0])
