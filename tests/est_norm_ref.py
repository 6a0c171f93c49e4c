"""fp64 restatement of the estimator's any-N normalisation, adjoint, head and reduction kernels (csrc/est_norm.hip: est_norm_fwd_r_kernel,
est_norm_fwd_n_kernel<0|1|2>, est_in_bwd_r_kernel, est_in_bwd_n_kernel<0|1|2>, est_in_bwd_kernel, est_head_fwd_kernel, est_head_dw_kernel,
est_dgamma_zero_kernel; csrc/est_planes.hip: est_colsum_kernel; csrc/inorm.hip: inorm_lrelu_*_kernel) that tests/est_norm_cases.py holds them to, element by
element.  torch float64, no GPU needed.  U, SLACK, TOL, GAMMA_MIN, the plane helpers and compare() are tests/est_gemm_ref.py's.

Like that module it works from the VALUES of what a kernel reads -- the fp32 partial products, the planes' bits, the fp32 partial
gradients, rstd as given --, so nothing an input lost before the kernel saw it is in the reference.

Bounds (u = 2^-24; first order, x SLACK; each on |an fp32 evaluation - the exact value of the same expression of the inputs|).  A sum
of terms t_i whose longest chain of dependent additions is n is known to  n u sum|t_i|  in ANY order of that depth; every function
takes `chain`, the n of the kernel that is being held (tests/est_norm_cases.py counts it from the source), default: the row count.
------------------------------------------------------------------------------------------------------------------------------------
norm_forward   est_norm_fwd_r_kernel, est_norm_fwd_n_kernel<0>.  It is EPI_IN's chain with N in
               place of 100 and two changes, both written down here:
                 y = sum of the S partials in slice order (the _r kernel's first loop), the fp64 sum   dy    = (S - 1) u sum_s |Y_s|
                 mu = (sum y) * fl(1 / N)                                                       dmu   = mean(dy) + (n + 2) u mean|y|
                 d = y - mu                                   h = dy + u |d| is the part of d's error that differs from row to row,
                                                              dmu the part common to all rows:  dd    = h + dmu
                 q = sum d^2.  sum_i (d_i - delta + eta_i)^2 = q + N delta^2 + 2 sum (d_i - delta) eta_i + sum eta_i^2 because
                 sum d_i = 0: the mean's error enters q in SECOND order only.  (EPI_IN's 2 |d| dd counts it in first order; at a
                 mean of 40 that bound is too wide to tell a one-pass variance from a two-pass one.  N dmu^2 is kept although it is
                 second order: it is all there is for a constant channel.)
                                                         dq    = N dmu^2 + sum (2 (|d| + dmu) h + h^2) + (n + 2) u q
               merged statistics, est_norm_fwd_n_kernel<1> + <2> (the MODE 1 store and the MODE 2 merge): split t (n_t > 0 rows, R = ceil(N / S) apiece) leaves
               its own two-pass m_t, Q_t (dm_t, dQ_t as above with n_t for N); then over the T non-empty splits
                 mu = (sum_t fma(n_t, m_t)) / N                 dmu   = (sum n_t dm_t + T u sum n_t |m_t|) / N + u |mu|
                 d_t = m_t - mu                                 e_t   = dm_t + u |d_t|   (not common to the splits; dmu is)
                 Q = sum_t (Q_t + n_t d_t d_t)                  dQ    = sum dQ_t + sum n_t (2 (|d_t| + dmu) e_t + e_t^2) + N dmu^2
                                                                        + 2 u sum n_t d_t^2 + 2 T u Q
                 (sum n_t d_t = 0: the merged mean's error is second order here too.)  The VALUE is the same biased variance.
               then, as EPI_IN:  var = q fl(1 / N): dvar = dq / N + 2 u var;  v = var + eps: dv = dvar + u v;
                 rstd = 1 / sqrt(v): drstd = rstd (dv / (2 v) + 2 u);  k = rstd gamma: dk = |gamma| drstd + u |k|;
                 z = fma(d, k, beta): dz = |k| dd + |d| dk + u |z|;  a = z > 0 ? z : z slope: da = dz, or slope dz + u |a|
               planes: two fp16 max(2^-22 |a|, 2^-25), two bf16 2^-16 |a|, none (inorm_lrelu) 0.  undecided: |z| <= dz, widened by |z|.
adjoint_n      est_in_bwd_r_kernel, est_in_bwd_n_kernel (its `item` and the two loops over it), est_in_bwd_kernel.  Not EPI_INBWD's
               arithmetic: a = the fp32 sum of the two stored planes (exact: same bits on both sides),
                 d = sum of the S partials in slice order          dd    = (S - 1) u sum_s |dA_s|;  head form dl w: u |d|
                 z = a, or a fl(1 / slope)                          dzz   = 0, or 2 u |z|
                 e = d, or d slope                                  de    = dd, or slope dd + u |e|;  a == 0: + |d| |1 - slope|
                 x^ = (z - beta) fl(1 / gamma), 0 at |gamma| <= 1e-30    dx = (dzz + u |z - beta|) / |gamma| + 2 u |x^|
                 s1 = sum e (d beta of the pair)                    ds1   = sum de + n u sum|e|
                 s2 = sum fma(e, x^) (d gamma of the pair)          ds2   = sum (de |x^| + |e| dx) + (n + 1) u sum|e x^|
                 m1 = s1 fl(1 / N), m2 = s2 fl(1 / N)               dm    = ds / N + 2 u |m|
                 t = e - m1 - x^ m2 (contracted or not)             dt    = de + dm1 + dx |m2| + |x^| dm2 + u |x^ m2| + u |e - m1| + u |t|
                 dY = (rstd gamma) t                                |k| dt + 2 u |dY|, and 2^-16 |dY| for the two bf16 planes
               The split form (est_in_bwd_n_kernel<1> + <2>) adds the S partial sums in order: S more additions in n.
head_forward   est_head_fwd_kernel: C / 16 fused multiply-adds per lane, four cross-lane additions, the bias:
               (C / 16 + 5) u (sum|w a| + |bias|), a = the fp32 sum of the two fp16 planes (the kernel's own first operation).
head_dw        est_head_dw_kernel: block b owns columns [b cpb, min((b + 1) cpb, ncols)), cpb = ceil(ncols / blocks);
               a thread adds every eighth column, eight partial sums through LDS: (ceil(cpb / 8) + 8) u sum|dl a|; bias_part
               (ceil(cpb / 8) + 3) u sum|dl|.  A block without columns: exactly 0, both.
colsum         est_colsum_kernel (its WIDE and TALL branches): rows <= 32: rows additions in order; rows > 32: ceil(rows / 16) + 15.
dgamma_zero    est_dgamma_zero_kernel (the loop over pairs): y = W[ch] . x over Ci fused multiply-adds: dy = Ci u sum|W||x|;
               mean = (sum y) / N, n = ceil(N / 256) + 8: dmean = mean(dy) + (n + 1) u mean|y|;
               x^ = (y - mean) rstd: dx = rstd (dy + dmean + u |y - mean|) + u |x^|;
               d = dA (exact), dl w (u |d|), or dY_next[col] . W_next[:, ch] (C_next u sum|..|);  dz as e above;
               G = sum fma(dz, x^): sum (de |x^| + |dz| dx) + (n + 1) u sum|dz x^|.

Both of DESIGN.md's "Recorded, not fixed" notes of the GEMM section apply unchanged: the adjoints' 1e-30 threshold is their definition
(a |gamma| = 1e-29 channel is taken as live; the cases give it beta = 0 and a forward-sized activation).
"""
import torch

from est_gemm_ref import GAMMA_MIN, SLACK, TOL, U, block, compare, host_planes_bf16, host_planes_f16, stored_activation, unblock  # noqa: F401


def sum_parts(parts):
    """(value, bound) of the S partials [S, rows, C] added in slice order."""
    P = parts.double()
    return P.sum(0), (P.shape[0] - 1) * U * P.abs().sum(0)


def split_rows(N, S):
    """(begin, end) rows of each of the S splits of est_norm_fwd_n_kernel / est_in_bwd_n_kernel (their R, r0, r1); end <= begin: empty."""
    R = -(-N // S)
    return [(t * R, min(t * R + R, N)) for t in range(S)]


def _two_pass(Y, DY, n):
    """mean, its bound, q = sum of squared deviations, its bound of Y [pairs, rows, C] known to DY."""
    N = Y.shape[1]
    mu = Y.mean(1, keepdim=True)
    dmu = DY.mean(1, keepdim=True) + (n + 2) * U * Y.abs().mean(1, keepdim=True)
    d = Y - mu
    h = DY + U * d.abs()
    q = (d * d).sum(1, keepdim=True)
    dq = N * dmu ** 2 + (2 * (d.abs() + dmu) * h + h * h).sum(1, keepdim=True) + (n + 2) * U * q
    return mu, dmu, q, dq


def _merged(Y, DY, S, n):
    """The same from per-split statistics merged by Chan's formula."""
    N = Y.shape[1]
    live = [(a, b) for a, b in split_rows(N, S) if b > a]
    st = [_two_pass(Y[:, a:b], DY[:, a:b], n) for a, b in live]
    nt = [b - a for a, b in live]
    T = len(live)
    mu = sum(k * s[0] for k, s in zip(nt, st)) / N
    dmu = (sum(k * s[1] for k, s in zip(nt, st)) + T * U * sum(k * s[0].abs() for k, s in zip(nt, st))) / N + U * mu.abs()
    Q = torch.zeros_like(mu)
    dQ = N * dmu ** 2
    for k, (m, dm, q, dq) in zip(nt, st):
        dt = m - mu
        e = dm + U * dt.abs()
        Q = Q + q + k * dt * dt
        dQ = dQ + dq + k * (2 * (dt.abs() + dmu) * e + e * e) + 2 * U * k * dt * dt
    return mu, dmu, Q, dQ + 2 * T * U * Q


def norm_forward(Y_parts, N, gamma, beta, eps, slope, mode="two_pass", chain=None):
    """InstanceNorm + LeakyReLU of the sum of the partial products Y_parts [S, pairs * N, C] (fp32 values).  mode: "two_pass" (one
    workgroup holds the pair) or ("chan", splits).  chain: additions on the longest path of one row sum (of one split's, when merged).
    Returns a dict of float64 tensors: a, bound_f16, bound_bf16, bound_f32 [ncols, C], rstd, rstd_bound [pairs, C], undecided."""
    y, dy = sum_parts(Y_parts)
    ncols, C = y.shape
    pairs = ncols // N
    assert pairs * N == ncols
    g, b = gamma.double().view(1, 1, C), beta.double().view(1, 1, C)
    Y, DY = y.view(pairs, N, C), dy.view(pairs, N, C)
    if mode == "two_pass":
        mu, dmu, q, dq = _two_pass(Y, DY, N if chain is None else chain)
    else:
        mu, dmu, q, dq = _merged(Y, DY, mode[1], -(-N // mode[1]) if chain is None else chain)
    d = Y - mu
    dd = DY + dmu + U * d.abs()
    var = q / N
    dvar = dq / N + 2 * U * var
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
    a, da, und = a.reshape(ncols, C), da.reshape(ncols, C), und.reshape(ncols, C)
    return {"a": a, "bound_f16": SLACK * (da + torch.clamp(2.0 ** -22 * a.abs(), min=2.0 ** -25)),
            "bound_bf16": SLACK * (da + 2.0 ** -16 * a.abs()), "bound_f32": SLACK * da, "rstd": rstd.reshape(pairs, C),
            "rstd_bound": SLACK * drstd.reshape(pairs, C), "mean": mu.reshape(pairs, C), "mean_bound": SLACK * dmu.reshape(pairs, C),
            "undecided": und}


def _inv_gamma(g):
    live = g.abs() > GAMMA_MIN
    return torch.where(live, 1.0 / torch.where(live, g, torch.ones_like(g)), torch.zeros_like(g))


def _tail(E, DE, X, DX, k, N, n, plane):
    """s1, s2, dY and their bounds from e, x^ [pairs, N, C] (the part the three adjoints and inorm_lrelu's share)."""
    s1 = E.sum(1, keepdim=True)
    ds1 = DE.sum(1, keepdim=True) + n * U * E.abs().sum(1, keepdim=True)
    s2 = (E * X).sum(1, keepdim=True)
    ds2 = (DE * X.abs() + E.abs() * DX).sum(1, keepdim=True) + (n + 1) * U * (E * X).abs().sum(1, keepdim=True)
    m1, m2 = s1 / N, s2 / N
    dm1, dm2 = ds1 / N + 2 * U * m1.abs(), ds2 / N + 2 * U * m2.abs()
    t = E - m1 - X * m2
    dt = DE + dm1 + DX * m2.abs() + X.abs() * dm2 + U * (X * m2).abs() + U * (E - m1).abs() + U * t.abs()
    dY = k * t
    dYb = k.abs() * dt + 2 * U * dY.abs() + plane * dY.abs()
    return s1, ds1, s2, ds2, dY, dYb


def adjoint_n(up, a, rstd, gamma, beta, slope, N, chain=None):
    """The stand-alone InstanceNorm + LeakyReLU adjoints.  up: the partial gradients dA_parts [S, ncols, C] (fp32 values), or the
    head's rank-one form (dlogit [ncols], w_head [C]); a: stored_activation() of the layer's output planes [ncols, C]; rstd
    [pairs, C] as given.  Returns dY, dY_bound [ncols, C], dgamma_part, dgamma_bound, dbeta_part, dbeta_bound [pairs, C], undecided."""
    if isinstance(up, (tuple, list)):
        d = up[0].double()[:, None] * up[1].double()[None, :]
        dd = U * d.abs()
    else:
        d, dd = sum_parts(up)
    ncols, C = d.shape
    pairs = ncols // N
    n = N if chain is None else chain
    g, b = gamma.double().view(1, 1, C), beta.double().view(1, 1, C)
    a = a.double()
    pos = a > 0
    z = torch.where(pos, a, a / slope)
    dzz = torch.where(pos, torch.zeros_like(z), 2 * U * z.abs())
    e = torch.where(pos, d, d * slope)
    de = torch.where(pos, dd, slope * dd + U * e.abs())
    und = a.abs() < 2.0 ** -120
    de = torch.where(und, de + d.abs() * abs(1.0 - slope), de)
    Z, DZZ, E, DE = (t.view(pairs, N, C) for t in (z, dzz, e, de))
    ig = _inv_gamma(g)
    X = (Z - b) * ig
    DX = (DZZ + U * (Z - b).abs()) * ig.abs() + 2 * U * X.abs()
    k = rstd.double().view(pairs, 1, C) * g
    s1, ds1, s2, ds2, dY, dYb = _tail(E, DE, X, DX, k, N, n, 2.0 ** -16)
    return {"dY": dY.reshape(ncols, C), "dY_bound": SLACK * dYb.reshape(ncols, C), "dgamma_part": s2.reshape(pairs, C),
            "dgamma_bound": SLACK * ds2.reshape(pairs, C), "dbeta_part": s1.reshape(pairs, C), "dbeta_bound": SLACK * ds1.reshape(pairs, C),
            "undecided": und}


def adjoint_f32(gA, y, mean, rstd, gamma, beta, slope, chain=None):
    """inorm_lrelu_bwd_kernel (inorm.hip:97-129): the same adjoint from the fp32 pre-normalisation rows y [rows, N] of channels
    gamma / beta [rows] (already expanded per row), the saved mean and rstd [rows] as given, and the upstream gradient gA [rows, N]:
    x^ = (y - mean) rstd (2 u |x^|), the branch by the sign of fma(x^, gamma, beta) (undecided within its own 3 u (|x^ gamma| + |beta|):
    bound widened by |gA| |1 - slope|), e = gA or gA slope.  Returns gY, gY_bound [rows, N], row_ggamma, row_gbeta and bounds [rows]."""
    rows, N = y.shape
    n = N if chain is None else chain
    Y, G = y.double().view(rows, N, 1), gA.double().view(rows, N, 1)
    mu, rs = mean.double().view(rows, 1, 1), rstd.double().view(rows, 1, 1)
    g, b = gamma.double().view(rows, 1, 1), beta.double().view(rows, 1, 1)
    X = (Y - mu) * rs
    DX = 2 * U * X.abs()
    z = X * g + b
    dz = DX * g.abs() + U * ((X * g).abs() + b.abs())
    pos = z > 0
    E = torch.where(pos, G, G * slope)
    DE = torch.where(pos, torch.zeros_like(E), U * E.abs())
    und = z.abs() <= TOL * dz
    DE = torch.where(und, DE + G.abs() * abs(1.0 - slope), DE)
    s1, ds1, s2, ds2, dY, dYb = _tail(E, DE, X, DX, g * rs, N, n, 0.0)
    return {"gY": dY.reshape(rows, N), "gY_bound": SLACK * dYb.reshape(rows, N), "row_ggamma": s2.reshape(rows), "row_ggamma_bound": SLACK * ds2.reshape(rows),
            "row_gbeta": s1.reshape(rows), "row_gbeta_bound": SLACK * ds1.reshape(rows), "undecided": und.reshape(rows, N)}


def f16_activation(ap):
    """a as est_head_fwd_kernel reads it: the fp32 sum of the two fp16 planes, float64 [ncols, C]."""
    n, rows, C = ap.shape
    return unblock((ap[0].float() + ap[1].float()).view(1, rows, C))[0]


def head_forward(ap, w, bias):
    """(value, bound) [ncols] of logits[col] = sum_c w[c] a[col][c] + bias (bias: a one-element tensor or None)."""
    a = f16_activation(ap)
    C = a.shape[1]
    t = a * w.double()[None, :]
    b0 = 0.0 if bias is None else float(bias.double().reshape(-1)[0])
    return t.sum(1) + b0, SLACK * (C // 16 + 5) * U * (t.abs().sum(1) + abs(b0))


def head_blocks(ncols, blocks):
    """(begin, end) columns of each block of dfepe_est_head_dw (its cpb; c0, c1 of est_head_dw_kernel); end <= begin: the block owns none."""
    cpb = -(-ncols // blocks)
    return [(b * cpb, min(b * cpb + cpb, ncols)) for b in range(blocks)]


def head_dw(ap, dlogit, blocks):
    """(part, part_bound [blocks, C], bias_part, bias_bound [blocks]) from the backward's bf16 planes ap [>= 2, ncols, C]."""
    a = stored_activation(ap)
    dl = dlogit.double()
    ncols, C = a.shape
    cpb = -(-ncols // blocks)
    t = a * dl[:, None]
    part, dpart, bias, dbias = (torch.zeros(blocks, C, dtype=torch.float64), torch.zeros(blocks, C, dtype=torch.float64),
                                torch.zeros(blocks, dtype=torch.float64), torch.zeros(blocks, dtype=torch.float64))
    for i, (c0, c1) in enumerate(head_blocks(ncols, blocks)):
        if c1 > c0:
            part[i], dpart[i] = t[c0:c1].sum(0), (-(-cpb // 8) + 8) * U * t[c0:c1].abs().sum(0)
            bias[i], dbias[i] = dl[c0:c1].sum(), (-(-cpb // 8) + 3) * U * dl[c0:c1].abs().sum()
    return part, SLACK * dpart, bias, SLACK * dbias


def colsum(src):
    """(value, bound) [cols] of dst[c] = sum_r src[r][c]; src [rows, cols] (rows = 0: zeros, exactly)."""
    rows = src.shape[0]
    n = rows if rows <= 32 else -(-rows // 16) + 15
    s = src.double()
    return s.sum(0), SLACK * n * U * s.abs().sum(0)


def dgamma_zero(up, ap_out, ap_in, W, rstd, slope, N):
    """dfepe_est_dgamma_zero's per-pair d gamma of EVERY channel (the caller picks those with |gamma| <= 1e-30).  up: ("dA", dA [ncols, C]),
    ("head", dlogit, w_head) or ("next", dYn planes [2, ncols, Cn], W_next [Cn, C]); ap_out / ap_in: the layer's output / input bf16
    planes; W [C, Ci] fp32 (Ci <= the input planes' channels); rstd [pairs, C].  Returns (value, bound) [pairs, C]."""
    a, x = stored_activation(ap_out), stored_activation(ap_in)
    ncols, C = a.shape
    pairs = ncols // N
    Wd = W.double()
    Ci = Wd.shape[1]
    x = x[:, :Ci]
    y = x @ Wd.t()
    dy = Ci * U * (x.abs() @ Wd.abs().t())
    n = -(-N // 256) + 8
    Y, DY = y.view(pairs, N, C), dy.view(pairs, N, C)
    mean = Y.mean(1, keepdim=True)
    dmean = DY.mean(1, keepdim=True) + (n + 1) * U * Y.abs().mean(1, keepdim=True)
    rs = rstd.double().view(pairs, 1, C)
    X = (Y - mean) * rs
    DX = rs * (DY + dmean + U * (Y - mean).abs()) + U * X.abs()
    if up[0] == "dA":
        d = up[1].double()
        dd = torch.zeros_like(d)
    elif up[0] == "head":
        d = up[1].double()[:, None] * up[2].double()[None, :]
        dd = U * d.abs()
    else:
        dyn, Wn = stored_activation(up[1]), up[2].double()
        d = dyn @ Wn
        dd = Wn.shape[0] * U * (dyn.abs() @ Wn.abs())
    pos = a > 0
    e = torch.where(pos, d, d * slope)
    de = torch.where(pos, dd, slope * dd + U * e.abs())
    de = torch.where(a.abs() < 2.0 ** -120, de + d.abs() * abs(1.0 - slope), de)
    E, DE = e.view(pairs, N, C), de.view(pairs, N, C)
    G = (E * X).sum(1)
    dG = (DE * X.abs() + E.abs() * DX).sum(1) + (n + 1) * U * (E * X).abs().sum(1)
    return G, SLACK * dG
