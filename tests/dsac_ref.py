"""fp64 restatement of the DSAC hypothesis loop (deepFEPE/dsac_tools/dsac.py:37-92, :138-176, :194), one function per stage of
dfepe_dsac (include/dfepe.h).  Each stage takes the PREVIOUS stage's outputs as arguments, so a kernel is checked stage by stage on
its own intermediate results (the way tests/homography_ref.py is used), and each returns, next to its values, what bounds them.

The contract fixes where fp32 enters: the K^-1 points are rounded to fp32 before the fits read them, the refit's weights are
sqrt(soft) of the fp32 `soft` rounded to fp32, F = K^-T E K^-1 and the losses are formed from the fp32 E.  The restatement rounds at
the same places and computes everything else in float64, so what separates it from the kernel is the kernel's own arithmetic.

Stages 1 and 3 (the fits).  E is compared up to sign as a unit-Frobenius matrix.  Its conditioning term is
    term = e9 / (e2 - e1)  *  max(1, s1 / (s2 - s3))  *  cond(T1) cond(T2)
e1 <= .. <= e9 the eigenvalues of the (weighted) normal matrix of the Hartley-normalised design rows -- a perturbation of relative
size u of the rows turns the null vector by about u e9 / (e2 - e1) -- s1 >= s2 >= s3 the singular values of the 3x3 it reshapes
to (forcing them to (1,1,0) keeps the third singular vectors, which turn by about |dF| / (s2 - s3)), and T1, T2 the Hartley
transforms the result is carried back through.  The bound is C_FIT u32 term, u32 = 2^-24.  No existing test of ops.eight_point
derives such a constant (tests/test_compat_gpu.py holds it to fixed 5e-4 / 2e-5), so it is measured: C_FIT_MEASURED is the largest
|E - E64| / (u32 term) of ops.eight_point over the decided hypotheses of every shared case (scripts/dsac_time.py --measure-fit;
the figure is in profiles/dsac.md), and C_FIT = 4 C_FIT_MEASURED.  A hypothesis with C_FIT u32 term > TAU is undecided: a bound that
large says nothing about two unit matrices.

The "null" vector is V[:, -1] of torch.svd(XX, some=True) (utils_F.py:132-138), as the library's fits take it (csrc/w8pt16_body.h,
phase 4): with nine rows or more the right singular vector of the smallest singular value; with the eight rows of S = 8 the reduced
SVD has eight columns and V[:, -1] is the direction of the smallest NON-ZERO singular value, not the null vector of the 8x9 matrix.
Its gap is then the smaller of the distances to the eigenvalue above and to the zero below.
"""
import math

import numpy as np

U32 = 2.0 ** -24
SQRT2 = math.sqrt(2.0)
C_FIT_MEASURED = 1.2533e-3  # see the docstring; profiles/dsac.md has the run (MI355X; the host build of the fit kernels gives 1.14e-3)
C_FIT = 4.0 * C_FIT_MEASURED
TAU = 0.05            # a unit-Frobenius matrix pair further apart than this is not "equal within the bound" in any useful sense
F32 = np.float32


def _homo(P):
    return np.concatenate((P, np.ones(P.shape[:-1] + (1,))), -1)


def kinv_points(P, K):
    """_de_homo(K^-1 (x, y, 1)) with its 1e-10 guard (utils_F.py:111-112, utils_misc.py:69-78), rounded to fp32 as the contract says;
    P [...,N,2], K [...,3,3] -> float64 holding fp32 values."""
    Ki = np.linalg.inv(np.asarray(K, np.float64))
    Ph = _homo(np.asarray(P, np.float64)) @ np.swapaxes(Ki, -1, -2)
    return (Ph[..., :2] / (Ph[..., 2:3] + 1e-10)).astype(F32).astype(np.float64)


def _hartley(P):
    """T of _normalize_XY (utils_F.py:15-38) and the transformed points."""
    m = P.mean(0)
    s = SQRT2 / np.linalg.norm(P - m, axis=1).mean()
    T = np.array([[s, 0, -s * m[0]], [0, s, -s * m[1]], [0, 0, 1.0]])
    return (P - m) * s, T


def fit(xn, yn, w=None):
    """_E_from_XY after the K^-1 step (utils_F.py:114-155) on xn, yn [n,2] with row weights w [n] or None -> (E [3,3], term).
    A fit that is not finite, or whose gaps vanish, has term = inf."""
    with np.errstate(all="ignore"):
        X, T1 = _hartley(xn)
        Y, T2 = _hartley(yn)
        rows = np.stack((Y[:, 0] * X[:, 0], Y[:, 0] * X[:, 1], Y[:, 0], Y[:, 1] * X[:, 0], Y[:, 1] * X[:, 1], Y[:, 1], X[:, 0], X[:, 1],
                         np.ones(len(X))), 1)
        if w is not None:
            rows = rows * np.asarray(w, np.float64)[:, None]
        if not np.isfinite(rows).all():
            return np.full((3, 3), np.nan), math.inf
        _, sv, Vt = np.linalg.svd(rows, full_matrices=False)
        k = len(sv) - 1                               # V[:, -1] of the reduced SVD: the smallest of the min(n, 9) directions
        e = sv ** 2
        f = Vt[k]
        U, s, Wt = np.linalg.svd(f.reshape(3, 3))
        E = T2.T @ (U @ np.diag([1.0, 1.0, 0.0]) @ Wt) @ T1
        g9 = e[k - 1] - e[k] if len(rows) >= 9 else min(e[k - 1] - e[k], e[k])   # with 8 rows the null space lies below as well
        g3 = s[1] - s[2]
        if not (g9 > 0 and g3 > 0 and e[0] > 0 and np.isfinite(E).all()):
            return E, math.inf
        term = e[0] / g9 * max(1.0, s[0] / g3) * np.linalg.cond(T1) * np.linalg.cond(T2)
    return E, float(term)


def unit_diff(E, E64):
    """|E/|E| -+ E64/|E64||_F, the smaller of the two signs; inf when either is not finite."""
    E, E64 = np.asarray(E, np.float64), np.asarray(E64, np.float64)
    if not (np.isfinite(E).all() and np.isfinite(E64).all()) or not E.any() or not E64.any():
        return math.inf
    a, b = E / np.linalg.norm(E), E64 / np.linalg.norm(E64)
    return float(min(np.linalg.norm(a - b), np.linalg.norm(a + b)))


def fit_bound(term):
    return C_FIT * U32 * term


def decided(term):
    return fit_bound(term) <= TAU


def stage1(X, Y, K, idx):
    """Sample fits: X, Y [B,N,2], K [B,3,3], idx [B,H,S] -> E_sample [B,H,3,3], term [B,H]."""
    B, H = idx.shape[:2]
    xn, yn = kinv_points(X, K), kinv_points(Y, K)
    E, term = np.zeros((B, H, 3, 3)), np.zeros((B, H))
    for b in range(B):
        for h in range(H):
            E[b, h], term[b, h] = fit(xn[b][idx[b, h]], yn[b][idx[b, h]])
    return E, term


def e_to_f(E, K):
    Ki = np.linalg.inv(np.asarray(K, np.float64))
    return np.swapaxes(Ki, -1, -2) @ np.asarray(E, np.float64) @ Ki


def sampson(M, X, Y):
    """_sampson_dist (utils_F.py:291-308) of pixel points X, Y [N,2] under M [3,3] -> (d [N], bound [N]): the bound is that of
    the bilinear form evaluated with fp32 roundings, u32 times the sum of the absolute terms, carried through the quotient, plus
    the rounding of the output."""
    Xh, Yh = _homo(np.asarray(X, np.float64)), _homo(np.asarray(Y, np.float64))
    with np.errstate(all="ignore"):
        a, b = Xh @ M.T, Yh @ M                      # F x, F^T y
        s = (Yh * a).sum(1)
        den = a[:, 0] ** 2 + a[:, 1] ** 2 + b[:, 0] ** 2 + b[:, 1] ** 2
        d = s * s / den
        aa, ba = np.abs(Xh) @ np.abs(M).T, np.abs(Yh) @ np.abs(M)
        ds = U32 * (np.abs(Yh) * aa).sum(1)
        dden = 2 * U32 * (aa[:, 0] ** 2 + aa[:, 1] ** 2 + ba[:, 0] ** 2 + ba[:, 1] ** 2)
        bound = ((np.abs(s) + ds) ** 2 - s * s) / den + d * dden / den + U32 * np.abs(d)
    return d, bound


def soft_inlier(d, thresh, beta):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(beta * (d - thresh)))


def stage2(E_sample, X, Y, K, thresh, beta):
    """Given the kernel's fp32 E_sample [B,H,3,3]: d, soft [B,H,N], score [B,H] and their bounds
    (|soft - soft64| <= beta/4 |dd| + 2^-24: the logistic's slope is at most 1/4; score: the sum of those plus its own rounding)."""
    B, H = E_sample.shape[:2]
    N = X.shape[1]
    d, bd = np.zeros((B, H, N)), np.zeros((B, H, N))
    F = e_to_f(np.asarray(E_sample, np.float64), np.asarray(K, np.float64)[:, None])
    for b in range(B):
        for h in range(H):
            d[b, h], bd[b, h] = sampson(F[b, h], X[b], Y[b])
    soft = soft_inlier(d, thresh, beta)
    bs = abs(beta) / 4 * bd + U32
    score = soft.sum(2)
    return {"sampson": d, "sampson_bound": bd, "soft": soft, "soft_bound": bs, "score": score, "score_bound": bs.sum(2) + U32 * np.abs(score)}


def stage3(soft, X, Y, K):
    """Refits, given the kernel's fp32 soft [B,H,N]: the row weights are sqrt(soft) rounded to fp32 -> E_refit [B,H,3,3], term."""
    B, H = soft.shape[:2]
    xn, yn = kinv_points(X, K), kinv_points(Y, K)
    with np.errstate(invalid="ignore"):
        w = np.sqrt(np.asarray(soft, F32).astype(np.float64)).astype(F32).astype(np.float64)
    E, term = np.zeros((B, H, 3, 3)), np.zeros((B, H))
    for b in range(B):
        for h in range(H):
            E[b, h], term[b, h] = fit(xn[b], yn[b], w[b, h])
    return E, term


def stage4(E_refit, X, Y, K, loss_kind):
    """Given the kernel's fp32 E_refit: loss [B,H] (kind 1: HLoss(E_refit, X, Y) on the pixel points, dsac.py:157 with H_loss.py:28;
    kind 2: under K^-T E_refit K^-1; kind 0: zeros) and its bound, of stage 2's form."""
    B, H = E_refit.shape[:2]
    loss, bound = np.zeros((B, H)), np.zeros((B, H))
    if loss_kind == 0:
        return loss, bound
    M = np.asarray(E_refit, np.float64)
    if loss_kind == 2:
        M = e_to_f(M, np.asarray(K, np.float64)[:, None])
    for b in range(B):
        for h in range(H):
            d, bd = sampson(M[b, h], X[b], Y[b])
            loss[b, h] = d.mean()
            bound[b, h] = bd.mean() + U32 * abs(loss[b, h])
    return loss, bound


def vote(score, idx, N):
    """The reference's sequential float32 `+=` (dsac.py:163-165, :194), given fp32 scores [H] and idx [H,S] -> quality, counts [N]
    float32, bit for bit."""
    ns, nc = np.zeros(N, F32), np.zeros(N, F32)
    for h in range(len(score)):
        ns[idx[h]] += F32(score[h])
        nc[idx[h]] += F32(1.0)
    return ns / (nc + F32(1e-10)), nc


def first_best(score):
    """The first hypothesis whose score is the strict maximum above 0 (dsac.py:130, :168); -1 when none is."""
    best, top = -1, 0.0
    for h, s in enumerate(score):
        if s > top:
            best, top = h, s
    return best


def stage5(score, idx, N, loss=None, alpha=0.0, score64=None, score_bound=None):
    """Given the kernel's fp32 scores [B,H] and idx: quality, counts [B,N] (bitwise), best [B] (exact, from those scores), and with
    the fp64 scores of stage 2 and their bounds the set `near` [B] of hypotheses whose score is within the bounds of the top one;
    exp_loss [B] = sum_h softmax(alpha score)_h loss_h in fp64 with its bound 4 u32 sum_h p_h |loss_h| (the rounding of the output
    and the fp64 noise of H terms), top_loss [B]."""
    B, H = score.shape
    out = {"quality": np.zeros((B, N), F32), "counts": np.zeros((B, N), F32), "best": np.zeros(B, np.int64), "near": [],
           "exp_loss": np.zeros(B), "exp_loss_bound": np.zeros(B), "top_loss": np.zeros(B, F32)}
    for b in range(B):
        out["quality"][b], out["counts"][b] = vote(score[b], idx[b], N)
        out["best"][b] = first_best(score[b])
        if score64 is not None:
            lo = np.max(score64[b] - score_bound[b])
            out["near"].append(set(np.nonzero(score64[b] + score_bound[b] >= lo)[0].tolist()))
        if loss is not None:
            with np.errstate(all="ignore"):
                a = alpha * score[b].astype(np.float64)
                p = np.exp(a - a.max())
                p = p / p.sum()
                out["exp_loss"][b] = (p * loss[b]).sum()
                out["exp_loss_bound"][b] = 4 * U32 * (p * np.abs(loss[b])).sum()
            out["top_loss"][b] = loss[b][out["best"][b]] if out["best"][b] >= 0 else 0.0
    return out
