"""fp64 restatement of the adjoint of the DSAC loop (dfepe_dsac_bwd, include/dfepe.h), one function per stage.  In check()
(tests/dsac_adjoint_cases.py) each stage runs on the PREVIOUS stage's totals as the kernel wrote them, so what separates a stage from
the kernel is the kernel's own arithmetic.  The formulas are this file's own: the Sampson derivative is written out below, the two
fit adjoints come from tests/eight_point_adjoint_ref.py.

Every new stage returns, next to its value, its bound, derived the way tests/dsac_ref.py derives its bounds: u32 = 2^-24 times the sum
of the ABSOLUTE terms of the sum the stage forms (carried through K^-1 . K^-T where the stage does that), plus the rounding of the
output, u32 |value|.  The kernels compute in fp64, so no measured constant enters.

`pure` mode (pure_forward / pure_gradient): the whole chain in float64 without any fp32 rounding -- K^-1 points, fits, weights and
totals all stay float64 -- which is the function the reference's float64 autograd differentiates wherever that is finite.
"""
import numpy as np

import dsac_ref as dr
import eight_point_adjoint_ref as er

U32 = 2.0 ** -24
F32 = np.float32
MIN_GAP = 1e-6  # (lam_8 - lam_9) / lam_1 of a decided fit: eight_point_adjoint_cases.MIN_GAP_LAM


def f32(a):
    return np.asarray(a, np.float64).astype(F32).astype(np.float64)


def ident(a):
    return np.asarray(a, np.float64)


def _homo(P):
    return np.concatenate((P, np.ones(P.shape[:-1] + (1,))), -1)


def kinv_points(P, K, rnd=f32):
    Ki = np.linalg.inv(np.asarray(K, np.float64))
    Ph = _homo(np.asarray(P, np.float64)) @ np.swapaxes(Ki, -1, -2)
    return rnd(Ph[..., :2] / (Ph[..., 2:3] + 1e-10))


def sampson_grad(M, X, Y):
    """d = s^2 / D, s = y^T M x, D = a0^2 + a1^2 + b0^2 + b1^2, a = M x, b = M^T y, for pixel points X, Y [N,2]:
    (d [N], dd/dM [N,3,3], dd/dx [N,2], dd/dy [N,2]) and the same three sums with every term taken absolute."""
    Xh, Yh = _homo(np.asarray(X, np.float64)), _homo(np.asarray(Y, np.float64))
    with np.errstate(all="ignore"):
        a, b = Xh @ M.T, Yh @ M
        s = (Yh * a).sum(1)
        D = a[:, 0] ** 2 + a[:, 1] ** 2 + b[:, 0] ** 2 + b[:, 1] ** 2
        k1, k2 = 2 * s / D, s * s / (D * D)
        yx = Yh[:, :, None] * Xh[:, None, :]
        dD = np.zeros_like(yx)
        dD[:, :2, :] += 2 * a[:, :2, None] * Xh[:, None, :]
        dD[:, :, :2] += 2 * Yh[:, :, None] * b[:, None, :2]
        gM = k1[:, None, None] * yx - k2[:, None, None] * dD
        ax = 2 * (a[:, :2] @ M[:2, :2])            # dD/dx_c = 2 (a0 M_0c + a1 M_1c)
        by = 2 * (b[:, :2] @ M[:2, :2].T)          # dD/dy_r = 2 (b0 M_r0 + b1 M_r1)
        gx = k1[:, None] * b[:, :2] - k2[:, None] * ax
        gy = k1[:, None] * a[:, :2] - k2[:, None] * by
        aM = np.abs(k1)[:, None, None] * np.abs(yx) + k2[:, None, None] * np.abs(dD)
        ax_abs = 2 * (np.abs(a[:, :2]) @ np.abs(M[:2, :2]))
        by_abs = 2 * (np.abs(b[:, :2]) @ np.abs(M[:2, :2].T))
        agx = np.abs(k1)[:, None] * np.abs(b[:, :2]) + k2[:, None] * ax_abs
        agy = np.abs(k1)[:, None] * np.abs(a[:, :2]) + k2[:, None] * by_abs
    return s * s / D, gM, gx, gy, aM, agx, agy


def softmax_parts(score, loss, alpha):
    """p [B,H] and Lbar [B] in float64, max-subtracted."""
    with np.errstate(all="ignore"):
        a = alpha * np.asarray(score, np.float64)
        e = np.exp(a - a.max(1, keepdims=True))
        p = e / e.sum(1, keepdims=True)
    return p, (p * loss).sum(1)


def _z(g, shape):
    return np.zeros(shape) if g is None else np.asarray(g, np.float64)


def head(score, loss, counts, idx, alpha, g_score, g_loss, g_quality, g_exp_loss):
    """Stage 1 -> t_loss, t_score [B,H] and their bounds."""
    B, H = score.shape
    N = counts.shape[1]
    score, loss = np.asarray(score, np.float64), np.asarray(loss, np.float64)
    p, Lbar = softmax_parts(score, loss, alpha)
    ge = _z(g_exp_loss, (B,))[:, None]
    gl, gs = _z(g_loss, (B, H)), _z(g_score, (B, H))
    with np.errstate(all="ignore"):
        t_loss = gl + ge * p
        b_loss = U32 * (np.abs(gl) + np.abs(ge * p)) + U32 * np.abs(t_loss)
        e_term = ge * alpha * p * (loss - Lbar[:, None])
        # Lbar is itself a sum of H products: its terms enter the bound of the difference loss_h - Lbar
        e_abs = np.abs(ge * alpha) * p * (np.abs(loss) + (p * np.abs(loss)).sum(1)[:, None])
        t_score, a_score = gs + e_term, np.abs(gs) + e_abs
        if g_quality is not None:
            gq, cn = np.asarray(g_quality, np.float64), np.asarray(counts, np.float64)
            for b in range(B):
                for h in range(H):
                    for n in idx[b, h]:
                        if 0 <= n < N:
                            v = gq[b, n] / (cn[b, n] + 1e-10)
                            t_score[b, h] += v
                            a_score[b, h] += abs(v)
    return t_loss, b_loss, t_score, U32 * a_score + U32 * np.abs(t_score)


def _conj(Ki, G):
    return Ki @ G @ Ki.T


def loss_adjoint(E_refit, X, Y, K, kind, t_loss, g_E_refit):
    """Stage 2 -> t_E_refit [B,H,3,3] and its bound."""
    B, H = E_refit.shape[:2]
    N = X.shape[1]
    out = _z(g_E_refit, (B, H, 3, 3)).copy()
    bound = np.abs(out)
    Ki = np.linalg.inv(np.asarray(K, np.float64))
    if kind != 0:
        for b in range(B):
            for h in range(H):
                E = np.asarray(E_refit[b, h], np.float64)
                M = Ki[b].T @ E @ Ki[b] if kind == 2 else E
                _, gM, _, _, aM, _, _ = sampson_grad(M, X[b], Y[b])
                with np.errstate(all="ignore"):
                    k = float(t_loss[b, h]) / N
                    tM, tA = k * gM.sum(0), abs(k) * aM.sum(0)
                    if kind == 2:
                        tM, tA = _conj(Ki[b], tM), np.abs(Ki[b]) @ tA @ np.abs(Ki[b]).T
                out[b, h] += tM
                bound[b, h] += tA
    return out, U32 * bound + U32 * np.abs(out)


def refit_weights(soft, rnd=f32):
    with np.errstate(invalid="ignore"):
        return rnd(np.sqrt(np.asarray(soft, np.float64)))


def score_coeff(beta, s, w, t_score, t_w):
    """c [B,H,N]: s, w [B,H,N], t_score [B,H], t_w [B,H,N]."""
    with np.errstate(all="ignore"):
        return -beta * (1.0 - s) * (s * t_score[..., None] + 0.5 * w * t_w)


def score_adjoint(E_sample, X, Y, K, c, g_E_sample):
    """Stage 4 -> t_E_sample [B,H,3,3] and its bound."""
    B, H = E_sample.shape[:2]
    out = _z(g_E_sample, (B, H, 3, 3)).copy()
    bound = np.abs(out)
    Ki = np.linalg.inv(np.asarray(K, np.float64))
    for b in range(B):
        for h in range(H):
            F = Ki[b].T @ np.asarray(E_sample[b, h], np.float64) @ Ki[b]
            _, gM, _, _, aM, _, _ = sampson_grad(F, X[b], Y[b])
            with np.errstate(all="ignore"):
                tF = (c[b, h][:, None, None] * gM).sum(0)
                tA = (np.abs(c[b, h])[:, None, None] * aM).sum(0)
            out[b, h] += _conj(Ki[b], tF)
            bound[b, h] += np.abs(Ki[b]) @ tA @ np.abs(Ki[b]).T
    return out, U32 * bound + U32 * np.abs(out)


def fit_adjoint(xn, yn, w_hbn, E_bh, tE_bh):
    """The refits' adjoint (stage 3): xn, yn [B,N,2], w [H,B,N], E, t_E [B,H,3,3] -> er.adjoint's record (gX, gY summed over the sets,
    gw [H,B,N], gap_lam [H,B])."""
    with np.errstate(all="ignore"):
        return er.adjoint(xn, yn, w_hbn, True, True, np.swapaxes(E_bh, 0, 1), np.swapaxes(tE_bh, 0, 1))


def sample_adjoint(g1, g2, E_bh, tE_bh):
    """The sample fits' adjoint (stage 5): g1, g2 [B H,S,2] -> record with gX, gY [B H,S,2], gap_lam [1,B H]."""
    BH = g1.shape[0]
    with np.errstate(all="ignore"):
        return er.adjoint(g1, g2, None, True, True, E_bh.reshape(1, BH, 3, 3), tE_bh.reshape(1, BH, 3, 3))


def points(X, Y, K, idx, E_sample, E_refit, kind, c, t_loss, gpn1, gpn2, gg1, gg2):
    """Stage 6 -> g_X, g_Y [B,N,2] and their bounds, given the fit adjoints' outputs gpn [B,N,2] and gg [B,H,S,2]."""
    B, N = X.shape[:2]
    H, S = idx.shape[1:]
    Ki = np.linalg.inv(np.asarray(K, np.float64))
    out, bound = [np.zeros((B, N, 2)), np.zeros((B, N, 2))], [np.zeros((B, N, 2)), np.zeros((B, N, 2))]
    for b in range(B):
        G = [np.asarray(gpn1[b], np.float64).copy(), np.asarray(gpn2[b], np.float64).copy()]
        A = [np.abs(G[0]), np.abs(G[1])]
        D, DA = [np.zeros((N, 2)), np.zeros((N, 2))], [np.zeros((N, 2)), np.zeros((N, 2))]
        for h in range(H):
            for j in range(S):
                n = idx[b, h, j]
                if 0 <= n < N:
                    for i, gg in enumerate((gg1, gg2)):
                        G[i][n] += gg[b, h, j]
                        A[i][n] += np.abs(gg[b, h, j])
            F = Ki[b].T @ np.asarray(E_sample[b, h], np.float64) @ Ki[b]
            _, _, gx, gy, _, agx, agy = sampson_grad(F, X[b], Y[b])
            with np.errstate(all="ignore"):
                for i, (g, a) in enumerate(((gx, agx), (gy, agy))):
                    D[i] += c[b, h][:, None] * g
                    DA[i] += np.abs(c[b, h])[:, None] * a
                if kind != 0:
                    E = np.asarray(E_refit[b, h], np.float64)
                    M = Ki[b].T @ E @ Ki[b] if kind == 2 else E
                    _, _, gx, gy, _, agx, agy = sampson_grad(M, X[b], Y[b])
                    k = float(t_loss[b, h]) / N
                    for i, (g, a) in enumerate(((gx, agx), (gy, agy))):
                        D[i] += k * g
                        DA[i] += abs(k) * a
        for i, P in enumerate((X, Y)):
            ph = _homo(np.asarray(P[b], np.float64)) @ Ki[b].T      # (u, v, w)
            ig = 1.0 / (ph[:, 2] + 1e-10)
            with np.errstate(all="ignore"):
                gu, gv = G[i][:, 0] * ig, G[i][:, 1] * ig
                gw = -(G[i][:, 0] * ph[:, 0] + G[i][:, 1] * ph[:, 1]) * ig * ig
                au, av = A[i][:, 0] * np.abs(ig), A[i][:, 1] * np.abs(ig)
                aw = (A[i][:, 0] * np.abs(ph[:, 0]) + A[i][:, 1] * np.abs(ph[:, 1])) * ig * ig
                J = np.stack((gu * Ki[b, 0, 0] + gv * Ki[b, 1, 0] + gw * Ki[b, 2, 0], gu * Ki[b, 0, 1] + gv * Ki[b, 1, 1] + gw * Ki[b, 2, 1]), 1)
                JA = np.stack((au * abs(Ki[b, 0, 0]) + av * abs(Ki[b, 1, 0]) + aw * abs(Ki[b, 2, 0]),
                               au * abs(Ki[b, 0, 1]) + av * abs(Ki[b, 1, 1]) + aw * abs(Ki[b, 2, 1])), 1)
                out[i][b] = J + D[i]
                bound[i][b] = U32 * (JA + DA[i]) + U32 * np.abs(out[i][b])
    return out[0], bound[0], out[1], bound[1]


def gather(P, idx):
    """P [B,N,2], idx [B,H,S] -> [B H,S,2] with the forward's clamp."""
    B, N = P.shape[:2]
    ix = np.clip(idx, 0, N - 1)
    return np.stack([P[b][ix[b]] for b in range(B)]).reshape(-1, idx.shape[2], 2)


def chain(X, Y, K, idx, beta, alpha, kind, fwd, up, rnd=f32):
    """The whole adjoint on the forward values `fwd` (E_sample, soft, score, E_refit, loss, counts) and upstreams `up` (by output name;
    missing = 0).  rnd = f32: every total is rounded where the kernel rounds it; rnd = ident: the pure chain.  Returns every total."""
    B, H, S = idx.shape
    r = {}
    r["t_loss"], _, r["t_score"], _ = head(fwd["score"], fwd["loss"], fwd["counts"], idx, alpha, up.get("score"), up.get("loss"),
                                           up.get("quality"), up.get("exp_loss"))
    r["t_loss"], r["t_score"] = rnd(r["t_loss"]), rnd(r["t_score"])
    r["t_E_refit"] = rnd(loss_adjoint(fwd["E_refit"], X, Y, K, kind, r["t_loss"], up.get("E_refit"))[0])
    xn, yn = kinv_points(X, K, rnd), kinv_points(Y, K, rnd)
    s = np.asarray(fwd["soft"], np.float64)
    w = refit_weights(s, rnd)
    fa = fit_adjoint(xn, yn, np.ascontiguousarray(np.swapaxes(w, 0, 1)), np.asarray(fwd["E_refit"], np.float64), r["t_E_refit"])
    r["t_w"], r["gpn1"], r["gpn2"] = rnd(fa.gw), rnd(fa.gX), rnd(fa.gY)
    r["c"] = score_coeff(beta, s, w, r["t_score"], np.swapaxes(r["t_w"], 0, 1))
    r["t_E_sample"] = rnd(score_adjoint(fwd["E_sample"], X, Y, K, r["c"], up.get("E_sample"))[0])
    sa = sample_adjoint(gather(xn, idx), gather(yn, idx), np.asarray(fwd["E_sample"], np.float64), r["t_E_sample"])
    r["gg1"], r["gg2"] = rnd(sa.gX).reshape(B, H, S, 2), rnd(sa.gY).reshape(B, H, S, 2)
    r["g_X"], _, r["g_Y"], _ = points(X, Y, K, idx, fwd["E_sample"], fwd["E_refit"], kind, r["c"], r["t_loss"], r["gpn1"], r["gpn2"],
                                      r["gg1"], r["gg2"])
    r["gap_refit"], r["gap_sample"] = np.swapaxes(fa.gap_lam, 0, 1), sa.gap_lam.reshape(B, H)
    return r


# ---- pure mode ----------------------------------------------------------------------------------------------------------------------------
def hartley(P):
    """T of _normalize_XY (utils_F.py:15-38) for P [n,2]."""
    m = P.mean(0)
    sc = np.sqrt(2.0) / np.linalg.norm(P - m, axis=1).mean()
    return np.array([[sc, 0, -sc * m[0]], [0, sc, -sc * m[1]], [0, 0, 1.0]])


def pure_fit(xn, yn, w=None, T=None):
    """_E_from_XY after the K^-1 step in float64 (n >= 9 rows) -> (E, (T1, T2)).  T given: the Hartley transforms are held at those
    values, which is how the adjoint (and the reference's autograd, utils_F.py:25,35) treats them."""
    T1, T2 = (hartley(xn), hartley(yn)) if T is None else T
    a, b = _homo(xn) @ T1.T, _homo(yn) @ T2.T
    rows = (b[:, :, None] * a[:, None, :]).reshape(len(xn), 9)
    if w is not None:
        rows = rows * np.asarray(w, np.float64)[:, None]
    Vt = np.linalg.svd(rows, full_matrices=False)[2]
    U, _, Wt = np.linalg.svd(Vt[-1].reshape(3, 3))
    return T2.T @ (U @ np.diag([1.0, 1.0, 0.0]) @ Wt) @ T1, (T1, T2)


def pure_forward(X, Y, K, idx, thresh, beta, alpha, kind, frozen=None):
    """dfepe_dsac's stages in float64 with no fp32 rounding anywhere (quality included) -> dict.  `frozen`: the "T" entry of an earlier
    call, to hold every fit's Hartley transforms at that call's values (for finite differences of the function the adjoint
    differentiates)."""
    X, Y, K = (np.asarray(a, np.float64) for a in (X, Y, K))
    B, N = X.shape[:2]
    H = idx.shape[1]
    xn, yn = kinv_points(X, K, ident), kinv_points(Y, K, ident)
    Ki = np.linalg.inv(K)
    f = {"E_sample": np.zeros((B, H, 3, 3)), "E_refit": np.zeros((B, H, 3, 3)), "soft": np.zeros((B, H, N)), "score": np.zeros((B, H)),
         "loss": np.zeros((B, H)), "counts": np.zeros((B, N)), "quality": np.zeros((B, N)), "T": {}}
    for b in range(B):
        for h in range(H):
            f["E_sample"][b, h], f["T"][b, h, 0] = pure_fit(xn[b][idx[b, h]], yn[b][idx[b, h]], None, frozen and frozen[b, h, 0])
            d = sampson_grad(Ki[b].T @ f["E_sample"][b, h] @ Ki[b], X[b], Y[b])[0]
            f["soft"][b, h] = dr.soft_inlier(d, thresh, beta)
            f["score"][b, h] = f["soft"][b, h].sum()
            f["E_refit"][b, h], f["T"][b, h, 1] = pure_fit(xn[b], yn[b], np.sqrt(f["soft"][b, h]), frozen and frozen[b, h, 1])
            if kind:
                M = Ki[b].T @ f["E_refit"][b, h] @ Ki[b] if kind == 2 else f["E_refit"][b, h]
                f["loss"][b, h] = sampson_grad(M, X[b], Y[b])[0].mean()
            f["counts"][b, idx[b, h]] += 1
            f["quality"][b, idx[b, h]] += f["score"][b, h]
    f["quality"] = f["quality"] / (f["counts"] + 1e-10)
    p, f["exp_loss"] = softmax_parts(f["score"], f["loss"], alpha)
    return f


def pure_gradient(X, Y, K, idx, thresh, beta, alpha, kind, up):
    """(g_X, g_Y) of sum(up . outputs) in pure float64, and the forward values."""
    f = pure_forward(X, Y, K, idx, thresh, beta, alpha, kind)
    r = chain(np.asarray(X, np.float64), np.asarray(Y, np.float64), np.asarray(K, np.float64), idx, beta, alpha, kind, f, up, rnd=ident)
    return r["g_X"], r["g_Y"], f
