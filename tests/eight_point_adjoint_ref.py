"""fp64 restatement of the adjoint of the textbook normalised eight-point solvers (dfepe_eight_point_bwd, include/dfepe.h;
csrc/eight_point_adjoint_math.h), with numpy.linalg.svd (of the design matrix A itself for the eigenpairs of A^T A, and of the
3x3), and a 50-digit mpmath twin of one problem.  The twin applies no N = 8 rule: it is the independent check of that rule.

A problem is one pair under one weight set.  Forward, recomputed from the float32 inputs widened exactly:
  per image (normalize): c = mean p, s = sqrt(2) / mean |p - c|, p~ = s (p - c) / (1 + 1e-10), T = [[s,0,-s cx],[0,s,-s cy],[0,0,1]]
  a_i = [x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1], A_i = w_i a_i, M9 = A^T A, f = its eigenvector of the smallest eigenvalue
  F0 = reshape(f) = U diag(s1,s2,s3) V^T, M = U diag(s1,s2,0) V^T (essential: diag(1,1,0)), out = T2^T M T1, oriented to F_out
Adjoint with T1, T2 constant (the reference detaches them, utils_F.py:25,35):
  G^ = U^T (T2 g_F T1^T) V, g_F0 = U P V^T (P as in the header), u = sum_{k != 9} q_k (q_k . g_f) / (lam_9 - lam_k),
  g_A_i = (A_i . f) u + (A_i . u) f (A_i . f is the constant 0 when N = 8: eight rows have an exact null vector),
  g_w_i = a_i . g_A_i, g_a_i = w_i g_A_i, to the points by the product rule and s / (1 + 1e-10).
Guard rule, restated: every denominator lam_9 - lam_k, s_k^2 - s3^2, s1 + s2 keeps its sign and has its magnitude floored at 1e-30.
The twin has no guard: it is only asked where no denominator vanishes."""
from types import SimpleNamespace

import numpy as np

DEHOMO = 1.0 + 1e-10
GUARD = 1e-30


def guard_den(d):
    return np.where(np.abs(d) < GUARD, np.where(d < 0, -GUARD, GUARD), d)


def _hartley(P, normalize):
    """P [N,2] float64 -> (normalised points, T [3,3], scale of the gradient)."""
    if not normalize:
        return P, np.eye(3), 1.0
    c = P.mean(0)
    s = np.sqrt(2.0) / np.sqrt(((P - c) ** 2).sum(1)).mean()
    T = np.array([[s, 0.0, -s * c[0]], [0.0, s, -s * c[1]], [0.0, 0.0, 1.0]])
    return s * (P - c) / DEHOMO, T, s / DEHOMO


def _rows(p1, p2):
    x1, y1, x2, y2 = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    return np.stack((x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, np.ones_like(x1)), 1)


def rank2_P(Gh, s, essential):
    """P of g_F0 = U P V^T from G^ = U^T G V and the singular values."""
    P = np.zeros((3, 3)) if essential else Gh.copy()
    P[2, 2] = 0.0
    if essential:
        P[0, 1] = (Gh[0, 1] - Gh[1, 0]) / guard_den(s[0] + s[1])
        P[1, 0] = -P[0, 1]
    for k in range(2):
        dk = guard_den(s[k] * s[k] - s[2] * s[2])
        gk3, g3k = Gh[k, 2], Gh[2, k]
        if essential:
            P[k, 2] = (s[k] * gk3 + s[2] * g3k) / dk
            P[2, k] = (s[2] * gk3 + s[k] * g3k) / dk
        else:
            P[k, 2] = gk3 + s[2] * (s[2] * gk3 + s[k] * g3k) / dk
            P[2, k] = g3k + s[2] * (s[k] * gk3 + s[2] * g3k) / dk
    return P


def problem(X, Y, w, essential, normalize, F_out, g_F):
    """One problem.  X, Y [N,2], w [N] or None, F_out, g_F [3,3] (None: forward only).  Everything float64."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    N = X.shape[0]
    w = np.ones(N) if w is None else np.asarray(w, np.float64)
    r = SimpleNamespace(gX=np.full((N, 2), np.nan), gY=np.full((N, 2), np.nan), gw=np.full(N, np.nan), out=np.full((3, 3), np.nan),
                        gap_lam=np.nan, gap_s=np.nan, s=np.full(3, np.nan), gw_df=np.full(N, np.nan))
    if not (np.isfinite(X).all() and np.isfinite(Y).all() and np.isfinite(w).all()):
        return r
    p1, T1, sc1 = _hartley(X, normalize)
    p2, T2, sc2 = _hartley(Y, normalize)
    a = _rows(p1, p2)
    A = a * w[:, None]
    # the eigenpairs of M9 = A^T A from the SVD of A itself (lam = sigma^2, q = right singular vectors): not the kernel's route, and
    # the small singular values keep their relative accuracy, which the residual A f of a nearly exact fit needs
    _, sig, Vt = np.linalg.svd(A, full_matrices=True)
    lam = np.concatenate((sig, np.zeros(9 - len(sig))))[::-1] ** 2  # ascending; N = 8 has lam_9 = 0
    Q = Vt.T[:, ::-1]
    f = Q[:, 0]
    U, s, Vt = np.linalg.svd(f.reshape(3, 3))
    V = Vt.T
    D = np.diag([1.0, 1.0, 0.0]) if essential else np.diag([s[0], s[1], 0.0])
    out = T2.T @ (U @ D @ V.T) @ T1
    r.gap_lam, r.gap_s, r.s = (lam[1] - lam[0]) / lam[-1], (s[1] - s[2]) / s[0], s
    if F_out is not None and (out * np.asarray(F_out, np.float64)).sum() < 0:
        f, U, out = -f, -U, -out
    r.out = out
    if g_F is None:
        return r
    Gh = U.T @ (T2 @ np.asarray(g_F, np.float64) @ T1.T) @ V
    gf = (U @ rank2_P(Gh, s, essential) @ V.T).reshape(9)
    coef = (Q[:, 1:].T @ gf) / guard_den(lam[0] - lam[1:])
    u = Q[:, 1:] @ coef
    Af = np.zeros(N) if N == 8 else A @ f  # eight rows, nine unknowns: A f = 0 exactly
    gA = np.outer(Af, u) + np.outer(A @ u, f)
    r.gw = np.zeros(N) if N == 8 else (a * gA).sum(1)  # = 2 w (a . f)(a . u)
    r.gw_df = 2.0 * w * np.sqrt((a * a).sum(1)) * np.abs(a @ u)  # |d g_w,i| per unit |d f|, to first order
    ga = gA * w[:, None]
    r.gX = sc1 * np.stack((ga[:, 0] * p2[:, 0] + ga[:, 3] * p2[:, 1] + ga[:, 6], ga[:, 1] * p2[:, 0] + ga[:, 4] * p2[:, 1] + ga[:, 7]), 1)
    r.gY = sc2 * np.stack((ga[:, 0] * p1[:, 0] + ga[:, 1] * p1[:, 1] + ga[:, 2], ga[:, 3] * p1[:, 0] + ga[:, 4] * p1[:, 1] + ga[:, 5]), 1)
    return r


def forward(X, Y, w, essential, normalize):
    """out [S,B,3,3] in float64 (LAPACK's sign), and the two gap figures [S,B]: (lam_8 - lam_9) / lam_1 and (s2 - s3) / s1."""
    B = X.shape[0]
    S = 1 if w is None else w.shape[0]
    out, gl, gs = np.empty((S, B, 3, 3)), np.empty((S, B)), np.empty((S, B))
    for s in range(S):
        for b in range(B):
            r = problem(X[b], Y[b], None if w is None else w[s, b], essential, normalize, None, None)
            out[s, b], gl[s, b], gs[s, b] = r.out, r.gap_lam, r.gap_s
    return out, gl, gs


def adjoint(X, Y, w, essential, normalize, F_out, g_F):
    """The whole call: X, Y [B,N,2], w [S,B,N] or None, F_out, g_F [S,B,3,3] -> gX, gY [B,N,2] (the sets added in order), gw [S,B,N],
    per-set point gradients gXs, gYs [S,B,N,2], out [S,B,3,3] and the gap figures [S,B]."""
    B, N = X.shape[:2]
    S = F_out.shape[0]
    r = SimpleNamespace(gXs=np.empty((S, B, N, 2)), gYs=np.empty((S, B, N, 2)), gw=np.empty((S, B, N)), out=np.empty((S, B, 3, 3)),
                        gap_lam=np.empty((S, B)), gap_s=np.empty((S, B)), gw_df=np.empty((S, B, N)))
    for s in range(S):
        for b in range(B):
            q = problem(X[b], Y[b], None if w is None else w[s, b], essential, normalize, F_out[s, b], g_F[s, b])
            r.gw_df[s, b] = q.gw_df
            r.gXs[s, b], r.gYs[s, b], r.gw[s, b], r.out[s, b] = q.gX, q.gY, q.gw, q.out
            r.gap_lam[s, b], r.gap_s[s, b] = q.gap_lam, q.gap_s
    r.gX, r.gY = r.gXs[0].copy(), r.gYs[0].copy()
    for s in range(1, S):
        r.gX += r.gXs[s]
        r.gY += r.gYs[s]
    return r


def twin(X, Y, w, essential, normalize, F_out, g_F, digits=50):
    """The 50-digit twin of problem(): returns (gX [N,2], gY [N,2], gw [N]) as float64 arrays rounded from mpmath values."""
    import mpmath as mp

    with mp.workdps(digits):
        N = len(X)
        mpf = mp.mpf
        one = mpf(1)
        dehomo = one + mpf("1e-10")
        wv = [one] * N if w is None else [mpf(float(v)) for v in w]

        def hartley(P):
            P = [(mpf(float(x)), mpf(float(y))) for x, y in P]
            if not normalize:
                return P, mp.eye(3), one
            cx, cy = mp.fsum(p[0] for p in P) / N, mp.fsum(p[1] for p in P) / N
            s = mp.sqrt(2) / (mp.fsum(mp.sqrt((p[0] - cx) ** 2 + (p[1] - cy) ** 2) for p in P) / N)
            T = mp.matrix([[s, 0, -s * cx], [0, s, -s * cy], [0, 0, 1]])
            return [(s * (p[0] - cx) / dehomo, s * (p[1] - cy) / dehomo) for p in P], T, s / dehomo

        p1, T1, sc1 = hartley(X)
        p2, T2, sc2 = hartley(Y)
        a = [[q[0] * p[0], q[0] * p[1], q[0], q[1] * p[0], q[1] * p[1], q[1], p[0], p[1], one] for p, q in zip(p1, p2)]
        M9 = mp.zeros(9, 9)
        for i in range(9):
            for j in range(i, 9):
                M9[i, j] = M9[j, i] = mp.fsum((wv[n] * a[n][i]) * (wv[n] * a[n][j]) for n in range(N))
        lam, Q = mp.eigsy(M9)  # ascending
        k9 = min(range(9), key=lambda k: lam[k])
        f = [Q[c, k9] for c in range(9)]
        F0 = mp.matrix(3, 3)
        for c in range(9):
            F0[c // 3, c % 3] = f[c]
        U, s, Vt = mp.svd_r(F0)
        V = Vt.T
        D = mp.diag([one, one, 0]) if essential else mp.diag([s[0], s[1], 0])
        out = T2.T * (U * D * V.T) * T1
        dot = mp.fsum(out[i, j] * mpf(float(F_out[i][j])) for i in range(3) for j in range(3))
        if dot < 0:
            f, U = [-v for v in f], -U
        g = mp.matrix([[mpf(float(g_F[i][j])) for j in range(3)] for i in range(3)])
        Gh = U.T * (T2 * g * T1.T) * V
        P = mp.zeros(3, 3) if essential else Gh.copy()
        P[2, 2] = 0
        if essential:
            P[0, 1] = (Gh[0, 1] - Gh[1, 0]) / (s[0] + s[1])
            P[1, 0] = -P[0, 1]
        for k in range(2):
            dk = s[k] ** 2 - s[2] ** 2
            gk3, g3k = Gh[k, 2], Gh[2, k]
            if essential:
                P[k, 2] = (s[k] * gk3 + s[2] * g3k) / dk
                P[2, k] = (s[2] * gk3 + s[k] * g3k) / dk
            else:
                P[k, 2] = gk3 + s[2] * (s[2] * gk3 + s[k] * g3k) / dk
                P[2, k] = g3k + s[2] * (s[k] * gk3 + s[2] * g3k) / dk
        gF0 = U * P * V.T
        gf = [gF0[c // 3, c % 3] for c in range(9)]
        u = [mpf(0)] * 9
        for k in range(9):
            if k == k9:
                continue
            coef = mp.fsum(Q[c, k] * gf[c] for c in range(9)) / (lam[k9] - lam[k])
            u = [u[c] + coef * Q[c, k] for c in range(9)]
        gX, gY, gw = np.empty((N, 2)), np.empty((N, 2)), np.empty(N)
        for n in range(N):
            af = mp.fsum(a[n][k] * f[k] for k in range(9))  # no N = 8 rule here: at 50 digits A f = 0 shows by itself
            au = mp.fsum(a[n][k] * u[k] for k in range(9))
            gA = [wv[n] * af * u[k] + wv[n] * au * f[k] for k in range(9)]
            gw[n] = float(mp.fsum(a[n][k] * gA[k] for k in range(9)))
            ga = [wv[n] * v for v in gA]
            x1, y1, x2, y2 = p1[n][0], p1[n][1], p2[n][0], p2[n][1]
            gX[n] = (float(sc1 * (ga[0] * x2 + ga[3] * y2 + ga[6])), float(sc1 * (ga[1] * x2 + ga[4] * y2 + ga[7])))
            gY[n] = (float(sc2 * (ga[0] * x1 + ga[1] * y1 + ga[2])), float(sc2 * (ga[3] * x1 + ga[4] * y1 + ga[5])))
        return gX, gY, gw
