"""fp64 restatement of the five-point RANSAC essential-matrix estimator the tests hold csrc/ransac5.hip and csrc/ransac5_math.h
to: OpenCV 3.4's findEssentialMat(RANSAC) as include/dfepe.h (dfepe_ransac_essential) specifies it -- sampler, five-point solve,
Sampson error, RANSACUpdateNumIters with exponent 5 and the sequential selection rule with ten slots.  numpy only; written from
the published algorithm (Stewenius, Engels, Nister 2006), independently of the kernels: the null space comes from numpy's SVD,
the ten cubics are reduced to the action matrix of x on the monomials of degree <= 2, and its eigenvectors give the solutions
(the kernels eliminate towards a degree-10 polynomial in z and polish)."""
import math

import numpy as np

from ransac_ref import DBL_MIN, Stream

NO_ROOT = -1
LIN = (16, 4, 1, 0)  # codes of x, y, z, 1: a monomial x^i y^j z^k is 16 i + 4 j + k, and codes add under multiplication
CUBIC = [16 * i + 4 * j + k for i in range(4) for j in range(4) for k in range(4) if i + j + k == 3]
BASIS = [32, 20, 17, 8, 5, 2, 16, 4, 1, 0]  # x^2 xy xz y^2 yz z^2 x y z 1


def draw_sample(seed, k, N):
    """Iteration k's five distinct indices (no geometric rejection)."""
    s, idx = Stream(seed, k), []
    while len(idx) < 5:
        v = s.index(N)
        if v not in idx:
            idx.append(v)
    return idx


def normalize(pts, K):
    """float32 pixels [N,4], K [3,3] -> fp64 normalised coordinates [N,4]."""
    p = np.asarray(pts, np.float32).astype(np.float64)
    K = np.asarray(K, np.float32).astype(np.float64).reshape(3, 3)
    return np.stack([(p[:, 0] - K[0, 2]) / K[0, 0], (p[:, 1] - K[1, 2]) / K[1, 1],
                     (p[:, 2] - K[0, 2]) / K[0, 0], (p[:, 3] - K[1, 2]) / K[1, 1]], 1)


def threshold2(threshold, K):
    K = np.asarray(K, np.float32).astype(np.float64).reshape(3, 3)
    t = threshold / ((K[0, 0] + K[1, 1]) / 2.0)
    return t * t


def unit(E):
    """Unit Frobenius norm, the entry of largest magnitude positive."""
    e = np.asarray(E, np.float64).ravel()
    e = e / np.linalg.norm(e)
    return e * np.sign(e[np.argmax(np.abs(e))])


def _mul_lin(p, l):
    """p (64 coefficients by code) times a linear form l (x, y, z, 1)."""
    out = np.zeros(64)
    for a in range(4):
        c = LIN[a]
        out[c:] += p[:64 - c] * l[a]
    return out


def _lin(l):
    out = np.zeros(64)
    out[list(LIN)] = l
    return out


def five_point(q5):
    """q5 [5,4] normalised coordinates -> list of unit-norm, sign-fixed E [3,3] (q2^T E q1 = 0), one per real solution."""
    q5 = np.asarray(q5, np.float64)
    x1, y1, x2, y2 = q5.T
    A = np.stack([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, np.ones(5)], 1)
    NS = np.linalg.svd(A)[2][5:9]  # X, Y, Z, W as rows of 9
    e = [[NS[:, 3 * i + j] for j in range(3)] for i in range(3)]  # E_ij as a linear form in (x, y, z, 1)
    EEt = [[sum(_mul_lin(_lin(e[i][j]), e[k][j]) for j in range(3)) for k in range(3)] for i in range(3)]
    tr = EEt[0][0] + EEt[1][1] + EEt[2][2]
    rows = []
    for i in range(3):
        for j in range(3):
            rows.append(2.0 * sum(_mul_lin(EEt[i][k], e[k][j]) for k in range(3)) - _mul_lin(tr, e[i][j]))
    det = (_mul_lin(_mul_lin(_lin(e[1][1]), e[2][2]) - _mul_lin(_lin(e[1][2]), e[2][1]), e[0][0])
           - _mul_lin(_mul_lin(_lin(e[1][0]), e[2][2]) - _mul_lin(_lin(e[1][2]), e[2][0]), e[0][1])
           + _mul_lin(_mul_lin(_lin(e[1][0]), e[2][1]) - _mul_lin(_lin(e[1][1]), e[2][0]), e[0][2]))
    rows.append(det)
    M = np.array(rows)
    C, Bm = M[:, CUBIC], M[:, BASIS]
    try:
        Rm = np.linalg.solve(C, Bm)  # cubic monomial c = -Rm[c] . basis
    except np.linalg.LinAlgError:
        return []
    Ax = np.zeros((10, 10))
    for i, b in enumerate(BASIS):
        m = b + 16  # x times the basis monomial
        if m in BASIS:
            Ax[i, BASIS.index(m)] = 1.0
        else:
            Ax[i] = -Rm[CUBIC.index(m)]
    lam, V = np.linalg.eig(Ax)
    out = []
    for i in range(10):
        if abs(lam[i].imag) > 1e-9 * (1.0 + abs(lam[i])):
            continue
        v = V[:, i].real
        if v[9] == 0.0:
            continue
        v = v / v[9]
        out.append(unit(v[6] * NS[0] + v[7] * NS[1] + v[8] * NS[2] + NS[3]).reshape(3, 3))
    return out


def constraint_residuals(E):
    """(max |2 E E^T E - tr(E E^T) E|, |det E|)."""
    E = np.asarray(E, np.float64).reshape(3, 3)
    T = E @ E.T
    return float(np.abs(2.0 * T @ E - np.trace(T) * E).max()), float(abs(np.linalg.det(E)))


def sampson(E, q):
    """OpenCV's EMEstimatorCallback::computeError per correspondence of q [N,4] (normalised), fp64."""
    E = np.asarray(E, np.float64).reshape(3, 3)
    q = np.asarray(q, np.float64)
    h1 = np.c_[q[:, :2], np.ones(len(q))]
    h2 = np.c_[q[:, 2:], np.ones(len(q))]
    Eq1 = h1 @ E.T
    Etq2 = h2 @ E
    r = (h2 * Eq1).sum(1)
    return r * r / (Eq1[:, 0] ** 2 + Eq1[:, 1] ** 2 + Etq2[:, 0] ** 2 + Etq2[:, 1] ** 2)


def update_num_iters(p, ep, niters):
    """OpenCV's RANSACUpdateNumIters(p, ep, 5, niters), (1 - ep)^5 by the same multiplications as the kernels."""
    p = min(max(p, 0.0), 1.0)
    ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, DBL_MIN)
    q = 1.0 - ep
    q2 = q * q
    q4 = q2 * q2
    den = 1.0 - q4 * q
    if den < DBL_MIN:
        return 0
    ln, ld = math.log(num), math.log(den)
    if ld >= 0 or -ln >= niters * (-ld):
        return niters
    return int(np.rint(ln / ld))


def select(counts, N, confidence, max_iters):
    """The sequential rule over a count table [max_iters, 10] -> (best count, best k, best root, iterations consumed)."""
    best, niters, bk, br, k = 0, max_iters, -1, -1, 0
    while k < niters:
        for r in range(10):
            c = int(counts[k][r])
            if c > max(best, 4):
                best, bk, br = c, k, r
                niters = update_num_iters(confidence, (N - c) / N, niters)
        k += 1
    return best, bk, br, k
