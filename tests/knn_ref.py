"""float64 restatement of ratio-test 2-NN descriptor matching (csrc/knn_match.hip), per pair, with the margin inside
which a float32 evaluation of the same distances may legitimately decide otherwise.  Plain numpy; the float32 descriptors are taken as
given.  Written from the semantics of the operation (the two nearest columns by (L2 distance, column index), Lowe's ratio test in
Python floats), in the style of tests/match_ref.py, whose U = 2^-23 and bitwise row classes it reuses.

Distances.  For a row a of des1 and a row b of des2: p = |a|^2, q = |b|^2, G = a.b in float64 and t = max(p + q - 2 G, 0): the
radicand of the L2 distance.

The bound E on t -- derived, not tuned.  u = U = 2^-23 is TWICE the unit roundoff of float32 round-to-nearest: how the fp32 MFMA rounds
inside its two-term step has not been measured here, so u is an assumption with a factor-two allowance, not a measurement.  The kernel
evaluates t32 = fma(-2, dot32, n1 + n2) with n1, n2 the float32 sums of squares (one fmaf per component) and dot32 the MFMA dot.  For
ANY order of summation of D terms:
    |n1 - p| <= D u p,   |n2 - q| <= D u q                      (sums of non-negative terms)
    |dot32 - G| <= D u |a| |b| <= D u (p + q) / 2,  doubled by the factor 2: D u (p + q)
    the rounding of n1 + n2: <= u (p + q)
    the rounding of the fma: <= u |t| <= 2 u (p + q)            (t <= 2 (p + q))
(first order; the second-order terms are covered by the factor two in u).  The clamp at zero is 1-Lipschitz.  Hence
    |t32 - t64| <= E = (2 D + 3) u S,   S = max p + max q over the pair.
Exact pairs.  If every descriptor value is an integer and S + 2 max|G| < 2^24, every intermediate of the float32 evaluation is an
integer below 2^24 in any order, hence exact: E = 0 and t32 == t64 bitwise.

Order.  The columns of a row sorted by (t64, index): s1, s2, s3, ...  Two columns x before y are in CERTAIN order when t[y] - t[x] > 2 E
or when they are an exact tie that every tile evaluates alike -- bitwise-equal rows of des2 (their norms and dots are computed by the
same instructions on the same bits), or, on an exact pair, equal t64 -- which the lower index wins.  A row is ORDER-DECIDED when s1, s2
are in certain order and s2 is in certain order with every later column (for untied inputs this is the pairwise condition on the
three smallest keys); the expected (nn1, nn2) is then (s1, s2).  In any row nn1 must be a contender for first place
(t <= t[s1] + 2 E) and nn2 one for second place (t <= t[s2] + 2 E).

Distances are held on the radicand: |dist^2 - t64[i, nn]| <= E + (t64 + E) 2^-22 (one sqrtf rounding, factor-two allowance), as
match_ref.score_allowance.

Ratio.  Whatever the order decision, the float32 radicands of the reported neighbours lie within E of t[s1] and t[s2]: the k-th smallest
of values that are each within E of their float64 counterparts is within E of the k-th smallest of those.  This gives intervals
[lo, hi] on the float32 distances dist1, dist2 of every row: the roots of t[s_k] -+ (E + (t[s_k] + E) 2^-22); on an exact pair the
correctly rounded float32 root, exactly where it is representable (t a perfect square) and widened by one float32 step each way
otherwise.  The row is decided-pass if hi1 < ratio * lo2, decided-fail if lo1 >= ratio * hi2 (float64 products, as Python evaluates
`m.distance < ratio * n.distance`), decided-fail also when the row is order-decided, s1, s2 are bitwise-equal rows and ratio <= 1
(dist1 == dist2 bitwise, and d < ratio d is False for every d >= 0); otherwise undecided."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from match_ref import U, _classes, score_allowance  # noqa: F401  (re-exported)


def bound(D, S):
    """E = (2 D + 3) 2^-23 S on the radicand t."""
    return (2.0 * D + 3.0) * U * S


def _exact_root_interval(t):
    """[lo, hi] float64 arrays holding float32 values: the float32 root of the integer radicand t, exact where representable."""
    r = np.sqrt(t)
    r32 = r.astype(np.float32)
    exact = r32.astype(np.float64) ** 2 == t
    lo = np.where(exact, r32, np.nextafter(r32, np.float32(-np.inf))).astype(np.float64)
    hi = np.where(exact, r32, np.nextafter(r32, np.float32(np.inf))).astype(np.float64)
    return np.maximum(lo, 0.0), hi


class PairRef:
    """The restatement of one pair: t [N1,N2] float64, E, exact, and per row s1, s2 (expected), order_decided, the contenders C1, C2."""

    def __init__(self, d1, d2):
        d1, d2 = np.asarray(d1, np.float32), np.asarray(d2, np.float32)
        assert d1.ndim == 2 and d2.ndim == 2 and d1.shape[1] == d2.shape[1] and d1.shape[0] > 0 and d2.shape[0] >= 2
        self.N1, self.N2, self.D = d1.shape[0], d2.shape[0], d1.shape[1]
        a, b = d1.astype(np.float64), d2.astype(np.float64)
        # one float64 evaluation per distinct row of des2, shared by its bitwise copies: exact ties are ties here too
        self.cls = _classes(d2)
        rep = np.unique(self.cls, return_index=True)[1]
        p, q = (a * a).sum(1), (b * b).sum(1)[rep][self.cls]
        G = (a @ b[rep].T)[:, self.cls]
        self.S = float(p.max() + q.max())
        integer = bool((a == np.rint(a)).all() and (b == np.rint(b)).all())
        self.exact = integer and self.S + 2.0 * float(np.abs(G).max()) < 2.0 ** 24
        self.E = 0.0 if self.exact else bound(self.D, self.S)
        self.t = np.maximum(p[:, None] + q[None, :] - 2.0 * G, 0.0)
        E2 = 2.0 * self.E
        order = np.argsort(self.t, axis=1, kind="stable")  # by (t, index)
        rows = np.arange(self.N1)
        self.s1, self.s2 = order[:, 0], order[:, 1]
        self.t1, self.t2 = self.t[rows, self.s1], self.t[rows, self.s2]
        self.C1 = self.t <= (self.t1 + E2)[:, None]
        self.C2 = self.t <= (self.t2 + E2)[:, None]
        self.same12 = self.cls[self.s1] == self.cls[self.s2]
        if self.exact:  # every float32 radicand equals its float64 value: the order by (t64, index) is the order
            self.order_decided = np.ones(self.N1, dtype=bool)
        else:
            first = (self.t2 - self.t1 > E2) | self.same12
            later = np.ones((self.N1, self.N2), dtype=bool)
            later[rows, self.s1] = False
            later[rows, self.s2] = False
            unsure = later & self.C2 & (self.cls[None, :] != self.cls[self.s2][:, None])
            self.order_decided = first & ~unsure.any(axis=1)

    def allowance(self, t):
        return self.E + score_allowance(t, self.E)

    def _interval(self, t):
        if self.exact:
            return _exact_root_interval(t)
        lim = self.allowance(t)
        return np.sqrt(np.maximum(t - lim, 0.0)), np.sqrt(t + lim)

    def ratio_status(self, ratio):
        """Per row: +1 decided to pass `dist1 < ratio * dist2`, -1 decided to fail, 0 undecided."""
        ratio = float(ratio)
        lo1, hi1 = self._interval(self.t1)
        lo2, hi2 = self._interval(self.t2)
        st = np.zeros(self.N1, dtype=np.int64)
        st[hi1 < ratio * lo2] = 1
        st[lo1 >= ratio * hi2] = -1
        if ratio <= 1.0:
            st[self.same12 & self.order_decided] = -1
        return st

    def undecided_rows(self, ratio=None):
        """(rows undecided in order, rows undecided in ratio)."""
        uo = ~self.order_decided
        ur = np.zeros(self.N1, dtype=bool) if ratio is None else self.ratio_status(ratio) == 0
        return uo, ur

    def answer(self, ratio=0.8, ratio_test=True):
        """The float64 answer itself: nn1, nn2 int64 [N1], dist1, dist2 float32 [N1] = float32(sqrt(t)), good rows int64 [n]."""
        d1, d2 = np.sqrt(self.t1).astype(np.float32), np.sqrt(self.t2).astype(np.float32)
        good = d1.astype(np.float64) < float(ratio) * d2.astype(np.float64) if ratio_test else np.ones(self.N1, dtype=bool)
        return self.s1.copy(), self.s2.copy(), d1, d2, np.nonzero(good)[0]
