"""float64 restatement of two-way nearest-neighbour descriptor matching (csrc/match.hip), per pair, with the margin
inside which a float32 evaluation of the same distances may legitimately decide otherwise.  Plain numpy; the float32 descriptors are
taken as given.

Distances.  G = d1 d2^T in float64 and t = 2 - 2 clip(G, -1, 1): the radicand of the published distance sqrt(2 - 2 clip(dot)).

The bound E(D) on t -- derived, not tuned.  Let u = 2^-23.  That is TWICE the unit roundoff of float32 round-to-nearest (2^-24): how
the fp32 MFMA rounds inside its two-term step has not been measured here, so u is an assumption with a factor-two allowance, not a
measurement.  For unit-norm a and b and ANY order of summation, the float32 dot product of D terms obeys the classical bound
    |dot32 - dot64| <= gamma_D sum_k |a_k b_k| <= D u |a| |b| = D u
(gamma_D = D u / (1 - D u) to first order; the second-order term is covered by the factor two in u; Cauchy-Schwarz for the sum).  The
clip is 1-Lipschitz, the factor 2 is exact, and t = fma(-2, clip, 2) is ONE IEEE rounding of a value of at most 4, i.e. at most
2^-23 = u absolute.  Hence
    |t32 - t64| <= E(D) = (2 D + 1) u:      6.1e-5 at D = 256, 7.7e-6 at D = 32.
For inputs that are not unit-norm the dot part scales with s = max|a| max|b| (the clip keeps t <= 4, so the last rounding does not):
E = (2 D s + 1) u, with s never taken below 1.

Contenders and decided rows.  For row i, J_i = {j : t[i,j] <= min_j t[i,j] + 2 E}: every column a float32 evaluation within E may rank
first.  Row i is DECIDED when all members of J_i are certain to give bit-identical float32 radicands on any evaluation that treats
every column alike, which is the case when
  * their descriptors are bitwise equal (raw fp32 bytes of the rows compared), or
  * all of them are surely clipped: G >= 1 + D u s, so that t is exactly 0 in float32 as in float64.
The expected answer is then the LOWEST index of J_i: numpy's first-occurrence arg-min, the kernel's documented contract for exact
ties.  Any other row is undecided: the float64 order inside J_i says nothing about a correct float32 evaluation.  Columns likewise
(I_j over the rows).

Score.  Compared on the radicand: |score^2 - t64[i,j]| <= E + (t64 + E) 2^-22.  The second term is the one float32 sqrtf rounding
(score^2 = t32 (1 + d)^2, |d| <= 2^-24) with the same factor-two allowance.  A bound on the root itself is meaningless near t = 0
(sqrt(E) ~ 8e-3).

Threshold.  pick_threshold places thr so that thr^2 is at least 2 E away from every nearest-neighbour radicand of the float64 reference
(in the middle of a gap of at least 4 E).  A float32 radicand within E of its float64 value is then at least E away from thr^2, which
dwarfs the roundings of float32(sqrt(.)) on either side (<= 4 * 2^-23 each), so `score < thr` is decided by the reference alone."""
import numpy as np

U = 2.0 ** -23


def scale_of(d1, d2):
    """s = max|a| max|b| over the descriptors of a pair, never below 1."""
    n1 = np.sqrt((d1.astype(np.float64) ** 2).sum(-1)).max() if d1.size else 1.0
    n2 = np.sqrt((d2.astype(np.float64) ** 2).sum(-1)).max() if d2.size else 1.0
    return max(1.0, float(n1 * n2))


def bound(D, s=1.0):
    """E(D) = (2 D s + 1) 2^-23 on the radicand t."""
    return (2.0 * D * s + 1.0) * U


def score_allowance(t, E):
    """The one sqrtf rounding of the score, seen on score^2."""
    return (t + E) * 2.0 ** -22


def _classes(d):
    """One integer per row of d [N,D] float32: equal integers <=> bitwise-equal rows."""
    raw = np.ascontiguousarray(d, dtype=np.float32).view(np.uint32).reshape(d.shape[0], -1)
    _, inv = np.unique(raw, axis=0, return_inverse=True)
    return inv.reshape(-1).astype(np.int64)


def _side(t, G, cls, E, clip_margin):
    """Rows of t [N,M] against the M candidates: (min [N], contenders [N,M] bool, decided [N] bool, expected [N] lowest contender)."""
    tmin = t.min(axis=1)
    J = t <= tmin[:, None] + 2.0 * E
    big = np.iinfo(np.int64).max
    same = np.where(J, cls[None, :], big).min(axis=1) == np.where(J, cls[None, :], -1).max(axis=1)
    clipped = np.where(J, G, np.inf).min(axis=1) >= 1.0 + clip_margin
    return tmin, J, same | clipped, J.argmax(axis=1)


class PairRef:
    """The restatement of one pair: t [N1,N2] float64, E, and per row / column the minimum, the contenders, decided, expected."""

    def __init__(self, d1, d2):
        d1, d2 = np.asarray(d1, np.float32), np.asarray(d2, np.float32)
        assert d1.ndim == 2 and d2.ndim == 2 and d1.shape[1] == d2.shape[1] and d1.shape[0] > 0 and d2.shape[0] > 0
        self.N1, self.N2, self.D = d1.shape[0], d2.shape[0], d1.shape[1]
        self.s = scale_of(d1, d2)
        self.E = bound(self.D, self.s)
        G = d1.astype(np.float64) @ d2.astype(np.float64).T
        self.t = 2.0 - 2.0 * np.clip(G, -1.0, 1.0)
        margin = self.D * U * self.s
        self.rmin, self.J, self.row_decided, self.row_expect = _side(self.t, G, _classes(d2), self.E, margin)
        self.cmin, It, self.col_decided, self.col_expect = _side(self.t.T, G.T, _classes(d1), self.E, margin)
        self.I = It.T  # [N1,N2]: I[i,j] <=> row i contends for column j

    def status(self, thr):
        """Per row, against the float32 threshold `thr` (compared as score < thr): +1 decided and a mutual match, -1 decided and not
        a match, 0 undecided (the row, the threshold on it, or -- where everything else says match -- its column)."""
        thr2 = float(np.float32(thr)) ** 2
        below = self.rmin <= thr2 - 2.0 * self.E
        above = self.rmin >= thr2 + 2.0 * self.E
        j = self.row_expect
        st = np.zeros(self.N1, dtype=np.int64)
        rd = self.row_decided
        st[rd & above] = -1
        cd = self.col_decided[j]
        mutual = self.col_expect[j] == np.arange(self.N1)
        st[rd & cd & ~mutual] = -1
        st[rd & cd & mutual & below] = 1
        return st

    def undecided_rows(self, thr=None):
        """Rows left out of the completeness assertions: contenders not exactly tied, or (with thr) the threshold not clear of them."""
        und = ~self.row_decided
        if thr is not None:
            thr2 = float(np.float32(thr)) ** 2
            und = und | (np.abs(self.rmin - thr2) < 2.0 * self.E)
        return und

    def undecided_cols(self):
        return ~self.col_decided

    def matches(self, thr):
        """The float64 answer itself (first occurrence inside the contenders): m1, m2 int64, score float32 = float32(sqrt(t))."""
        i = np.arange(self.N1)
        j = self.row_expect
        keep = (np.sqrt(self.rmin).astype(np.float32) < np.float32(thr)) & (self.col_expect[j] == i)
        return i[keep], j[keep], np.sqrt(self.t[i[keep], j[keep]]).astype(np.float32)


def pick_threshold(refs, nominal):
    """A float32 threshold near `nominal` whose square is at least 2 E from every nearest-neighbour radicand (row minimum) of the given
    PairRef(s).  Candidates: nominal itself where it already lies that clear of every radicand, the middle of every gap between
    consecutive sorted radicands (and between 0 and the smallest), and 4 E above the largest; gaps count from 5 E, which leaves room
    for the rounding of the threshold to float32.  The candidate nearest nominal (on the radicand) wins."""
    refs = list(refs) if isinstance(refs, (list, tuple)) else [refs]
    E = max(r.E for r in refs)
    r = np.sort(np.concatenate([x.rmin for x in refs]))
    n2 = float(np.float32(nominal)) ** 2
    cands = [r[-1] + 4.0 * E]
    if np.abs(r - n2).min() >= 2.5 * E:
        cands.append(n2)
    edges = np.concatenate(([0.0], r))
    cands += [0.5 * (edges[k] + edges[k + 1]) for k in np.nonzero(np.diff(edges) >= 5.0 * E)[0]]
    thr = np.float32(np.sqrt(min(cands, key=lambda c: abs(c - n2))))
    assert np.abs(r - float(thr) ** 2).min() >= 2.0 * E, (nominal, float(thr))
    return float(thr)
