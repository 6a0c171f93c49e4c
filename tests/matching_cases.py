"""Inputs of the descriptor-matching tests, shared by the host test (tests/test_matching_ref_cpu.py) and the GPU test
(tests/test_matching_edges_gpu.py), with the float64 restatement (tests/match_ref.py) of each computed once per process, and the one
check() every result goes through.

Every case is a Case: d1 [B,N1,D], d2 [B,N2,D] float32 numpy, thr (a float32 value placed by match_ref.pick_threshold so that the
reference alone decides every `score < thr`), strict (True: nothing of the case may be undecided).  D = 32 unless the name says
otherwise, so each case is one tiny launch.  Names (CASES lists them all):

  block_copy-<delta>-rows / -cols   d2 = consecutive blocks [X_k ; X_k] of delta fresh random unit descriptors and their bitwise copy,
                     cut at N = 300 (two full 128-tiles and one of 44); d1 = the distinct descriptors shuffled, plus 20 unrelated
                     ones.  "rows": (d1, d2), every row whose two copies lie inside N has an exact tie delta apart in its arg-min over
                     the columns and must take the first.  "cols": (d2, d1), rows j and j + delta both choose column c, the column's
                     arg-min over the rows is tied, (j, c) survives the mutual check and (j + delta, c) must be absent.
  all_equal-<D>      300 x 290 copies of one descriptor: exactly the match (0, 0), across 3 x 3 tiles.
  clipped            200 x 200, norm 1.5 on both sides: 25 orthonormal centres with 8 noisy members each per side, shuffled.  Every dot
                     inside a cluster is > 1.2 (clipped: t = 0 exactly, a tie of 8 non-identical columns), every other < 0.8.
  antipodal-2.5 (-2.0)  N = 65, d1 in a cone of half-angle ~0.4 rad about one direction, d2 = -d1[perm]: every dot is in [-1, -0.65],
                     every radicand in [3.3, 4] where float32 is coarsest, the dot with the own negative clips at -1.  (With d1 spread
                     over the whole sphere the nearest neighbours would sit at t ~ 1 and nothing would be near 4.)  thr = 2.5 keeps
                     every mutual pair; thr = 2.0 is kept only where pick_threshold finds a gap within 0.01 of it.
  edges-<N1>x<N2>[-D]  B = 2, the _rand_desc recipe of tests/test_matching.py, thr near 0.9: the full cross of the MFMA tile (32), the
                     wavefront (64) and the workgroup (128) edges on both sides.
  remap-<B>          129 x 257 (B = 4: 24 tiles, B = 3: 18) and 257 x 129 (B = 8: 48): every pair has its own descriptors and its own
                     share of true correspondences (the last row and the last column among them: the one-element corner tile), the
                     middle pair has none at all (all its scores are above thr).
  long_rows-<N1>     N2 = 130 noisy copies of rows of d1 that include 0, 63, 64, N1 - 1 and both sides of every multiple of 1024.
  perm1100           d2 = d1[perm] bitwise, 1100 x 1100, thr = 0.5: count = 1100 and m1 = arange, dense in every wavefront of both
                     passes of the compaction.
  none1100           1100 x 130 unrelated descriptors, thr below the smallest score: count = 0.
  rand-<N1>x<N2>-256 B = 2 at D = 256 (1100 x 1000, 1300 x 1300): the shapes whose undecided shares DESIGN.md 5 quotes."""
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_ref as mr  # noqa: E402
from test_matching import _rand_desc  # noqa: E402

DELTAS = (1, 2, 3, 4, 8, 16, 31, 32, 33, 64, 96, 127, 128, 129, 256)
EDGE_NS = (1, 33, 64, 65, 128, 129, 257)
LONG_N1 = (1023, 1024, 1025, 2049)
CAP = 0.01  # at most this share of a case's rows, and of its columns, may be undecided: a condition on the inputs


class Case:
    def __init__(self, name, d1, d2, nominal, strict=False, need=None):
        self.name = name
        self.d1 = np.ascontiguousarray(d1, dtype=np.float32)
        self.d2 = np.ascontiguousarray(d2, dtype=np.float32)
        self.d1.setflags(write=False)
        self.d2.setflags(write=False)
        self.B, self.N1, self.D = self.d1.shape
        self.N2 = self.d2.shape[1]
        self.strict = strict
        self.refs = tuple(mr.PairRef(self.d1[b], self.d2[b]) for b in range(self.B))
        self.thr = mr.pick_threshold(self.refs, nominal)
        if need is not None:
            assert abs(self.thr - nominal) <= need + 1e-6, (name, self.thr, nominal)


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def _block_copy(delta, way, N=300):
    g = np.random.default_rng(1000 + delta)
    blocks, first = [], []
    while sum(len(b) for b in blocks) < N:
        X = _unit(g.standard_normal((delta, 32))).astype(np.float32)
        blocks += [X, X.copy()]
        first += [np.ones(delta, bool), np.zeros(delta, bool)]
    d2 = np.concatenate(blocks)[:N]
    dist = d2[np.concatenate(first)[:N]]  # the distinct descriptors of d2 (a block cut by N may have lost its copies)
    d1 = np.concatenate((dist[g.permutation(len(dist))], _unit(g.standard_normal((20, 32))).astype(np.float32)))
    a, b = (d1, d2) if way == "rows" else (d2, d1)
    return Case(f"block_copy-{delta}-{way}", a[None], b[None], 0.5, strict=True, need=0.05)


def _all_equal(D, N1=300, N2=290):
    g = np.random.default_rng(7 + D)
    x = _unit(g.standard_normal(D)).astype(np.float32)
    return Case(f"all_equal-{D}", np.broadcast_to(x, (1, N1, D)), np.broadcast_to(x, (1, N2, D)), 0.5, strict=True, need=0.0)


def _clipped(N=200, K=25):
    g = np.random.default_rng(11)
    Q, _ = np.linalg.qr(g.standard_normal((32, K)))
    cen = Q.T  # [K,32] orthonormal
    side = lambda: (1.5 * _unit(np.repeat(cen, N // K, axis=0) + 0.3 * g.standard_normal((N, 32)) / 32 ** 0.5))[g.permutation(N)]
    d1, d2 = side().astype(np.float32), side().astype(np.float32)
    G = d1.astype(np.float64) @ d2.astype(np.float64).T
    assert ((G > 1.2) | (G < 0.8)).all() and (G > 1.2).sum() == N * N // K
    return Case("clipped", d1[None], d2[None], 0.5, strict=True, need=0.0)


def _antipodal(nominal, N=65):
    g = np.random.default_rng(13)
    c = _unit(g.standard_normal(32))
    d1 = _unit(c + 0.4 * _unit(g.standard_normal((N, 32))) * g.uniform(0.3, 1.0, (N, 1))).astype(np.float32)
    d2 = -d1[g.permutation(N)]
    G = d1.astype(np.float64) @ d2.astype(np.float64).T
    assert G.max() < -0.65
    return Case(f"antipodal-{nominal}", d1[None], d2[None], nominal, need=0.01)


def _edges(N1, N2, D=32):
    d1, d2 = _rand_desc(2, N1, N2, D, seed=1000 * N1 + N2 + D)
    return Case(f"edges-{N1}x{N2}" + ("" if D == 32 else f"-{D}"), d1.numpy(), d2.numpy(), 0.9, need=0.1)


def _remap(B):
    N1, N2 = (257, 129) if B == 8 else (129, 257)
    d1, d2 = [], []
    for b in range(B):
        common = 0.0 if b == B // 2 else 0.15 + 0.1 * b
        a, c = _rand_desc(1, N1, N2, 32, seed=700 + 10 * B + b, common=common)
        a, c = a[0].numpy(), c[0].numpy()
        if common:  # the last row and the last column correspond: the one-element corner tile of every pair carries a match
            c[N2 - 1] = _unit(a[N1 - 1] + 0.1 * np.random.default_rng(b).standard_normal(32) / 32 ** 0.5)
        d1.append(a)
        d2.append(c)
    case = Case(f"remap-{B}", np.stack(d1), np.stack(d2), 0.6, need=0.05)
    assert case.refs[B // 2].rmin.min() > case.thr ** 2 + 2 * case.refs[B // 2].E  # the middle pair has no match
    return case


def long_rows_sources(N1, N2, g):
    """The rows of d1 that d2 copies: both sides of every wavefront-0 / pass edge, then a random spread."""
    want = [0, 63, 64, N1 - 1]
    for m in range(1024, N1 + 1, 1024):
        want += [m - 65, m - 64, m - 2, m - 1, m, m + 1, m + 63, m + 64]
    want = list(dict.fromkeys(i for i in want if 0 <= i < N1))
    rest = np.setdiff1d(np.arange(N1), want)
    src = np.array(want + g.choice(rest, N2 - len(want), replace=False).tolist())
    return src[g.permutation(N2)]


def _long_rows(N1, N2=130):
    g = np.random.default_rng(N1)
    d1 = _unit(g.standard_normal((2, N1, 32))).astype(np.float32)
    d2 = np.stack([_unit(d1[b, long_rows_sources(N1, N2, g)] + 0.1 * g.standard_normal((N2, 32)) / 32 ** 0.5) for b in range(2)])
    return Case(f"long_rows-{N1}", d1, d2, 0.5, need=0.05)


def _perm1100(N=1100):
    g = np.random.default_rng(17)
    d1 = _unit(g.standard_normal((2, N, 32))).astype(np.float32)
    d2 = np.stack([d1[b, g.permutation(N)] for b in range(2)])
    return Case("perm1100", d1, d2, 0.5, strict=True, need=0.0)


def _none1100():
    g = np.random.default_rng(19)
    d1 = _unit(g.standard_normal((2, 1100, 32))).astype(np.float32)
    d2 = _unit(g.standard_normal((2, 130, 32))).astype(np.float32)
    case = Case("none1100", d1, d2, 0.3, need=0.0)
    assert min(r.rmin.min() for r in case.refs) > case.thr ** 2
    return case


def _rand256(N1, N2):
    d1, d2 = _rand_desc(2, N1, N2, 256, seed=N1 + N2)
    return Case(f"rand-{N1}x{N2}-256", d1.numpy(), d2.numpy(), 0.9, need=0.1)


_BUILDERS = {}
for _d in DELTAS:
    for _w in ("rows", "cols"):
        _BUILDERS[f"block_copy-{_d}-{_w}"] = functools.partial(_block_copy, _d, _w)
for _D in (32, 64):
    _BUILDERS[f"all_equal-{_D}"] = functools.partial(_all_equal, _D)
_BUILDERS["clipped"] = _clipped
_BUILDERS["antipodal-2.5"] = functools.partial(_antipodal, 2.5)
_BUILDERS["antipodal-2.0"] = functools.partial(_antipodal, 2.0)
for _a in EDGE_NS:
    for _b in EDGE_NS:
        _BUILDERS[f"edges-{_a}x{_b}"] = functools.partial(_edges, _a, _b)
for _D in (64, 256):
    for _a, _b in ((129, 257), (257, 129)):
        _BUILDERS[f"edges-{_a}x{_b}-{_D}"] = functools.partial(_edges, _a, _b, _D)
for _B in (4, 8, 3):
    _BUILDERS[f"remap-{_B}"] = functools.partial(_remap, _B)
for _n in LONG_N1:
    _BUILDERS[f"long_rows-{_n}"] = functools.partial(_long_rows, _n)
_BUILDERS["perm1100"] = _perm1100
_BUILDERS["none1100"] = _none1100
_BUILDERS["rand-1100x1000-256"] = functools.partial(_rand256, 1100, 1000)
_BUILDERS["rand-1300x1300-256"] = functools.partial(_rand256, 1300, 1300)


@functools.lru_cache(maxsize=None)
def get(name):
    """The case of that name with its restatement, built once per process and never modified.  antipodal-2.0 is None where
    pick_threshold finds no gap within 0.01 of 2.0 (the case is then dropped, as its description says)."""
    if name == "antipodal-2.0":
        try:
            return _BUILDERS[name]()
        except AssertionError:
            return None
    return _BUILDERS[name]()


CASES = [n for n in _BUILDERS if n != "antipodal-2.0" or get(n) is not None]
TIE_CASES = [n for n in CASES if n.startswith(("block_copy", "all_equal", "clipped", "perm1100"))]


def undecided_share(case, thr=None):
    """(undecided rows, rows, undecided columns, columns) of a case over its pairs, by the reference alone."""
    thr = case.thr if thr is None else thr
    ur = sum(int(r.undecided_rows(thr).sum()) for r in case.refs)
    uc = sum(int(r.undecided_cols().sum()) for r in case.refs)
    return ur, case.B * case.N1, uc, case.B * case.N2


def check_inputs(case, allow_undecided=True, thr=None):
    ur, nr, uc, nc = undecided_share(case, thr)
    if not allow_undecided:
        assert ur == 0 and uc == 0, f"{case.name}: {ur} rows and {uc} columns are undecided in a case built to have none"
    assert ur <= CAP * nr and uc <= CAP * nc, f"{case.name}: {ur}/{nr} rows, {uc}/{nc} columns undecided: over the 1 % cap"


# ---- the one check --------------------------------------------------------------------------------------------------------------
RECORD = {}  # D -> largest |score^2 - t64| seen / the bound it was held to; printed for the record, no bound is ever set from these


def _np(x):
    return np.asarray(x.detach().cpu() if hasattr(x, "detach") else x)


def check(d1, d2, thr, m1, m2, score, count, allow_undecided=True, tag="", refs=None):
    """Hold a result of nn_match_two_way (m1, m2 [B,>=count] integer, score [B,>=count] float32, count [B]) on d1 [B,N1,D],
    d2 [B,N2,D] at threshold thr to the float64 restatement, pair by pair:
      * 0 <= count <= N1 and m1[:count] strictly increasing;
      * every emitted (i, j, score): j in J_i and i in I_j, j / i the expected (lowest) index where the row / column is decided,
        score < thr as float32, |score^2 - t64[i,j]| within the bound;
      * every row that is decided and mutual by the reference is emitted, every row that is decided and not a match is absent;
      * undecided rows / columns are left out of the last item only, and at most 1 % of the rows and 1 % of the columns of the whole
        case may be undecided (none with allow_undecided=False): otherwise the case itself fails.
    refs: the PairRefs of (d1, d2) where the caller has them already.  Returns the largest |score^2 - t64| seen."""
    d1, d2 = _np(d1), _np(d2)
    m1, m2, score, count = _np(m1).astype(np.int64), _np(m2).astype(np.int64), _np(score), _np(count).astype(np.int64)
    assert score.dtype == np.float32
    B, N1, D = d1.shape
    N2 = d2.shape[1]
    refs = refs if refs is not None else [mr.PairRef(d1[b], d2[b]) for b in range(B)]
    thr32 = np.float32(thr)
    ur = sum(int(r.undecided_rows(thr).sum()) for r in refs)
    uc = sum(int(r.undecided_cols().sum()) for r in refs)
    if not allow_undecided:
        assert ur == 0 and uc == 0, f"{tag}: {ur} rows and {uc} columns are undecided in a case built to have none"
    assert ur <= CAP * B * N1 and uc <= CAP * B * N2, f"{tag}: {ur}/{B * N1} rows, {uc}/{B * N2} columns undecided: over the 1 % cap"
    worst, worst_ratio = 0.0, 0.0
    for b in range(B):
        r, n, w = refs[b], int(count[b]), f"{tag} pair {b}"
        assert 0 <= n <= N1, f"{w}: count {n} outside 0..{N1}"
        i, j, s = m1[b, :n], m2[b, :n], score[b, :n]
        assert (i[1:] > i[:-1]).all(), f"{w}: m1 is not strictly increasing"
        assert ((i >= 0) & (i < N1) & (j >= 0) & (j < N2)).all(), f"{w}: an index is out of range"
        bad = ~r.J[i, j]
        assert not bad.any(), f"{w}: column is no contender of its row: (i, j) = {list(zip(i[bad][:5], j[bad][:5]))}"
        bad = ~r.I[i, j]
        assert not bad.any(), f"{w}: row is no contender of its column (not mutual): (i, j) = {list(zip(i[bad][:5], j[bad][:5]))}"
        bad = r.row_decided[i] & (r.row_expect[i] != j)
        assert not bad.any(), f"{w}: not the first of an exact tie over the columns: (i, j, expected) = " \
                              f"{list(zip(i[bad][:5], j[bad][:5], r.row_expect[i][bad][:5]))}"
        bad = r.col_decided[j] & (r.col_expect[j] != i)
        assert not bad.any(), f"{w}: not the first of an exact tie over the rows: (i, j, expected) = " \
                              f"{list(zip(i[bad][:5], j[bad][:5], r.col_expect[j][bad][:5]))}"
        bad = ~(s < thr32)
        assert not bad.any(), f"{w}: score not below the threshold {thr32!r}: {s[bad][:5]} at rows {i[bad][:5]}"
        t = r.t[i, j]
        err = np.abs(s.astype(np.float64) ** 2 - t)
        lim = r.E + mr.score_allowance(t, r.E)
        if n:
            worst, worst_ratio = max(worst, float(err.max())), max(worst_ratio, float((err / lim).max()))
        bad = ~(err <= lim)
        assert not bad.any(), f"{w}: score^2 off the float64 radicand by {err[bad][:5]} (bound {lim[bad][:5]}) at rows {i[bad][:5]}"
        st = r.status(thr)
        emitted = np.zeros(N1, dtype=bool)
        emitted[i] = True
        bad = (st == 1) & ~emitted
        assert not bad.any(), f"{w}: decided mutual matches are missing: rows {np.nonzero(bad)[0][:8]}"
        bad = (st == -1) & emitted
        assert not bad.any(), f"{w}: rows that are decided not to match were emitted: {np.nonzero(bad)[0][:8]}"
    rec = RECORD.setdefault(D, [0.0, 0.0])
    rec[0], rec[1] = max(rec[0], worst), max(rec[1], worst_ratio)
    print(f"MATCH {tag}: D {D}  undecided rows {ur}/{B * N1} columns {uc}/{B * N2}  matches {count.tolist()}  "
          f"max |score^2 - t64| {worst:.3e} ({worst_ratio:.3f} of its bound; E = {refs[0].E:.3e})")
    return worst


def reference_answer(case, thr=None):
    """The reference's own matches of a case in the layout of ops.nn_match_two_way: m1, m2 [B,N1] int32 (0 beyond count),
    score [B,N1] float32, count [B] int32."""
    thr = case.thr if thr is None else thr
    m1 = np.zeros((case.B, case.N1), dtype=np.int32)
    m2 = np.zeros((case.B, case.N1), dtype=np.int32)
    sc = np.zeros((case.B, case.N1), dtype=np.float32)
    cnt = np.zeros(case.B, dtype=np.int32)
    for b, r in enumerate(case.refs):
        i, j, s = r.matches(thr)
        cnt[b] = len(i)
        m1[b, :len(i)], m2[b, :len(i)], sc[b, :len(i)] = i, j, s
    return m1, m2, sc, cnt


def run(dfepe, case, thr=None, device="cuda:0"):
    """The case through ops.nn_match_two_way and check(); returns the device result."""
    thr = case.thr if thr is None else thr
    out = dfepe.ops.nn_match_two_way(torch.tensor(case.d1, device=device), torch.tensor(case.d2, device=device), thr)
    check(case.d1, case.d2, thr, *out, allow_undecided=not case.strict, tag=case.name, refs=case.refs)
    return out
