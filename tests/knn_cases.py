"""Inputs of the ratio-test 2-NN matching tests, shared by the host test (tests/test_knn_ref_cpu.py) and the GPU test
(tests/test_knn_match_gpu.py), with the float64 restatement (tests/knn_ref.py) of each computed once per process, and the one check()
every result goes through.

Every case is a Case: d1 [B,N1,D], d2 [B,N2,D] float32 numpy, ratio (0.8), strict (True: no row of the case may be undecided, in order
or in ratio), exact (True: every pair is an exact pair of knn_ref, E = 0).  D = 32 unless the name says otherwise, so each case is one
tiny launch.  Names (CASES lists them all):

  edges-<N1>x<N2>[-D]  B = 2, the _rand_desc recipe of tests/test_matching.py: N1 over the MFMA tile (32), wavefront (64) and workgroup
                     (128) edges, N2 likewise and down to 2 and 3 (one or two real keys in a row's whole list).
  split-<delta>[-m]  N2 = 300 in blocks [X_k ; Y_k] of delta columns: X_k[m] = q + 0.1 n, Y_k[m] = q + 0.5 n' for a unit anchor q and
                     unit noises (t = 0.01 and 0.25, every other column near t = 2): query q has its best at c and its second at
                     c + delta.  "-m" is the mirrored order (second before best).  Columns of a block cut by N2 are unrelated.
  dup-<delta>, triple  the same layout with bitwise copies: d2[c] == d2[c + delta] (triple: three copies 50 apart), queries the
                     copied descriptor + 0.1 n.  nn1, nn2 are the two lowest indices, dist1 == dist2 bitwise, the ratio test rejects.
  all_equal-<D>      300 x 290 copies of one descriptor: (nn1, nn2) = (0, 1) in every row, nothing is good.
  sift-int-128-<N1>x<N2>  D = 128, integer SIFT-like values (non-negative, norm ~512, clipped at 255), B = 2; about half the rows of d1
                     have a noisy integer copy in d2.  Exact pairs: indices equal the reference everywhere.
  ratio-edge         D = 96, integers, exact.  Query 2 (k - 1) + e, k = 1 .. 32, is 1000 in a coordinate of its own (so every other
                     query's columns are ~1400 away); its two columns add a vector v1 with |v1|^2 = 16 k^2 (e = 0) or 16 k^2 - 1
                     (e = 1) and v2 with |v2|^2 = 25 k^2.  e = 0: 4 k < 0.8 * 5 k is False in float64 -> rejected; e = 1: accepted.
  long_rows-<N1>     N2 = 130 noisy copies of rows of d1 that include 0, 63, 64, N1 - 1 and both sides of every multiple of 1024
                     (matching_cases.long_rows_sources): good rows on both sides of every wavefront and pass edge of the compaction.
  wide-<N2>          N1 = 65, many slots per row; rows 0, 64: best in the first tile, second in the last; rows 1, 33: the reverse.
  remap-<B>          129 x 257 (B = 4: 24 tiles, B = 8: 48, B = 3: 18): both branches of the XCD tile remap; the middle pair has no
                     good row.
  rand-1100x1000-128 B = 2, unit-norm floats at D = 128."""
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_ref as kr  # noqa: E402
from matching_cases import CAP, DELTAS, LONG_N1, long_rows_sources  # noqa: E402
from test_matching import _rand_desc  # noqa: E402

EDGE_N1 = (1, 33, 64, 65, 128, 129, 257)
EDGE_N2 = (2, 3, 33, 64, 65, 128, 129, 257)
WIDE_N2 = (1100, 2049)
RATIO = 0.8


class Case:
    def __init__(self, name, d1, d2, ratio=RATIO, strict=False, exact=False):
        self.name = name
        self.d1 = np.ascontiguousarray(d1, dtype=np.float32)
        self.d2 = np.ascontiguousarray(d2, dtype=np.float32)
        self.d1.setflags(write=False)
        self.d2.setflags(write=False)
        self.B, self.N1, self.D = self.d1.shape
        self.N2 = self.d2.shape[1]
        self.ratio, self.strict, self.exact = ratio, strict, exact
        self.refs = tuple(kr.PairRef(self.d1[b], self.d2[b]) for b in range(self.B))
        assert all(r.exact for r in self.refs) == exact, (name, "exactness is not what the case claims")


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def _edges(N1, N2, D=32):
    """The cap is a condition on the inputs: the seed is the first of 1000 N1 + N2 + D + 7919 k, k = 0, 1, ..., whose descriptors meet
    it by the reference alone (at D = 256 the bound is wide enough for a draw of 258 rows to hold three undecided ones)."""
    for k in range(8):
        d1, d2 = _rand_desc(2, N1, N2, D, seed=1000 * N1 + N2 + D + 7919 * k)
        case = Case(f"edges-{N1}x{N2}" + ("" if D == 32 else f"-{D}"), d1.numpy(), d2.numpy())
        if sum(undecided_share(case)[:2]) <= CAP * case.B * case.N1:
            return case
    raise AssertionError(f"edges-{N1}x{N2}-{D}: no seed meets the cap")


def _firsts(delta, copies, N2):
    """Columns f that start a group f, f + delta, ... (copies members) lying wholly inside N2, in the block layout."""
    f = np.arange(N2)
    return f[((f // delta) % copies == 0) & (f + (copies - 1) * delta < N2)]


def _split(delta, mirrored, N2=300):
    g = np.random.default_rng(2000 + delta + (500 if mirrored else 0))
    d2 = _unit(g.standard_normal((N2, 32)))
    f = _firsts(delta, 2, N2)
    q = _unit(g.standard_normal((len(f), 32)))
    near, far = q + 0.1 * _unit(g.standard_normal(q.shape)), q + 0.5 * _unit(g.standard_normal(q.shape))
    d2[f], d2[f + delta] = (far, near) if mirrored else (near, far)
    perm = g.permutation(len(f))
    case = Case(f"split-{delta}" + ("-m" if mirrored else ""), q[perm][None], d2[None], strict=True)
    r = case.refs[0]
    best, second = (f + delta, f) if mirrored else (f, f + delta)
    assert (r.s1 == best[perm]).all() and (r.s2 == second[perm]).all()
    return case


def _dup(delta, copies=2, N2=300, name=None):
    g = np.random.default_rng(3000 + delta + copies)
    d2 = _unit(g.standard_normal((N2, 32))).astype(np.float32)
    f = _firsts(delta, copies, N2)
    for c in range(1, copies):
        d2[f + c * delta] = d2[f]
    perm = g.permutation(len(f))
    d1 = d2[f].astype(np.float64) + 0.1 * _unit(g.standard_normal((len(f), 32)))
    case = Case(name or f"dup-{delta}", d1[perm][None], d2[None], strict=True)
    r = case.refs[0]
    assert (r.s1 == f[perm]).all() and (r.s2 == f[perm] + delta).all() and r.same12.all() and (r.t1 == r.t2).all()
    return case


def _all_equal(D, N1=300, N2=290):
    g = np.random.default_rng(7 + D)
    x = (1.7 * _unit(g.standard_normal(D))).astype(np.float32)
    return Case(f"all_equal-{D}", np.broadcast_to(x, (1, N1, D)), np.broadcast_to(x, (1, N2, D)), strict=True)


def _sift_like(g, n, D=128):
    x = np.abs(g.standard_normal((n, D))) ** 1.5
    return np.minimum(np.rint(512.0 * x / np.linalg.norm(x, axis=1, keepdims=True)), 255.0)


def _sift_int(N1, N2, B=2):
    g = np.random.default_rng(N1 + N2)
    d1 = np.stack([_sift_like(g, N1) for _ in range(B)])
    d2 = np.stack([_sift_like(g, N2) for _ in range(B)])
    n = int(0.55 * min(N1, N2))
    for b in range(B):
        src, dst = g.permutation(N1)[:n], g.permutation(N2)[:n]
        sigma = g.uniform(3.0, 25.0, (n, 1))
        d2[b, dst] = np.clip(np.rint(d1[b, src] + sigma * g.standard_normal((n, 128))), 0.0, 255.0)
    case = Case(f"sift-int-128-{N1}x{N2}", d1, d2, strict=True, exact=True)
    for r in case.refs:  # about half the rows pass
        assert 0.35 * N1 < len(r.answer(RATIO)[4]) < 0.65 * N1
    return case


def _squares(n, parts=4):
    """n as a sum of `parts` squares (Lagrange), largest first."""
    if parts == 1:
        r = int(round(n ** 0.5))
        return [r] if r * r == n else None
    for a in range(int(n ** 0.5), -1, -1):
        rest = _squares(n - a * a, parts - 1)
        if rest is not None:
            return [a] + rest
    return None


def _ratio_edge(K=32, M=1000.0, D=96):
    g = np.random.default_rng(41)
    N1, N2 = 2 * K, 4 * K
    d1, d2 = np.zeros((N1, D)), np.zeros((N2, D))
    qpos, cpos = g.permutation(N1), g.permutation(N2)
    want = np.zeros((N1, 2), dtype=np.int64)
    for k in range(1, K + 1):
        for e in (0, 1):
            own = 2 * (k - 1) + e
            q, cb, cs = qpos[own], cpos[2 * own], cpos[2 * own + 1]
            d1[q, own] = d2[cb, own] = d2[cs, own] = M
            d2[cb, 64:68] = _squares(16 * k * k - e)
            d2[cs, 70] = 5 * k
            want[q] = (cb, cs)
            assert (d2[cb, 64:68] ** 2).sum() == 16 * k * k - e
    case = Case("ratio-edge", d1[None], d2[None], strict=True, exact=True)
    r = case.refs[0]
    st = r.ratio_status(RATIO)
    assert (r.s1 == want[:, 0]).all() and (r.s2 == want[:, 1]).all()
    for k in range(1, K + 1):
        q0, q1 = qpos[2 * (k - 1)], qpos[2 * (k - 1) + 1]
        assert r.t1[q0] == 16 * k * k and r.t2[q0] == 25 * k * k and r.t1[q1] == 16 * k * k - 1
        assert not (4.0 * k < RATIO * (5.0 * k))  # the float64 product does not fall below 4 k
        assert st[q0] == -1 and st[q1] == 1, (k, st[q0], st[q1])  # both decided by the interval rule
    return case


def _long_rows(N1, N2=130):
    g = np.random.default_rng(N1)
    d1 = _unit(g.standard_normal((2, N1, 32))).astype(np.float32)
    srcs = [long_rows_sources(N1, N2, g) for _ in range(2)]
    d2 = np.stack([_unit(d1[b, srcs[b]] + 0.1 * g.standard_normal((N2, 32)) / 32 ** 0.5) for b in range(2)])
    case = Case(f"long_rows-{N1}", d1, d2)
    for b, r in enumerate(case.refs):  # the copied rows are decided to pass: good rows on both sides of every edge
        must = {0, 63, 64, N1 - 1} | {m + o for m in range(1024, N1 + 1, 1024) for o in (-65, -64, -2, -1, 0, 1, 63, 64) if m + o < N1}
        assert must <= set(srcs[b].tolist()) and (r.ratio_status(RATIO)[srcs[b]] == 1).all()
    return case


WIDE_PLANTS = lambda N2: ((0, 5, N2 - 3), (1, N2 - 2, 7), (64, 100, N2 - 1), (33, N2 - 60, 64))  # (row, best, second)


def _wide(N2, N1=65):
    d1, d2 = (x.numpy().astype(np.float64) for x in _rand_desc(2, N1, N2, 32, seed=5000 + N2))
    g = np.random.default_rng(N2)
    for b in range(2):
        for row, cb, cs in WIDE_PLANTS(N2):
            d2[b, cb] = d1[b, row] + 0.01 * _unit(g.standard_normal(32))
            d2[b, cs] = d1[b, row] + 0.025 * _unit(g.standard_normal(32))
    case = Case(f"wide-{N2}", d1, d2)
    for r in case.refs:
        for row, cb, cs in WIDE_PLANTS(N2):
            assert r.order_decided[row] and (r.s1[row], r.s2[row]) == (cb, cs)
    return case


def _remap(B, N1=129, N2=257):
    d1, d2 = [], []
    for b in range(B):
        for k in range(16):  # the middle pair: the first seed whose unrelated descriptors leave every row decided to fail
            a, c = _rand_desc(1, N1, N2, 32, seed=900 + 10 * B + b + 7919 * k, common=0.0 if b == B // 2 else 0.15 + 0.1 * b)
            a, c = a[0].numpy(), c[0].numpy()
            if b != B // 2 or (kr.PairRef(a, c).ratio_status(RATIO) == -1).all():
                break
        d1.append(a)
        d2.append(c)
    case = Case(f"remap-{B}", np.stack(d1), np.stack(d2))
    assert (case.refs[B // 2].ratio_status(RATIO) == -1).all()  # the middle pair: every row is decided to fail
    assert all(len(r.answer(RATIO)[4]) > 0 for b, r in enumerate(case.refs) if b != B // 2)
    return case


def _rand128(N1=1100, N2=1000):
    d1, d2 = _rand_desc(2, N1, N2, 128, seed=N1 + N2 + 128)
    return Case(f"rand-{N1}x{N2}-128", d1.numpy(), d2.numpy())


_BUILDERS = {}
for _a in EDGE_N1:
    for _b in EDGE_N2:
        _BUILDERS[f"edges-{_a}x{_b}"] = functools.partial(_edges, _a, _b)
for _D in (64, 128, 256):
    for _a, _b in ((129, 257), (257, 129)):
        _BUILDERS[f"edges-{_a}x{_b}-{_D}"] = functools.partial(_edges, _a, _b, _D)
for _d in DELTAS:
    _BUILDERS[f"split-{_d}"] = functools.partial(_split, _d, False)
    _BUILDERS[f"split-{_d}-m"] = functools.partial(_split, _d, True)
for _d in DELTAS:
    _BUILDERS[f"dup-{_d}"] = functools.partial(_dup, _d)
_BUILDERS["triple"] = functools.partial(_dup, 50, 3, name="triple")
for _D in (32, 64):
    _BUILDERS[f"all_equal-{_D}"] = functools.partial(_all_equal, _D)
_BUILDERS["sift-int-128-300x290"] = functools.partial(_sift_int, 300, 290)
_BUILDERS["sift-int-128-1100x1000"] = functools.partial(_sift_int, 1100, 1000)
_BUILDERS["ratio-edge"] = _ratio_edge
for _n in LONG_N1:
    _BUILDERS[f"long_rows-{_n}"] = functools.partial(_long_rows, _n)
for _n in WIDE_N2:
    _BUILDERS[f"wide-{_n}"] = functools.partial(_wide, _n)
for _B in (3, 4, 8):
    _BUILDERS[f"remap-{_B}"] = functools.partial(_remap, _B)
_BUILDERS["rand-1100x1000-128"] = _rand128

CASES = list(_BUILDERS)
TIE_CASES = [n for n in CASES if n.startswith(("dup-", "triple", "all_equal"))]


@functools.lru_cache(maxsize=None)
def get(name):
    """The case of that name with its restatement, built once per process and never modified."""
    return _BUILDERS[name]()


def undecided_share(case, ratio=None):
    """(rows undecided in order, rows undecided in ratio, rows) of a case over its pairs, by the reference alone."""
    ratio = case.ratio if ratio is None else ratio
    uo = ur = 0
    for r in case.refs:
        a, b = r.undecided_rows(ratio)
        uo, ur = uo + int(a.sum()), ur + int(b.sum())
    return uo, ur, case.B * case.N1


def _cap(uo, ur, n, allow_undecided, tag):
    if not allow_undecided:
        assert uo == 0 and ur == 0, f"{tag}: {uo} rows undecided in order and {ur} in ratio in a case built to have none"
    assert uo + ur <= CAP * n, f"{tag}: {uo} rows undecided in order and {ur} in ratio of {n}: over the 1 % cap"


def check_inputs(case, ratio=None):
    _cap(*undecided_share(case, ratio), not case.strict, case.name)


# ---- the one check --------------------------------------------------------------------------------------------------------------
RECORD = {}  # D -> largest |dist^2 - t64| seen / the bound it was held to; printed for the record, no bound is ever set from these


def _np(x):
    return np.asarray(x.detach().cpu() if hasattr(x, "detach") else x)


def check(d1, d2, ratio, ratio_test, out, allow_undecided=True, tag="", refs=None):
    """Hold a result of knn_match, out = (nn1, nn2, dist1, dist2, m_idx1, m_idx2, score, count) on d1 [B,N1,D], d2 [B,N2,D], to the
    float64 restatement, pair by pair:
      * nn1 != nn2 in range; nn1 a contender for first place and nn2 for second place in every row; (nn1, nn2) the expected pair
        (the lowest indices on exact ties) in every order-decided row;
      * dist1 <= dist2, both within the bound of the float64 radicand of the reported column, bitwise equal where the two columns
        are bitwise-equal descriptors;
      * 0 <= count <= N1, m_idx1[:count] strictly increasing, m_idx2 / score the row's nn1 / dist1 (bitwise), and the list is
        exactly the rows with float64(dist1) < ratio * float64(dist2) on the reported distances (every row with ratio_test False);
      * with ratio_test: every decided-pass row is in the list, every decided-fail row absent;
      * at most 1 % of the rows of the whole case may be undecided (none with allow_undecided=False): otherwise the case fails.
    Returns the largest |dist^2 - t64| seen."""
    d1, d2 = _np(d1), _np(d2)
    nn1, nn2, dist1, dist2, m1, m2, score, count = (_np(x) for x in out)
    assert dist1.dtype == np.float32 and dist2.dtype == np.float32 and score.dtype == np.float32
    nn1, nn2, m1, m2, count = (x.astype(np.int64) for x in (nn1, nn2, m1, m2, count))
    B, N1, D = d1.shape
    N2 = d2.shape[1]
    refs = refs if refs is not None else [kr.PairRef(d1[b], d2[b]) for b in range(B)]
    uo = sum(int((~r.order_decided).sum()) for r in refs)
    ur = sum(int(r.undecided_rows(ratio)[1].sum()) for r in refs) if ratio_test else 0
    _cap(uo, ur, B * N1, allow_undecided, tag)
    worst, worst_ratio = 0.0, 0.0
    rows = np.arange(N1)
    for b in range(B):
        r, n, w = refs[b], int(count[b]), f"{tag} pair {b}"
        a1, a2, e1, e2 = nn1[b, :N1], nn2[b, :N1], dist1[b, :N1], dist2[b, :N1]
        assert ((a1 >= 0) & (a1 < N2) & (a2 >= 0) & (a2 < N2)).all(), f"{w}: a neighbour index is out of range"
        assert (a1 != a2).all(), f"{w}: nn1 == nn2 at rows {np.nonzero(a1 == a2)[0][:8]}"
        bad = ~r.C1[rows, a1]
        assert not bad.any(), f"{w}: nn1 is no contender for first place: (i, nn1) = {list(zip(rows[bad][:5], a1[bad][:5]))}"
        bad = ~r.C2[rows, a2]
        assert not bad.any(), f"{w}: nn2 is no contender for second place: (i, nn2) = {list(zip(rows[bad][:5], a2[bad][:5]))}"
        bad = r.order_decided & ((a1 != r.s1) | (a2 != r.s2))
        assert not bad.any(), f"{w}: not the expected (nn1, nn2) of an order-decided row (lowest indices on exact ties): " \
                              f"(i, got, expected) = {list(zip(rows[bad][:5], zip(a1[bad][:5], a2[bad][:5]), zip(r.s1[bad][:5], r.s2[bad][:5])))}"
        assert (e1 <= e2).all(), f"{w}: dist1 > dist2 at rows {np.nonzero(~(e1 <= e2))[0][:8]}"
        for which, col, e in (("dist1", a1, e1), ("dist2", a2, e2)):
            t = r.t[rows, col]
            err = np.abs(e.astype(np.float64) ** 2 - t)
            lim = r.allowance(t)
            worst = max(worst, float(err.max()))
            share = np.where(lim > 0, err / np.where(lim > 0, lim, 1.0), np.where(err > 0, np.inf, 0.0))
            worst_ratio = max(worst_ratio, float(share.max()))
            bad = ~(err <= lim)
            assert not bad.any(), f"{w}: {which}^2 off the float64 radicand by {err[bad][:5]} (bound {lim[bad][:5]}) at rows {rows[bad][:5]}"
        tied = r.cls[a1] == r.cls[a2]
        assert (e1[tied].view(np.uint32) == e2[tied].view(np.uint32)).all(), f"{w}: bitwise-equal descriptors at different distances"
        assert 0 <= n <= N1, f"{w}: count {n} outside 0..{N1}"
        i, j, s = m1[b, :n], m2[b, :n], score[b, :n]
        assert (i[1:] > i[:-1]).all(), f"{w}: the good list is not strictly increasing"
        assert ((i >= 0) & (i < N1)).all(), f"{w}: a good row is out of range"
        assert (j == a1[i]).all() and (s.view(np.uint32) == e1[i].view(np.uint32)).all(), f"{w}: the good list does not carry its rows' nn1 / dist1"
        emitted = np.zeros(N1, dtype=bool)
        emitted[i] = True
        own = (e1.astype(np.float64) < float(ratio) * e2.astype(np.float64)) if ratio_test else np.ones(N1, dtype=bool)
        bad = emitted != own
        assert not bad.any(), f"{w}: the good list is not the rows with float64(dist1) < ratio * float64(dist2): rows {np.nonzero(bad)[0][:8]}"
        if ratio_test:
            st = r.ratio_status(ratio)
            bad = (st == 1) & ~emitted
            assert not bad.any(), f"{w}: rows decided to pass the ratio test are missing: {np.nonzero(bad)[0][:8]}"
            bad = (st == -1) & emitted
            assert not bad.any(), f"{w}: rows decided to fail the ratio test were emitted: {np.nonzero(bad)[0][:8]}"
    rec = RECORD.setdefault(D, [0.0, 0.0])
    rec[0], rec[1] = max(rec[0], worst), max(rec[1], worst_ratio)
    print(f"KNN {tag}: D {D}  undecided rows: order {uo} ratio {ur} of {B * N1}  good {count.tolist()}  "
          f"max |dist^2 - t64| {worst:.3e} ({worst_ratio:.3f} of its bound; E = {refs[0].E:.3e})")
    return worst


def reference_answer(case, ratio=None, ratio_test=True):
    """The reference's own answer of a case in the layout of ops.knn_match (0 beyond count)."""
    ratio = case.ratio if ratio is None else ratio
    B, N1 = case.B, case.N1
    nn1, nn2, m1, m2 = (np.zeros((B, N1), dtype=np.int32) for _ in range(4))
    e1, e2, sc = (np.zeros((B, N1), dtype=np.float32) for _ in range(3))
    cnt = np.zeros(B, dtype=np.int32)
    for b, r in enumerate(case.refs):
        nn1[b], nn2[b], e1[b], e2[b], good = r.answer(ratio, ratio_test)
        n = cnt[b] = len(good)
        m1[b, :n], m2[b, :n], sc[b, :n] = good, nn1[b, good], e1[b, good]
    return nn1, nn2, e1, e2, m1, m2, sc, cnt


def run(dfepe, case, ratio=None, ratio_test=True, device="cuda:0"):
    """The case through ops.knn_match and check(); returns the device result."""
    ratio = case.ratio if ratio is None else ratio
    out = dfepe.ops.knn_match(torch.tensor(case.d1, device=device), torch.tensor(case.d2, device=device), ratio, ratio_test)
    check(case.d1, case.d2, ratio, ratio_test, out, allow_undecided=not case.strict, tag=case.name, refs=case.refs)
    return out
