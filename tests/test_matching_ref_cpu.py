"""Pins the float64 restatement of descriptor matching (tests/match_ref.py) and the one check() of tests/matching_cases.py.  CPU only.

  * the restatement against the existing oracle (numpy float32, pinned by the reference's own run): on every case of matching_cases
    and on the descriptors of tests/golden/matching.npz, the decided rows agree with oracle.nn_match_two_way; where the two differ the
    row is undecided; the oracle's scores lie within the bound of the float64 radicand;
  * the inputs: every case stays under the 1 % cap of undecided rows and columns by the reference alone; tie and clip cases have none;
  * check() has teeth: the reference's own answer passes, and each planted error raises."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_ref as mr  # noqa: E402
import matching_cases as mc  # noqa: E402


def test_bound_is_the_derived_one():
    assert mr.bound(256) == 513 * 2.0 ** -23 and abs(mr.bound(256) - 6.1e-5) < 1e-6
    assert mr.bound(32) == 65 * 2.0 ** -23 and abs(mr.bound(32) - 7.7e-6) < 1e-7
    assert mr.bound(32, 2.25) == (64 * 2.25 + 1) * 2.0 ** -23


def _agree(oracle, ref, d1, d2, thr, where):
    m = oracle.nn_match_two_way(d1.T, d2.T, thr)
    oi, oj, os_ = m[0].astype(np.int64), m[1].astype(np.int64), m[2]
    st = ref.status(thr)
    emitted = np.full(ref.N1, -1, dtype=np.int64)
    emitted[oi] = oj
    must = st == 1
    assert (emitted[must] == ref.row_expect[must]).all(), (where, "decided matches the oracle lacks or places elsewhere",
                                                           np.nonzero(must & (emitted != ref.row_expect))[0][:8])
    assert (emitted[st == -1] == -1).all(), (where, "decided non-matches the oracle emits", np.nonzero((st == -1) & (emitted >= 0))[0][:8])
    # where the oracle and the float64 answer differ, the row (or its column, or the threshold on it) is undecided
    ri, rj, _ = ref.matches(thr)
    mine = np.full(ref.N1, -1, dtype=np.int64)
    mine[ri] = rj
    assert (st[mine != emitted] == 0).all(), where
    # what the oracle emits is a contender both ways, and its float32 score obeys the bound
    assert ref.J[oi, oj].all() and ref.I[oi, oj].all(), where
    t = ref.t[oi, oj]
    assert (np.abs(os_ ** 2 - t) <= ref.E + mr.score_allowance(t, ref.E)).all(), where
    return len(oi)


@pytest.mark.parametrize("name", mc.CASES)
def test_reference_agrees_with_the_oracle_and_inputs_are_decided(oracle, name):
    case = mc.get(name)
    mc.check_inputs(case, allow_undecided=not case.strict)
    for b, r in enumerate(case.refs):
        _agree(oracle, r, case.d1[b], case.d2[b], case.thr, f"{name} pair {b}")
    # the reference's own answer passes the check every device result goes through
    mc.check(case.d1, case.d2, case.thr, *mc.reference_answer(case), allow_undecided=not case.strict, tag=name, refs=case.refs)


def test_tie_and_clip_cases_have_nothing_undecided():
    assert len(mc.TIE_CASES) == 2 * len(mc.DELTAS) + 4
    for name in mc.TIE_CASES:
        case = mc.get(name)
        assert case.strict and mc.undecided_share(case)[0::2] == (0, 0), name


def test_case_construction():
    """What the descriptions of the cases promise."""
    for d in mc.DELTAS:  # every row whose two copies lie inside N expects the first, delta columns before the second
        r = mc.get(f"block_copy-{d}-rows").refs[0]
        tied = r.J.sum(1) == 2
        assert tied.sum() >= 44 and (np.nonzero(r.J[tied])[1].reshape(-1, 2) @ [-1, 1] == d).all()
        assert (r.J[tied].argmax(1) == r.row_expect[tied]).all() and r.row_decided.all()
        c = mc.get(f"block_copy-{d}-cols").refs[0]
        assert ((c.I.sum(0) == 2).sum() == tied.sum()) and c.col_decided.all()
    for D in (32, 64):
        m1, m2, _, cnt = mc.reference_answer(mc.get(f"all_equal-{D}"))
        assert cnt.tolist() == [1] and m1[0, 0] == 0 and m2[0, 0] == 0
    cl = mc.get("clipped").refs[0]
    assert (cl.J.sum(1) == 8).all() and (cl.I.sum(0) == 8).all() and (cl.rmin == 0).all() and cl.s > 2.2
    assert mc.reference_answer(mc.get("clipped"))[3].tolist() == [25]
    an = mc.get("antipodal-2.5").refs[0]
    assert an.t.min() > 3.3 and an.t.max() == 4.0
    for B in (4, 8, 3):
        cnt = mc.reference_answer(mc.get(f"remap-{B}"))[3].tolist()
        assert cnt[B // 2] == 0 and len(set(cnt)) == B and min(cnt[:B // 2] + cnt[B // 2 + 1:]) > 0, cnt
    for n in mc.LONG_N1:
        m1, _, _, cnt = mc.reference_answer(mc.get(f"long_rows-{n}"))
        for b in range(2):
            rows = set(m1[b, :cnt[b]].tolist())
            assert {0, 63, 64, n - 1} <= rows and (n <= 1024 or {1023, 1024} <= rows) and (n < 2049 or {2047, 2048} <= rows)
    m1, _, _, cnt = mc.reference_answer(mc.get("perm1100"))
    assert cnt.tolist() == [1100, 1100] and (m1 == np.arange(1100)).all()
    assert mc.reference_answer(mc.get("none1100"))[3].tolist() == [0, 0]


def test_reference_agrees_with_the_oracle_on_the_golden_descriptors(oracle, golden):
    g = golden("matching")
    for tag in ("crop", "pad"):
        d1, d2 = g[f"{tag}_des0"], g[f"{tag}_des1"]
        thr = float(g[f"{tag}_cfg"][2])
        n = 0
        for b in range(d1.shape[0]):
            n += _agree(oracle, mr.PairRef(d1[b], d2[b]), d1[b], d2[b], thr, f"golden {tag} pair {b}")
        assert n > 0


def test_pick_threshold_sits_clear_of_every_radicand():
    case = mc.get("edges-129x257")
    r = np.concatenate([x.rmin for x in case.refs])
    E = case.refs[0].E
    for nominal in (0.3, 0.9, 1.2, float(np.sqrt(np.float32(r[5])))):  # the last one sits ON a radicand
        thr = mr.pick_threshold(case.refs, nominal)
        assert thr == float(np.float32(thr)) and np.abs(r - thr ** 2).min() >= 2 * E and abs(thr - nominal) < 0.05
        assert all((x.undecided_rows(thr) == ~x.row_decided).all() for x in case.refs)


# ---- check() has teeth ----------------------------------------------------------------------------------------------------------
def _answer(name):
    case = mc.get(name)
    return case, [a.copy() for a in mc.reference_answer(case)]


def _check(case, m1, m2, sc, cnt):
    mc.check(case.d1, case.d2, case.thr, m1, m2, sc, cnt, allow_undecided=not case.strict, tag=case.name, refs=case.refs)


@pytest.mark.parametrize("delta", [1, 33, 128])
def test_check_raises_for_the_second_copy(delta):
    case, (m1, m2, sc, cnt) = _answer(f"block_copy-{delta}-rows")
    _check(case, m1, m2, sc, cnt)
    r = case.refs[0]
    k = next(k for k in range(cnt[0]) if r.J[m1[0, k]].sum() == 2)
    m2[0, k] += delta
    assert r.J[m1[0, k], m2[0, k]]  # the second copy IS a contender: only the first-occurrence rule rejects it
    with pytest.raises(AssertionError, match="not the first of an exact tie over the columns"):
        _check(case, m1, m2, sc, cnt)
    # and the second of two tied rows for one column
    case, (m1, m2, sc, cnt) = _answer(f"block_copy-{delta}-cols")
    r = case.refs[0]
    k = next(k for k in range(cnt[0]) if r.I[:, m2[0, k]].sum() == 2)
    m1[0, k] += delta
    order = np.argsort(m1[0, :cnt[0]], kind="stable")
    assert (np.diff(m1[0, :cnt[0]][order]) > 0).all()  # row j + delta is the second copy: not emitted by the reference
    m1[0, :cnt[0]], m2[0, :cnt[0]], sc[0, :cnt[0]] = m1[0, :cnt[0]][order], m2[0, :cnt[0]][order], sc[0, :cnt[0]][order]
    with pytest.raises(AssertionError, match="not the first of an exact tie over the rows"):  # sorted: the tie rule is what fails
        _check(case, m1, m2, sc, cnt)


def _drop(a, k, n):
    a[k:n - 1] = a[k + 1:n].copy()


def test_check_raises_for_a_dropped_match():
    case, (m1, m2, sc, cnt) = _answer("edges-129x257")
    _check(case, m1, m2, sc, cnt)
    st = case.refs[1].status(case.thr)
    k = next(k for k in range(cnt[1]) if st[m1[1, k]] == 1)
    for a in (m1[1], m2[1], sc[1]):
        _drop(a, k, cnt[1])
    cnt[1] -= 1
    with pytest.raises(AssertionError, match="decided mutual matches are missing"):
        _check(case, m1, m2, sc, cnt)


def test_check_raises_for_a_non_mutual_row():
    case, (m1, m2, sc, cnt) = _answer("block_copy-32-rows")
    r = case.refs[0]
    n = cnt[0]
    i = next(i for i in range(case.N1) if r.status(2.5)[i] == -1)  # decided, below any threshold, and not mutual: one of the unrelated rows
    j = r.row_expect[i]
    pos = int(np.searchsorted(m1[0, :n], i))
    for a, v in ((m1[0], i), (m2[0], j), (sc[0], np.float32(0.1))):
        a[pos + 1:n + 1] = a[pos:n].copy()
        a[pos] = v
    cnt[0] += 1
    with pytest.raises(AssertionError, match="not mutual"):
        _check(case, m1, m2, sc, cnt)


def test_check_raises_for_a_swap_and_for_a_wrong_count():
    case, (m1, m2, sc, cnt) = _answer("edges-129x257")
    for a in (m1[0], m2[0], sc[0]):
        a[[3, 4]] = a[[4, 3]]
    with pytest.raises(AssertionError, match="strictly increasing"):
        _check(case, m1, m2, sc, cnt)
    for d in (1, -1):
        case, (m1, m2, sc, cnt) = _answer("edges-129x257")
        cnt[1] += d
        with pytest.raises(AssertionError):
            _check(case, m1, m2, sc, cnt)
    case, (m1, m2, sc, cnt) = _answer("perm1100")
    cnt[0] += 1
    with pytest.raises(AssertionError, match="outside 0"):
        _check(case, m1, m2, sc, cnt)


@pytest.mark.parametrize("name", ["edges-129x257", "edges-129x257-256", "antipodal-2.5"])
def test_check_raises_for_a_score_off_by_3E(name):
    case, (m1, m2, sc, cnt) = _answer(name)
    r = case.refs[0]
    k = cnt[0] // 2
    t = r.t[m1[0, k], m2[0, k]]
    for sign in (1.0, -1.0):
        s = sc.copy()
        s[0, k] = np.float32(np.sqrt(max(t + sign * 3.0 * r.E, 0.0)))
        if sign < 0 and t < 3.0 * r.E:
            continue
        with pytest.raises(AssertionError, match="off the float64 radicand"):
            _check(case, m1, m2, s, cnt)
        s[0, k] = np.float32(np.sqrt(t + sign * 0.5 * r.E))  # half the bound passes
        _check(case, m1, m2, s, cnt)


def test_check_raises_for_a_score_at_the_threshold():
    case, (m1, m2, sc, cnt) = _answer("edges-129x257")
    sc[1, 2] = np.float32(case.thr)
    with pytest.raises(AssertionError, match="not below the threshold"):
        _check(case, m1, m2, sc, cnt)


def test_check_enforces_the_cap_and_the_strict_switch():
    case = mc.get("edges-65x129")  # one undecided column of 258 by the reference alone
    assert mc.undecided_share(case) == (0, 130, 1, 258)
    ans = mc.reference_answer(case)
    mc.check(case.d1, case.d2, case.thr, *ans, refs=case.refs)
    with pytest.raises(AssertionError, match="built to have none"):
        mc.check(case.d1, case.d2, case.thr, *ans, allow_undecided=False, refs=case.refs)
    # the same descriptors with two near-duplicates per row (differing in the last bit of one component): all rows undecided
    d2 = np.concatenate((case.d1, case.d1), axis=1).copy()
    d2[:, 65:, 0] = np.nextafter(d2[:, 65:, 0], np.float32(2.0))
    with pytest.raises(AssertionError, match="over the 1 % cap"):
        mc.check(case.d1, d2, 0.5, *[a[:, :65] if a.ndim == 2 else a for a in ans])
