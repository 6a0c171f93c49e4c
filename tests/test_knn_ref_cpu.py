"""Pins the float64 restatement of ratio-test 2-NN matching (tests/knn_ref.py) and the one check() of tests/knn_cases.py.  CPU only.

  * the restatement against a naive per-query loop that spells the operation line by line: distances from the differences, a stable
    sort by distance, the first two, the ratio line in Python floats;
  * the inputs: every case stays under the 1 % cap of undecided rows by the reference alone (the shares are printed); strict cases
    have none;
  * check() has teeth: the reference's own answer passes, and each planted error raises."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_cases as kc  # noqa: E402
import knn_ref as kr  # noqa: E402


def test_bound_is_the_derived_one():
    assert kr.bound(128, 2.0) == 259 * 2.0 ** -23 * 2.0 and kr.bound(32, 1.0) == 67 * 2.0 ** -23
    r = kc.get("edges-129x257").refs[0]
    assert r.E == kr.bound(32, r.S) and 1.99 < r.S < 2.01 and not r.exact
    assert kc.get("sift-int-128-300x290").refs[0].E == 0.0


def _naive(d1, d2, ratio, if_ratio_test=True):
    a, b = d1.astype(np.float64), d2.astype(np.float64)
    all_m, good = [], []
    for i in range(a.shape[0]):
        dist = np.sqrt(((a[i] - b) ** 2).sum(axis=1))
        order = np.argsort(dist, kind="stable")
        m, n = int(order[0]), int(order[1])
        m_distance, n_distance = float(np.float32(dist[m])), float(np.float32(dist[n]))
        all_m.append((i, m, n))
        if if_ratio_test:
            if m_distance < ratio * n_distance:
                good.append(i)
    if not if_ratio_test:
        good = [i for i, _, _ in all_m]
    return np.array(all_m, dtype=np.int64).reshape(-1, 3), np.array(good, dtype=np.int64)


@pytest.mark.parametrize("name", kc.CASES)
def test_reference_agrees_with_the_naive_loop_and_inputs_are_decided(name):
    case = kc.get(name)
    uo, ur, n = kc.undecided_share(case)
    print(f"KNN INPUT {name}: undecided in order {uo}, in ratio {ur}, of {n} rows ({100.0 * (uo + ur) / n:.2f} %)")
    kc.check_inputs(case)
    for b, r in enumerate(case.refs):
        all_m, good = _naive(case.d1[b], case.d2[b], case.ratio)
        dec = r.order_decided
        assert (all_m[dec, 1] == r.s1[dec]).all() and (all_m[dec, 2] == r.s2[dec]).all(), (name, b)
        st = r.ratio_status(case.ratio)
        passed = np.zeros(case.N1, dtype=bool)
        passed[good] = True
        assert passed[st == 1].all() and not passed[st == -1].any(), (name, b)
        if r.exact:  # nothing is left to rounding: the two are the same answer
            s1, s2, _, _, mine = r.answer(case.ratio)
            assert (all_m[:, 1] == s1).all() and (all_m[:, 2] == s2).all() and (good == mine).all(), (name, b)
    # the reference's own answer passes the check every device result goes through, with and without the ratio test
    for rt in (True, False):
        kc.check(case.d1, case.d2, case.ratio, rt, kc.reference_answer(case, ratio_test=rt), allow_undecided=not case.strict,
                 tag=name, refs=case.refs)


def test_case_construction():
    """What the descriptions of the cases promise beyond what their builders assert."""
    assert len(kc.CASES) == 7 * 8 + 6 + 2 * len(kc.DELTAS) + len(kc.DELTAS) + 1 + 2 + 2 + 1 + 4 + 2 + 3 + 1
    for name in kc.TIE_CASES:
        case = kc.get(name)
        assert case.strict and kc.undecided_share(case)[:2] == (0, 0)
        assert kc.reference_answer(case)[7].tolist() == [0]                          # the ratio test rejects every tie
        assert kc.reference_answer(case, ratio_test=False)[7].tolist() == [case.N1]  # and they are present without it
    for D in (32, 64):
        nn1, nn2 = kc.reference_answer(kc.get(f"all_equal-{D}"))[:2]
        assert (nn1 == 0).all() and (nn2 == 1).all()
    for B in (3, 4, 8):
        cnt = kc.reference_answer(kc.get(f"remap-{B}"))[7].tolist()
        assert cnt[B // 2] == 0 and min(cnt[:B // 2] + cnt[B // 2 + 1:]) > 0, cnt
    for n in kc.LONG_N1:
        m1, cnt = kc.reference_answer(kc.get(f"long_rows-{n}"))[4::3]
        for b in range(2):
            rows = set(m1[b, :cnt[b]].tolist())
            assert {0, 63, 64, n - 1} <= rows and (n <= 1024 or {1023, 1024} <= rows) and (n < 2049 or {2047, 2048} <= rows)
    re = kc.get("ratio-edge")
    assert re.D == 96 and kc.reference_answer(re)[7].tolist() == [32]


# ---- check() has teeth ----------------------------------------------------------------------------------------------------------
def _answer(name, ratio_test=True):
    case = kc.get(name)
    return case, [a.copy() for a in kc.reference_answer(case, ratio_test=ratio_test)]


def _check(case, out, ratio_test=True):
    kc.check(case.d1, case.d2, case.ratio, ratio_test, out, allow_undecided=not case.strict, tag=case.name, refs=case.refs)


def test_check_raises_for_a_swapped_pair():
    case, out = _answer("edges-129x257")
    _check(case, out)
    i = int(np.nonzero(case.refs[0].order_decided)[0][7])
    for a, b in ((out[0], out[1]), (out[2], out[3])):
        a[0, i], b[0, i] = b[0, i], a[0, i]
    with pytest.raises(AssertionError, match="no contender for first place"):
        _check(case, out)
    # the swap of an exact tie keeps both contenders: only the lowest-index rule rejects it
    case, out = _answer("dup-33")
    out[0][0, 5], out[1][0, 5] = out[1][0, 5], out[0][0, 5]
    with pytest.raises(AssertionError, match="lowest indices on exact ties"):
        _check(case, out)


@pytest.mark.parametrize("name,delta", [("dup-1", 1), ("dup-33", 33), ("dup-128", 128), ("triple", 50)])
def test_check_raises_for_the_second_copy_reported_first(name, delta):
    case, out = _answer(name, ratio_test=False)
    _check(case, out, ratio_test=False)
    r = case.refs[0]
    if name == "triple":  # (first, third) instead of (first, second)
        out[1][0, 3] += delta
        assert r.C2[3, out[1][0, 3]]
    else:                 # the second copy first: nn1 of the dense output and of the good list
        out[0][0, 3] += delta
        out[1][0, 3] -= delta
        out[5][0, 3] += delta
        assert r.C1[3, out[0][0, 3]] and r.C2[3, out[1][0, 3]]
    with pytest.raises(AssertionError, match="lowest indices on exact ties"):
        _check(case, out, ratio_test=False)


def _drop(a, k, n):
    a[k:n - 1] = a[k + 1:n].copy()


def test_check_raises_for_a_dropped_decided_pass_row():
    case, out = _answer("edges-129x257")
    st = case.refs[1].ratio_status(case.ratio)
    k = next(k for k in range(out[7][1]) if st[out[4][1, k]] == 1)
    for a in (out[4][1], out[5][1], out[6][1]):
        _drop(a, k, out[7][1])
    out[7][1] -= 1
    with pytest.raises(AssertionError, match="good list is not the rows|decided to pass"):
        _check(case, out)


def test_check_raises_for_an_emitted_decided_fail_row():
    case, out = _answer("edges-129x257")
    st = case.refs[0].ratio_status(case.ratio)
    n = int(out[7][0])
    i = next(i for i in range(case.N1) if st[i] == -1)
    pos = int(np.searchsorted(out[4][0, :n], i))
    for a, v in ((out[4][0], i), (out[5][0], out[0][0, i]), (out[6][0], out[2][0, i])):
        a[pos + 1:n + 1] = a[pos:n].copy()
        a[pos] = v
    out[7][0] += 1
    with pytest.raises(AssertionError, match="good list is not the rows|decided to fail"):
        _check(case, out)
    # the same with the row's distances bent (inside their bounds) so that its own ratio line passes: the reference's decision holds
    case, out = _answer("dup-33")
    r = case.refs[0]
    out[4][0, 0], out[5][0, 0], out[7][0] = 0, out[0][0, 0], 1
    out[2][0, 0] = out[6][0, 0] = np.float32(0.79) * out[3][0, 0]
    with pytest.raises(AssertionError):
        _check(case, out)
    assert r.ratio_status(case.ratio)[0] == -1


def test_check_raises_for_a_non_increasing_good_list():
    case, out = _answer("edges-129x257")
    for a in (out[4][0], out[5][0], out[6][0]):
        a[[3, 4]] = a[[4, 3]]
    with pytest.raises(AssertionError, match="strictly increasing"):
        _check(case, out)
    case, out = _answer("edges-129x257")
    out[7][1] = case.N1 + 1
    with pytest.raises(AssertionError, match="outside 0"):
        _check(case, out)


@pytest.mark.parametrize("name", ["edges-129x257", "edges-129x257-256", "rand-1100x1000-128"])
@pytest.mark.parametrize("which", [2, 3])
def test_check_raises_for_a_distance_off_by_3E(name, which):
    case, out = _answer(name, ratio_test=False)
    r = case.refs[0]
    i = case.N1 // 2
    t = (r.t1, r.t2)[which - 2][i]
    assert t > 3.0 * r.E and r.order_decided[i]
    for sign in (1.0, -1.0):
        o = [a.copy() for a in out]
        o[which][0, i] = np.float32(np.sqrt(t + sign * 3.0 * r.E))
        with pytest.raises(AssertionError, match="off the float64 radicand|dist1 > dist2"):
            _check(case, o, ratio_test=False)
        o[which][0, i] = np.float32(np.sqrt(t + sign * 0.5 * r.E))  # half the bound passes
        if which == 2:
            o[6][0, i] = o[2][0, i]  # without the ratio test, position i of the good list is row i
        _check(case, o, ratio_test=False)


def test_check_raises_for_an_exact_case_off_by_one_step():
    """E = 0: the radicand must be the integer itself up to the one sqrtf rounding."""
    case, out = _answer("sift-int-128-300x290")
    _check(case, out)
    out[3][1, 17] = np.float32(np.sqrt(case.refs[1].t2[17] + 1.0))
    with pytest.raises(AssertionError, match="off the float64 radicand"):
        _check(case, out)


def test_check_enforces_the_cap_and_the_strict_switch():
    case = kc.get("edges-129x257")
    ans = kc.reference_answer(case)
    # the same queries against two near-duplicates per column (differing in the last bit of one component): every row is undecided
    d2 = np.concatenate((case.d2, case.d2), axis=1).copy()
    d2[:, case.N2:, 0] = np.nextafter(d2[:, case.N2:, 0], np.float32(2.0))
    with pytest.raises(AssertionError, match="over the 1 % cap"):
        kc.check(case.d1, d2, case.ratio, True, ans)
    loose = kc.get("rand-1100x1000-128")
    if sum(kc.undecided_share(loose)[:2]) > 0:
        with pytest.raises(AssertionError, match="built to have none"):
            kc.check(loose.d1, loose.d2, loose.ratio, True, kc.reference_answer(loose), allow_undecided=False, refs=loose.refs)
