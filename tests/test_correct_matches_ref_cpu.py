"""The optimal correction at every geometry edge, without a GPU: the fp64 restatement (tests/correct_matches_ref.py) against the
same steps at 50 digits (correct_one_mp), and the host build of csrc/correct_matches_math.h against the restatement, both through
the one check() of tests/correct_matches_cases.py (which lists the families and the bounds).

correct_one_mp runs on every fourth point of a family (a point takes up to 0.15 s where a chart's polynomial has a root near
infinity); every other test runs on all of them.  Figures seen on the host (g++ -O1; printed by the tests, copied to DESIGN.md 3.9):
  restatement against 50 digits   cost <= 2.1e-11 relative (rings[5]; 7.5e-14 on rings[50], <= 1.5e-14 elsewhere), position <= 2.1e-11 px
  header against the restatement  cost <= 9.7e-12 relative (rings[5]), position <= 5.7e-12 px
  near-ties                       0 on every family
With the restatement this file replaces -- all six roots from one numpy.roots call -- the ladder test below fails at
tz = 1e-15, 1e-12 and 1e-9: its cost is up to 1.3e16 and 3.4e5 times the scan's at the first two (shown once by putting it back)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import correct_matches_cases as cs  # noqa: E402
import correct_matches_ref as ref  # noqa: E402

NAMES = cs.names()
MP_STRIDE = 4


@functools.lru_cache(maxsize=None)
def mp_point(name, i):
    """correct_one_mp of point i of a family, computed once."""
    F, P, Q = cs.family(name)
    return ref.correct_one_mp(F, P[i], Q[i])


@pytest.fixture(scope="module")
def headers():
    """name -> (out [n,5] fp64, candidates) of the host header, computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = cs.header(*cs.family(name))
        return cache[name]
    return get


@pytest.mark.parametrize("name", NAMES)
def test_restatement_against_50_digits(name):
    """The fp64 restatement is itself within the bounds it lends to the header and the kernel (or the family is listed in
    cases.WIDER with this test's figure)."""
    F, P, Q = cs.family(name)
    R = cs.reference(name)
    idx = np.arange(0, len(P), MP_STRIDE)
    T = [mp_point(name, int(i)) for i in idx]
    want = np.array([np.r_[t["p"], t["q"], t["cost"]] for t in T])
    got = cs.as_array(R)[idx]
    assert np.array_equal(np.isnan(got), np.isnan(want))
    cost, pos = cs.distance(got, want, R["near_tie"][idx])
    print(f"CM restatement against 50 digits, {name}: cost {cost:.2e} relative, position {pos:.2e} px ({len(idx)} points)")
    cost_rel, pos_tol = cs.bounds(name)
    if name in cs.WIDER:  # the widened bound is 4 x the distance measured here: the distance itself is a quarter of it
        cost_rel, pos_tol = max(cost_rel / 4, cs.COST_REL), max(pos_tol / 4, cs.POS_FP64)
    assert cost <= cost_rel and pos <= pos_tol


@pytest.mark.parametrize("name", NAMES)
def test_restatement_through_the_check(name):
    """The restatement's own output: on the geometry, cost = squared displacement, never above the scan, the closed form where
    there is one, and by itself at most 1 % near-ties."""
    R = cs.reference(name)
    assert R["near_tie"].sum() <= cs.TIE_CAP * len(R["cost"])
    cs.check(cs.as_array(R), name, tag=f"restatement {name}")


@pytest.mark.parametrize("tz", cs.TZ)
def test_near_infinity_ladder(tz):
    """The regression test of the restatement: a pure translation whose epipoles move out to infinity.  One numpy.roots call on
    the sextic in t divides by a leading coefficient of order f1^4 (printed) and returned noise from tz = 1e-9 down."""
    name = f"near_infinity[{tz:g}]"
    F, P, Q = cs.family(name)
    R = cs.reference(name)
    e1 = ref.epipoles(F / np.abs(F).max())[0]
    f1 = e1[2] / np.hypot(e1[0] - P[:, 0] * e1[2], e1[1] - P[:, 1] * e1[2])
    print(f"CM {name}: f1^4 between {(f1 ** 4).min():.1e} and {(f1 ** 4).max():.1e}")
    assert np.isfinite(R["cost"]).all() and not R["near_tie"].any()
    top = cs.scan_min(name) * (1 + cs.SCAN_REL) + cs.SCAN_ABS
    assert (R["cost"] <= top).all(), f"{name}: the restatement is up to {(R['cost'] / top).max():.3g} x the scan's cost"
    # at this tz the geometry is, to every bound here, the planar one (epipoles AT infinity), whose restatement shares no root with it
    if tz <= 1e-12:
        Rp = ref.correct_matches(cs.family("planar_translation")[0], P, Q)
        assert cs.distance(cs.as_array(R), cs.as_array(Rp))[0] <= 1e-9


@pytest.mark.parametrize("name", NAMES)
def test_header_through_the_check(headers, name):
    out, _ = headers(name)
    cs.check(out, name)


@pytest.mark.parametrize("name", NAMES)
def test_header_exact_relations(headers, name):
    """Bit for bit: -F (every sextic coefficient and both cross products are even in F) and 2^+-40 F.  To the bounds of check():
    correct(F^T, q, p) = (q', p') with the same cost."""
    F, P, Q = cs.family(name)
    out, _ = headers(name)
    for G, what in ((-F, "-F"), (F * 2.0 ** 40, "2^40 F"), (F * 2.0 ** -40, "2^-40 F")):
        assert np.array_equal(cs.header(G, P, Q)[0], out, equal_nan=True), f"{name}: {what}"
    t = cs.header(np.ascontiguousarray(F.T), Q, P)[0]
    cs.check(np.ascontiguousarray(t[:, [2, 3, 0, 1, 4]]), name, tag=f"{name} transposed")


@pytest.mark.parametrize("name", NAMES)
def test_every_real_root_of_odd_multiplicity_is_among_the_headers_candidates(headers, name):
    """A real root t of the restatement counts as found when a candidate of the header lies within 1e-9 max(1, |t|) of it.  Its
    multiplicity is counted at 50 digits: the roots of correct_one_mp's polynomial within 1e-7 of it in its chart.  Where the sextic
    touches zero without changing sign the bracketing sees nothing, by design, and such a root must not count
    (the double roots of "on_geometry" mostly do not even reach this test: numpy.roots returns them as complex pairs).  A root with |1 / t| <= 1e-15 is t = infinity to the resolution of its chart ([-1, 1] in
    fp64), which is always a candidate: "rectified" has a fivefold root there that numpy.roots returns as 1 / t ~ 1e-18."""
    F, P, Q = cs.family(name)
    R = cs.reference(name)
    _, cand = headers(name)
    n_odd = n_even = 0
    for i in range(0, len(P), MP_STRIDE):
        T = mp_point(name, i)
        c = cand[i]
        assert np.isinf(c).sum() >= 1 and len(c) <= 13  # t = infinity, and again where u = 0 is a root
        c = c[np.isfinite(c)]
        for t in R["roots"][i]:
            zs, x = (T["roots_t"], t) if abs(t) <= 1 else (T["roots_u"], 1.0 / t)
            mult = sum(1 for z in zs if abs(complex(z) - x) <= 1e-7)
            if mult % 2 == 0:
                n_even += 1
                continue
            n_odd += 1
            if abs(t) >= 1e15:
                continue
            assert len(c) and np.abs(c - t).min() <= 1e-9 * max(1.0, abs(t)), (name, i, t, mult, c)
    print(f"CM {name}: {n_odd} real roots of odd multiplicity found among the candidates, {n_even} of even multiplicity not required")
    assert n_odd + n_even > 0
