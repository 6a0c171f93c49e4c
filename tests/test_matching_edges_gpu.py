"""Descriptor matching (csrc/match.hip) held to its float64 restatement (tests/match_ref.py) at every tile and tie edge: every case of
tests/matching_cases.py goes through ops.nn_match_two_way and the one check(); then the strictness of `score < nn_thresh` with no
margin, non-contiguous inputs, gather_matches against plain indexing, and bit-identical reruns.  Each test is a handful of launches of
at most a few hundred tiles.

The largest |score^2 - t64| the device showed per D is printed when the module finishes (and quoted in DESIGN.md 5) next to the
derived bound E(D) it must stay under; no bound is set from it."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_ref as mr  # noqa: E402
import matching_cases as mc  # noqa: E402

DEV = "cuda:0"
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _print_record():
    """After the module: the largest |score^2 - t64| the cases showed per D (the figures of DESIGN.md 5).  Each was asserted under its
    bound by check(); this only prints."""
    yield
    for D in sorted(mc.RECORD):
        worst, ratio = mc.RECORD[D]
        print(f"\nMATCH RECORD D = {D}: max |score^2 - t64| = {worst:.3e}, {ratio:.4f} of its bound (E(D) = {mr.bound(D):.3e})")


def _dev(case):
    return torch.tensor(case.d1, device=DEV), torch.tensor(case.d2, device=DEV)


def _host(out):
    return [t.cpu().numpy() for t in out]


@pytest.mark.parametrize("name", mc.CASES)
def test_nn_match_case_vs_fp64_reference(dfepe, name):
    case = mc.get(name)
    m1, m2, sc, cnt = _host(mc.run(dfepe, case, device=DEV))
    # what the descriptions of the cases promise beyond the reference's decided rows
    if name.startswith("all_equal"):
        assert cnt.tolist() == [1] and (m1[0, 0], m2[0, 0]) == (0, 0)
    if name == "clipped":
        assert cnt.tolist() == [25] and (sc[0, :25] == 0.0).all()
    if name == "perm1100":
        assert cnt.tolist() == [1100, 1100] and (m1 == np.arange(1100)).all()
    if name == "none1100":
        assert cnt.tolist() == [0, 0]
    if name.startswith("remap"):
        assert cnt[case.B // 2] == 0 and len(set(cnt.tolist())) == case.B
    if name.startswith("long_rows"):
        assert cnt.tolist() == [130, 130]


def test_threshold_is_strict_with_no_margin(dfepe):
    """`d < nn_thresh`, not `<=`: at nn_thresh = the float32 score of a match, that match (and every one with the same score) is gone
    and all matches with a smaller score are unchanged; one float32 step above, it is back."""
    case = mc.get("edges-129x257")
    d1, d2 = _dev(case)
    m1, m2, sc, cnt = _host(mc.run(dfepe, case, thr=mr.pick_threshold(case.refs, 1.3), device=DEV))  # generous; held to the reference
    for b in range(case.B):
        n = int(cnt[b])
        assert n > 20
        base = {(int(i), int(j)): s for i, j, s in zip(m1[b, :n], m2[b, :n], sc[b, :n])}
        k = n // 2
        s = np.float32(sc[b, k])
        key = (int(m1[b, k]), int(m2[b, k]))
        assert 0 < sum(v < s for v in base.values()) < n - 1
        for thr, inside in ((float(s), lambda v: v < s), (float(np.nextafter(s, np.float32(np.inf))), lambda v: v <= s)):
            a1, a2, asc, acnt = _host(dfepe.ops.nn_match_two_way(d1, d2, thr))
            na = int(acnt[b])
            got = {(int(i), int(j)): v for i, j, v in zip(a1[b, :na], a2[b, :na], asc[b, :na])}
            assert got == {p: v for p, v in base.items() if inside(v)}, (b, thr)
            assert (a1[b, 1:na] > a1[b, :na - 1]).all()
            assert (key in got) == (thr > float(s)), (b, thr)


def test_non_contiguous_inputs_equal_the_contiguous_call(dfepe):
    case = mc.get("edges-129x257")
    d1, d2 = _dev(case)
    ref = _host(dfepe.ops.nn_match_two_way(d1, d2, case.thr))
    # a [B,D,N] tensor transposed, and a slice of a wider tensor
    t1, t2 = d1.transpose(1, 2).contiguous().transpose(1, 2), d2.transpose(1, 2).contiguous().transpose(1, 2)
    w1 = torch.full((case.B, case.N1 + 3, case.D + 32), 7.0, device=DEV)
    w2 = torch.full((case.B, case.N2 + 5, case.D + 32), -7.0, device=DEV)
    w1[:, 2:2 + case.N1, 16:16 + case.D] = d1
    w2[:, 1:1 + case.N2, 32:] = d2
    s1, s2 = w1[:, 2:2 + case.N1, 16:16 + case.D], w2[:, 1:1 + case.N2, 32:]
    assert not t1.is_contiguous() and not t2.is_contiguous() and not s1.is_contiguous() and not s2.is_contiguous()
    for a, b in ((t1, t2), (s1, s2), (t1, s2)):
        out = _host(dfepe.ops.nn_match_two_way(a, b, case.thr))
        n = ref[3]
        np.testing.assert_array_equal(out[3], n)
        for x, y in zip(out[:3], ref[:3]):
            for p in range(case.B):
                np.testing.assert_array_equal(x[p, :n[p]], y[p, :n[p]])


@pytest.fixture(scope="module")
def gather_inputs(dfepe):
    """(B=3, N1=129, N2=257): m1, m2, sc, count of a real match call (held to the reference), keypoints and offsets."""
    case = mc.get("remap-3")
    thr = mr.pick_threshold(case.refs, 1.0)  # every pair has matches at this threshold
    m1, m2, sc, cnt = mc.run(dfepe, case, thr=thr, device=DEV)
    assert int(cnt.min()) >= 5
    g = torch.Generator().manual_seed(5)
    pts1, pts2 = (torch.randint(0, 1241, (3, n, 2), generator=g).float().to(DEV) for n in (case.N1, case.N2))
    off1, off2 = ((torch.rand(3, n, 2, generator=g) - 0.5).to(DEV) for n in (case.N1, case.N2))
    return m1, m2, sc, cnt, pts1, pts2, off1, off2


@pytest.mark.parametrize("n_out", [1, 85, 86, 256, 300, 1000])
def test_gather_matches_vs_plain_indexing(dfepe, gather_inputs, n_out):
    """B n_out = 255 / 258 sit on either side of one 256-thread block; n_out > count pads with repeated positions.  choice holds
    positions in [0, count[b]) only: nothing beyond a pair's count is ever read."""
    m1, m2, sc, cnt, pts1, pts2, off1, off2 = gather_inputs
    B = 3
    rng = np.random.default_rng(n_out)
    c = cnt.cpu().numpy()
    choice = np.stack([rng.integers(0, c[b], n_out) for b in range(B)]).astype(np.int32)
    if n_out >= c.max():  # every position at least once, then repeats: the padding of crop_or_pad_choice
        for b in range(B):
            choice[b, :c[b]] = np.arange(c[b])
    assert all(0 <= choice[b].min() and choice[b].max() < c[b] for b in range(B))
    ch = torch.from_numpy(choice).to(DEV)
    bi = torch.arange(B, device=DEV)[:, None]
    i, j = m1[bi, ch.long()].long(), m2[bi, ch.long()].long()
    want_xs = torch.cat((pts1[bi, i], pts2[bi, j]), dim=2)
    want_off = torch.cat((off1[bi, i], off2[bi, j]), dim=2)
    want_q = sc[bi, ch.long()][..., None]
    for with_off in (False, True):
        xs, offs, q = dfepe.ops.gather_matches(pts1, pts2, off1 if with_off else None, off2 if with_off else None, m1, m2, sc, ch)
        assert xs.shape == (B, n_out, 4) and q.shape == (B, n_out, 1)
        np.testing.assert_array_equal(xs.cpu().numpy(), want_xs.cpu().numpy())
        np.testing.assert_array_equal(q.cpu().numpy(), want_q.cpu().numpy())
        if with_off:
            assert offs.shape == (B, n_out, 4)
            np.testing.assert_array_equal(offs.cpu().numpy(), want_off.cpu().numpy())
        else:
            assert offs is None


@pytest.mark.parametrize("name", ["remap-4", "remap-8", "remap-3"])
def test_reruns_are_bit_identical(dfepe, name):
    """The order in which the tiles' atomicMin arrive must not matter."""
    case = mc.get(name)
    d1, d2 = _dev(case)
    a = _host(dfepe.ops.nn_match_two_way(d1, d2, case.thr))
    b = _host(dfepe.ops.nn_match_two_way(d1, d2, case.thr))
    np.testing.assert_array_equal(a[3], b[3])
    for x, y in zip(a[:3], b[:3]):
        for p in range(case.B):
            n = int(a[3][p])
            np.testing.assert_array_equal(x[p, :n].view(np.uint32), y[p, :n].view(np.uint32))
