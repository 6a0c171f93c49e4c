"""The cheirality kernel (csrc/cheirality_body.h) at its launch edges, held per correspondence to the fp64 restatement of
tests/cheirality_ref.py.

Every device result goes through one comparison (cheirality_cases.check_cheirality): the gauge between the device's candidate order
and the restatement's is resolved from the winner's pose (never by sorting counts); for each of the four candidates the
per-correspondence mask of ops.ransac_in_front(winner = c) equals the restatement's outside its `undecided` band; counts[c] is the
row sum of that mask and lies in the restatement's interval (equal where nothing is undecided); the vote over the device's counts
is the reference's rule, and where the restatement's intervals decide the vote the winner and its pose are the restatement's.
Every case runs the adaptive default, the fp64-only route and both ways of forming the per-pair constants, which must agree bit
for bit.  The cases sit on the edges of the launch: 64-lane tails and the clamped prefetch, one / several wavefronts per pair,
the per-wavefront queue of ambiguous correspondences and its full drain with a carry, NaN rows, no model, the fused routes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cheirality_cases as cc  # noqa: E402
import cheirality_ref as cref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W_IMG, H_IMG = 1241.0, 376.0
TALLY = cc.new_tally()   # pairs of this module compared with no / some undecided correspondences, or not compared at all
SHARES = {}              # case -> share of its (candidate, correspondence) tests that were undecided


def _equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def run(dfepe, name, E, K, m, thr, pre=None, src=None, compare=True):
    """All launch variants of one case (bit-identical), then the default's result through the comparison.  CPU fp32 tensors in."""
    Ed, Kd, md = E.to(DEV).contiguous(), K.to(DEV).contiguous(), m.to(DEV).contiguous()
    pd = None if pre is None else pre.to(DEV).contiguous()
    B = md.shape[0]
    out = dfepe.ops.cheirality(Ed, Kd, md, thr, pre=pd)
    for kw in (dict(fp64_only=True), dict(prepared=True), dict(prepared=False), dict(fp64_only=True, prepared=B < 2048)):
        other = dfepe.ops.cheirality(Ed, Kd, md, thr, pre=pd, **kw)
        assert _equal(out, other), (name, kw)
    torch.cuda.synchronize()
    assert torch.isfinite(out[0]).all(), name
    if not compare:
        return out
    before = dict(TALLY)
    t = cc.new_tally()
    cc.check_cheirality(dfepe, None, Ed, Kd, md, thr, out, pre=pd, tally=t, where=name, src=src)
    for k in ("exact", "undecided"):
        TALLY[k] += t[k]
    for k in ("n_undecided", "n_tests"):
        TALLY[k] += t[k]
    SHARES[name] = t["n_undecided"] / max(1, t["n_tests"])
    print(f"[cheirality edges] {name}: {B} pairs, {t['exact']} with nothing undecided, {t['undecided']} with some "
          f"({t['n_undecided']} of {t['n_tests']} tests undecided); winners {np.bincount(out[1].cpu().numpy() + 1, minlength=5).tolist()}")
    assert TALLY["exact"] + TALLY["undecided"] == before["exact"] + before["undecided"] + B
    return out


def scene(dfepe, B, N, seed, outliers=0.2, noise=0.5, planar=False):
    sc = dfepe.synth.make_scene(B, N, seed=seed, outlier_ratio=outliers, noise_px=noise, planar=planar)
    return sc, cc.unit_E(sc), sc["Ks"].float(), sc["matches_xy_ori"].float()


def tile(B, D, seed, *tensors):
    """B slots over D source pairs under a fixed permutation: (src [B], tensors indexed by it)."""
    src = torch.from_numpy(np.random.default_rng(seed).permutation(B) % D)
    return (src.numpy(),) + tuple(t[src].contiguous() for t in tensors)


def T_K(K):
    T = torch.tensor([[2.0 / W_IMG, 0.0, -1.0], [0.0, 2.0 / H_IMG, -1.0], [0.0, 0.0, 1.0]])
    return (T @ K).contiguous()


def fit_F(dfepe, sc):
    """The fit's fp32 F of random softmax weights (a poor model: a few per cent of the correspondences are ambiguous in fp32)."""
    w = torch.softmax(sc["logits_layers"][0].float().to(DEV), 1).contiguous()
    return dfepe.ops.w8pt_forward(sc["matches_xy_ori"].float().to(DEV), None, w, True, W_IMG, H_IMG, 0.5, False, False)[0].cpu(), w


# ---- lane tails and wavefront counts (B < 2048: min(groups, 4) wavefronts per pair) -----------------------------------------
TAIL_N = [(1, "one lane, prefetch clamped to row 0"), (2, "two lanes, prefetch clamped"), (63, "one group less a lane"),
          (64, "one full group"), (65, "second wavefront with one lane"), (127, "two wavefronts, tail"), (128, "two full groups"),
          (129, "third wavefront with one lane"), (191, "three wavefronts, tail"), (192, "three full groups"),
          (193, "fourth wavefront with one lane"), (255, "four wavefronts, tail"), (256, "four full groups"),
          (257, "wavefront 0 takes a second group of one lane"), (1000, "benchmark N"), (2048, "cooperative-fit maximum"),
          (4096, "16 groups per wavefront"), (8191, "tail lane missing in the last of 128 groups")]


@pytest.mark.parametrize("N", [n for n, _ in TAIL_N], ids=[f"N{n}-{why.replace(' ', '_')}" for n, why in TAIL_N])
def test_lane_tails_and_wavefront_counts(dfepe, N):
    B = 5 if N <= 4096 else 2
    _, E, K, m = scene(dfepe, B, N, seed=1000 + N, outliers=0.3)
    run(dfepe, f"tails N={N}", E, K, m, 50.0)


# ---- one wavefront per pair (B >= 2048), a few dozen distinct pairs tiled through the batch ----------------------------------
@pytest.mark.parametrize("B,N", [(2048, 1), (2048, 64), (2048, 65), (2048, 1000), (2049, 1), (2049, 64), (2049, 65), (2049, 1000),
                                 (4096, 1000)])
def test_one_wavefront_per_pair(dfepe, B, N):
    D = 24 if N < 1000 else 8
    _, E, K, m = scene(dfepe, D, N, seed=B + N, outliers=0.3)
    src, Et, Kt, mt = tile(B, D, B, E, K, m)
    run(dfepe, f"one wavefront B={B} N={N}", Et, Kt, mt, 50.0, src=src)


@pytest.mark.parametrize("N", [65, 1000])
def test_launch_shape_does_not_change_a_count(dfepe, N):
    """The same pairs at B = 2047 (up to four wavefronts per pair, constants through LDS) and B = 2048 (one wavefront, constants
    from the preparation launch): identical outputs."""
    D = 16
    _, E, K, m = scene(dfepe, D, N, seed=N, outliers=0.3)
    src, Et, Kt, mt = tile(2048, D, 7, E, K, m)
    big = run(dfepe, f"launch shape 2048 N={N}", Et, Kt, mt, 50.0, src=src)
    small = run(dfepe, f"launch shape 2047 N={N}", Et[:2047], Kt[:2047], mt[:2047], 50.0, src=src[:2047])
    assert _equal([t[:2047] for t in big], small)


# ---- E quality --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gt", "fit", "random", "scaled_1e-3", "scaled_1e3", "negated"])
def test_E_quality_and_gauge(dfepe, kind):
    B, N = 6, 1000
    sc, E, K, m = scene(dfepe, B, N, seed=31, outliers=0.2)
    if kind == "fit":
        F, _ = fit_F(dfepe, sc)
        E = dfepe.ops.congruence(F.to(DEV), T_K(K).to(DEV)).cpu()
    elif kind == "random":
        E = torch.randn(B, 3, 3, generator=torch.Generator().manual_seed(3))
    elif kind.startswith("scaled"):
        E = E * float(kind.split("_")[1])  # the decomposition is scale-free
    elif kind == "negated":
        E = -E  # flips the device's gauge: the candidate map must absorb it
    out = run(dfepe, f"E {kind}", E, K, m, 50.0)
    if kind in ("scaled_1e-3", "scaled_1e3", "negated"):
        base = dfepe.ops.cheirality(cc.unit_E(sc).to(DEV), K.to(DEV), m.to(DEV), 50.0)
        # the winner's pose is the same camera motion whatever the scale or sign of E
        np.testing.assert_allclose(out[0].cpu().numpy(), base[0].cpu().numpy(), atol=2e-5)


# ---- cameras ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", ["kitti", "fy_ne_fx", "identity_normalised", "K_per_pair"])
def test_cameras(dfepe, camera):
    B, N = 6, 500
    sc, E, K, m = scene(dfepe, B, N, seed=41, outliers=0.2)
    if camera == "fy_ne_fx":
        m, K = cc.scaled_y(sc)
        m, K = m.float(), K.float()
    elif camera == "identity_normalised":
        Ki = torch.linalg.inv(sc["Ks"].double())
        md = sc["matches_xy_ori"].double()
        one = torch.ones(B, N, 1, dtype=torch.float64)
        n1 = torch.cat((md[..., :2], one), -1) @ Ki.transpose(1, 2)
        n2 = torch.cat((md[..., 2:], one), -1) @ Ki.transpose(1, 2)
        m = torch.cat((n1[..., :2], n2[..., :2]), -1).float()
        K = torch.eye(3).expand(B, 3, 3).contiguous()
    elif camera == "K_per_pair":
        s = torch.tensor([[0.5, 0.5], [1.0, 1.0], [1.5, 0.75], [2.0, 3.0], [0.8, 1.9], [4.0, 4.0]], dtype=torch.float64)
        md, Kd = sc["matches_xy_ori"].double().clone(), sc["Ks"].double().clone()
        md[..., 0::2] *= s[:, None, 0:1]
        md[..., 1::2] *= s[:, None, 1:2]
        Kd[:, 0] *= s[:, 0:1]
        Kd[:, 1] *= s[:, 1:2]
        m, K = md.float(), Kd.float()
        assert not torch.equal(K[0], K[2])
    run(dfepe, f"camera {camera}", E, K, m, 50.0)


# ---- thresholds -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr,why", [(50.0, "default"), (5.0, "lower edge of the scene"), (0.5, "below every depth: no candidate counts"),
                                     (1e6, "never cuts"), (20.0, "inside the 5-35 m scene: the upper bound cuts")])
def test_thresholds(dfepe, thr, why):
    _, E, K, m = scene(dfepe, 6, 1000, seed=51, outliers=0.2)
    out = run(dfepe, f"thr {thr}", E, K, m, thr)
    cnt = out[2].cpu().numpy()
    if thr == 0.5:  # every correspondence is beyond the bound for every candidate: no winner, zero pose
        assert (out[1].cpu().numpy() == -1).all() and (cnt == 0).all() and (out[0] == 0).all()
    if thr == 20.0:
        full = dfepe.ops.cheirality(E.to(DEV), K.to(DEV), m.to(DEV), 50.0)[2].cpu().numpy()
        assert (cnt.max(1) < 0.8 * full.max(1)).all()  # the bound does cut


# ---- far / low-parallax scenes: fp32 cannot decide, fp64 can ----------------------------------------------------------------
@pytest.mark.parametrize("thr", [50.0, 1e6])
@pytest.mark.parametrize("zmin", [200.0, 2e4])
def test_far_scenes(dfepe, zmin, thr):
    E, K, m = cc.far_scene(dfepe, 4, 1000, seed=int(zmin) + int(thr) % 97, zmin=zmin)
    amb = [int(cc.predicted_ambiguous(E[b], K[b], m[b], thr).sum()) for b in range(4)]
    assert min(amb) >= 10, amb  # these scenes do use the fp64 route
    run(dfepe, f"far zmin={zmin:g} thr={thr:g}", E, K, m, thr)


# ---- the queue's full drain: one wavefront collects >= 128 ambiguous correspondences -----------------------------------------
@pytest.mark.parametrize("B,N,D", [(2048, 12288, 2), (3, 32768, 3)], ids=["one_wavefront_per_pair", "four_wavefronts_per_pair"])
def test_queue_full_drain_with_carry(dfepe, B, N, D):
    """Two or more full drains of a wavefront's queue with a non-empty carry.  The kernel's margin rule, evaluated on the CPU with
    exact eigenvectors, predicts for every source pair and every wavefront >= 256 ambiguous correspondences: twice the 128 that
    two drains need (the kernel evaluates the rule on its fp32 vector, which moves single correspondences across the margin).
    thr = 1e4 m sits inside the depth range, so about half of the correspondences are in front of a candidate and a
    correspondence lost or counted twice by the queue changes a count.  The tiled case takes, of six far pairs, the first D the
    RESTATEMENT leaves nothing undecided in (points next to the epipole have s3 ~ s4), so that its 2048 slots are compared
    exactly."""
    thr = 1e4
    nw = cc.wavefronts(B, N)
    assert nw == (1 if B >= 2048 else 4)
    E, K, m = cc.far_scene(dfepe, D if B == D else 6, N, seed=N % 1000, zmin=200.0)
    if B != D:
        keep = [b for b in range(6) if not cref.reference(E[b].numpy(), K[b].numpy(), m[b].numpy(), thr)["undecided"].any()][:D]
        assert len(keep) == D
        E, K, m = E[keep], K[keep], m[keep]
    pred = [cc.per_wavefront(cc.predicted_ambiguous(E[b], K[b], m[b], thr), nw) for b in range(D)]
    print(f"[cheirality edges] drain B={B} N={N}: predicted ambiguous per wavefront {pred}")
    assert min(min(p) for p in pred) >= 256, pred
    # the same prediction run through the queue's rule: every wavefront drains at least four times, at least twice with a carry
    for b in range(D):
        for carries in cc.predicted_drains(cc.predicted_ambiguous(E[b], K[b], m[b], thr), nw):
            assert len(carries) >= 4 and sum(c > 0 for c in carries) >= 2, carries
    if B == D:
        run(dfepe, f"drain B={B} N={N}", E, K, m, thr)
    else:
        src, Et, Kt, mt = tile(B, D, 11, E, K, m)
        run(dfepe, f"drain B={B} N={N}", Et, Kt, mt, thr, src=src)


# ---- NaN rows (the RANSAC leg's mask=) ------------------------------------------------------------------------------------
def test_nan_rows(dfepe):
    pats = ["none", "first", "last", "group", "all_but_one", "all", "one_coordinate"]
    N = 300
    _, E, K, m = scene(dfepe, len(pats), N, seed=61, outliers=0.1)
    m = m.clone()
    nan = float("nan")
    m[1, 0] = nan
    m[2, N - 1] = nan
    m[3, 64:128] = nan
    m[4, :] = nan
    m[4, 77] = scene(dfepe, len(pats), N, seed=61, outliers=0.1)[3][4, 77]
    m[5, :] = nan
    m[6, ::3, 2] = nan
    out = run(dfepe, "NaN rows", E, K, m, 50.0)
    Rt, win, cnt = (t.cpu().numpy() for t in out)
    assert win[5] == -1 and (cnt[5] == 0).all() and (Rt[5] == 0).all()
    assert cnt[4].max() <= 1 and cnt[1].max() > 100 and cnt[6].max() <= N - N // 3, cnt
    # and with one wavefront per pair
    src, Et, Kt, mt = tile(2048, len(pats), 5, E, K, m)
    run(dfepe, "NaN rows B=2048", Et, Kt, mt, 50.0, src=src)


# ---- no model -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["zero", "rank1"])
def test_no_model_is_finite_and_self_consistent(dfepe, kind):
    """An all-zero or rank-1 E has no pose: the SVD gauge is arbitrary, so the restatement is not compared (these pairs count
    against the module's 95 % condition).  Whatever the kernel returns is finite, the same in every variant, its counts are
    within [0, N], the vote over them is the reference's rule and the pose is zero exactly when there is no winner."""
    B, N = 4, 300
    _, E, K, m = scene(dfepe, B, N, seed=71)
    if kind == "zero":
        E = torch.zeros(B, 3, 3)
    else:
        g = torch.Generator().manual_seed(1)
        E = torch.randn(B, 3, 1, generator=g) @ torch.randn(B, 1, 3, generator=g)
    out = run(dfepe, f"no model {kind}", E, K, m, 50.0, compare=False)
    Rt, win, cnt = (t.cpu().numpy() for t in out)
    assert ((cnt >= 0) & (cnt <= N)).all()
    for b in range(B):
        assert cref.select(cnt[b]) == win[b]
        assert (Rt[b] == 0).all() == (win[b] < 0)
    TALLY["skipped"] += B


def test_correspondences_behind_every_candidate(dfepe):
    """A pair made of correspondences that NO candidate sees in front of both cameras (second-view points drawn at random; those
    kept are the ones the restatement decides, outside its band, to be behind a camera or beyond the bound for all four
    candidates): no winner, zero counts, zero pose -- at both launch shapes."""
    N = 300
    sc, E, K, m = scene(dfepe, 2, 6000, seed=91, outliers=1.0)
    rows = []
    for b in range(2):
        r = cref.reference(E[b].numpy(), K[b].numpy(), m[b].numpy(), 50.0)
        keep = np.nonzero(~r["in_front"].any(0) & ~r["undecided"].any(0))[0]
        assert len(keep) >= N, len(keep)
        rows.append(m[b, torch.from_numpy(keep[:N])])
    m = torch.stack(rows).contiguous()
    for B in (2, 2048):
        src, Et, Kt, mt = tile(B, 2, 3, E, K, m)
        out = run(dfepe, f"behind every candidate B={B}", Et, Kt, mt, 50.0, src=src)
        assert (out[1] == -1).all() and (out[2] == 0).all() and (out[0] == 0).all()


# ---- the fused routes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", [(1, 129), (9, 1000), (512, 2048), (1280, 129), (1281, 129), (3071, 129), (3072, 129), (9, 2049)],
                         ids=["B1-N129_first_cooperative_N", "B9-N1000", "B512-N2048_last_cooperative_N", "B1280_last_cooperative_B",
                              "B1281_two_launches", "B3071_two_launches_below_backward_limit", "B3072_two_launches_at_backward_limit",
                              "N2049_two_launches"])
def test_fused_routes(dfepe, B, N):
    """ops.cheirality(F, pre = T K) and ops.fit_pose (one cooperative launch for 128 < N <= 2048 up to 1280 pairs, the forward fit's limit
    for pixel matches; csrc/fit_plan.h.  3072 pairs is the BACKWARD fit's limit: the forward takes the two launches on both sides of it)
    through the same comparison, the restatement's E formed in fp64 from the fp32 F the device returns."""
    D = min(B, 8)
    sc = dfepe.synth.make_scene(D, N, seed=B + N, outlier_ratio=0.2, noise_px=0.5)
    src = np.random.default_rng(B).permutation(B) % D
    idx = torch.from_numpy(src)
    m = sc["matches_xy_ori"].float()[idx].contiguous().to(DEV)
    K = sc["Ks"].float()[idx].contiguous().to(DEV)
    w = torch.softmax(sc["logits_layers"][0].float()[idx].to(DEV), 1).contiguous()
    TK = T_K(K.cpu()).to(DEV)
    res = dfepe.ops.fit_pose(m, w, K, W_IMG, H_IMG, 50.0, pre=TK)
    F, fused = res[0], res[4:7]
    two = dfepe.ops.cheirality(F, K, m, 50.0, pre=TK)
    three = dfepe.ops.cheirality(dfepe.ops.congruence(F, TK), K, m, 50.0)
    torch.cuda.synchronize()
    assert _equal(fused, two) and _equal(fused, three)
    run(dfepe, f"fused B={B} N={N}", F.cpu(), K.cpu(), m.cpu(), 50.0, pre=TK.cpu(), src=src)


# ---- compat ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,thr", [(257, 50.0), (1000, 20.0)])
def test_compat_wrappers_return_the_same_winner_pose(dfepe, N, thr):
    uf = dfepe.compat.utils_F
    _, E, K, m = scene(dfepe, 2, N, seed=81 + N, outliers=0.2)
    out = run(dfepe, f"compat N={N}", E, K, m, thr)
    for b in range(2):
        args = (E[b].to(DEV), K[b].numpy(), m[b, :, :2].numpy(), m[b, :, 2:].numpy())
        for fn in (uf._E_to_M_train, uf._E_to_M):
            res = fn(*args, depth_thres=thr, show_result=False)
            if int(out[1][b]) < 0:
                assert res[2] is None
            else:
                assert torch.equal(res[2], out[0][b])


def test_module_compared_most_pairs_with_nothing_undecided():
    """Runs last in the module: how many pairs were compared with no undecided correspondence, with some, or not at all."""
    n = TALLY["exact"] + TALLY["undecided"] + TALLY["skipped"]
    print(f"[cheirality edges] module: {n} pairs, {TALLY['exact']} with nothing undecided, {TALLY['undecided']} with some, "
          f"{TALLY['skipped']} not compared; {TALLY['n_undecided']} of {TALLY['n_tests']} (candidate, correspondence) tests undecided, "
          f"worst case share {max(SHARES.values(), default=0.0):.2e}")
    if n:
        assert TALLY["exact"] >= 0.95 * n
        assert max(SHARES.values(), default=0.0) <= 1e-3, {k: v for k, v in SHARES.items() if v > 1e-3}
