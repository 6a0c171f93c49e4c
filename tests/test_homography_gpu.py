"""csrc/homography.hip on the GPU, stage by stage against the fp64 restatement (tests/homography_ref.py) through the check() of
tests/homography_cases.py: the count table per iteration, the rule on it (best count, winning iteration, iterations consumed),
H_model, the mask, the refit (NO_REFINE), H_out, the transfer and corner measures, and the compat layer on top.  Tolerances and
bands: tests/homography_cases.py and tests/homography_ref.py (measured against the 50-digit twin, never against the kernel)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import homography_cases as hc  # noqa: E402
import homography_ref as hr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = []  # what check() called every pair compared in this module: the cap on ambiguous pairs is over all of them


def run(dfepe, mats, n_list, t, p, iters, seed, flags, with_refit=True):
    """One launch sequence over the batch `mats` (list of [N,4] arrays of one N) -> list of per-pair dicts for hc.check()."""
    m = torch.as_tensor(np.stack(mats), device=DEV)
    nv = None if all(n is None for n in n_list) else torch.as_tensor([m.shape[1] if n is None else n for n in n_list], dtype=torch.int32, device=DEV)
    kw = dict(n_valid=nv, threshold=t, confidence=p, max_iters=iters, seed=seed, all_points=bool(flags & hr.ALL_POINTS))
    o = dfepe.ops.ransac_homography(m, refine=not flags & hr.NO_REFINE, want_hyp_counts=True, want_model=True, **kw)
    o2 = dfepe.ops.ransac_homography(m, refine=False, **kw) if with_refit and not flags & hr.NO_REFINE else None
    c = {k: (None if v is None else v.cpu().numpy()) for k, v in o.items()}
    out = []
    for b in range(len(mats)):
        g = {"table": None if flags & hr.ALL_POINTS else c["hyp_counts"][b].astype(np.int64), "best": c["n_inliers"][b], "best_k": c["best_iter"][b],
             "iters": c["iters_run"][b], "H_model": c["H_model"][b], "mask": c["mask"][b]}
        if flags & hr.NO_REFINE:
            g["H_refit"] = c["H"][b]
        else:
            g["H_out"] = c["H"][b]
            if o2 is not None:
                g["H_refit"] = o2["H"][b].cpu().numpy()
                if c["n_inliers"][b] > 4:  # the refinement's own cost before and after, from the reported matrices and mask
                    g["S0"], g["S1"] = hc.cost(g["H_refit"], mats[b], c["mask"][b]), hc.cost(g["H_out"], mats[b], c["mask"][b])
        out.append(g)
    return out, o


def run_and_check(dfepe, jobs):
    """jobs: (name, N, n, t, p, iters, seed, flags); batched by everything but (name, n).  Returns the kinds check() gave."""
    groups = {}
    for j in jobs:
        groups.setdefault((j[1],) + tuple(j[3:]), []).append(j)
    kinds = []
    for (N, t, p, iters, seed, flags), js in groups.items():
        got, _ = run(dfepe, [hc.pair(j[0], N) for j in js], [j[2] for j in js], t, p, iters, seed, flags)
        for j, g in zip(js, got):
            r = hc.ref(j[0], N, j[2], t, p, iters, seed, flags)
            kinds.append(hc.check(g, r, hc.pair(j[0], N), t, p, what=f"{j[0]} N={N} n={j[2]} t={t} p={p} iters={iters} seed={seed} flags={flags}"))
    KINDS.extend(kinds)
    return kinds


def test_every_family_setting_and_pair_size(dfepe):
    """The job list the host build is held to (tests/test_homography_ref_cpu.py): every family at every setting, both flags,
    n_valid 0 / 3 / 4 / 5 / N in mixed batches, the pair without a sample and the pair whose sampler stops."""
    kinds = run_and_check(dfepe, hc.jobs())
    assert kinds.count("ambiguous") <= 0.10 * len(kinds)


# the last N whose count launch stays inside 64 KiB of LDS (16 N + 64 * 72 + 512 bytes) is 3776
@pytest.mark.parametrize("N", [4, 5, 63, 64, 65, 255, 256, 257, 1000, 3776, 3777, 4096])
def test_number_of_correspondences(dfepe, N):
    kinds = run_and_check(dfepe, [("synth_30_5_4", N, None, 3.0, 0.995, 16, 0, 0)])
    assert kinds == ["exact"]


@pytest.mark.parametrize("iters", [1, 2, 63, 64, 65, 128, 129, 2000])
def test_number_of_iterations(dfepe, iters):
    # 60 % outliers keep the rule from stopping early, so that the table is read past every chunk edge
    names = ("synth_60_5_7", "synth_30_0_3", "noise") if iters < 2000 else ("synth_60_5_7",)
    kinds = run_and_check(dfepe, [(n, hc.N_DEFAULT, None, 3.0, 0.995, iters, 0, 0) for n in names])
    assert "ambiguous" not in kinds


@pytest.mark.parametrize("t", [1.0, 3.0, 5.0, 0.0, -2.0])
@pytest.mark.parametrize("p", [0.0, 0.5, 0.995, 1.0])
def test_threshold_and_confidence(dfepe, t, p):
    # confidence 0 stops at the first model, whatever it is: a fit to five points whose refinement is ill-posed may be called
    # ambiguous by the restatement (the invariants are still checked); the cap at the end of the module counts it
    run_and_check(dfepe, [(n, hc.N_DEFAULT, None, t, p, 64, 0, 0) for n in ("synth_30_5_4", "synth_60_0_6", "projective")])


@pytest.mark.parametrize("seed", [0, 3, (1 << 64) - 1])
def test_seed(dfepe, seed):
    kinds = run_and_check(dfepe, [(n, hc.N_DEFAULT, None, 3.0, 0.995, 64, seed, 0) for n in ("synth_30_5_4", "duplicates", "w_zero")])
    assert "ambiguous" not in kinds


@pytest.mark.parametrize("B", [1, 3, 5, 7])
def test_batch_size_and_bit_identity(dfepe, B):
    """B pairs in one call: every pair as in a call of its own (bit for bit), two calls bit-identical, n_valid = N as NULL."""
    names = hc.FAMILIES[:B]
    mats = [hc.pair(n) for n in names]
    _, a = run(dfepe, mats, [None] * B, 3.0, 0.995, 64, 0, 0, with_refit=False)
    _, b = run(dfepe, mats, [None] * B, 3.0, 0.995, 64, 0, 0, with_refit=False)
    _, c = run(dfepe, mats, [hc.N_DEFAULT] * B, 3.0, 0.995, 64, 0, 0, with_refit=False)
    for k, v in a.items():
        assert torch.equal(v, b[k]) and torch.equal(v, c[k]), k
    for i in range(B):
        _, s = run(dfepe, mats[i:i + 1], [None], 3.0, 0.995, 64, 0, 0, with_refit=False)
        for k, v in a.items():
            assert torch.equal(v[i], s[k][0]), (k, i)


def test_a_pair_does_not_depend_on_the_batch_around_it(dfepe):
    """4096 pairs of 100 matches, the families in a seeded random order: every copy of a family gives the bits of its first."""
    rng = np.random.default_rng(5)
    which = rng.integers(0, len(hc.FAMILIES), 4096)
    base = torch.as_tensor(np.stack([hc.pair(n) for n in hc.FAMILIES]), device=DEV)
    idx = torch.as_tensor(which, device=DEV)
    o = dfepe.ops.ransac_homography(base[idx].contiguous(), max_iters=64, want_hyp_counts=True, want_model=True)
    s = dfepe.ops.ransac_homography(base, max_iters=64, want_hyp_counts=True, want_model=True)
    for k, v in o.items():
        assert torch.equal(v, s[k][idx]), k


def test_cap_on_ambiguous_pairs():
    """At most 10 % of the pairs compared above may have been held to the invariants only."""
    print(f"{KINDS.count('ambiguous')} of {len(KINDS)} compared pairs ambiguous")
    assert KINDS.count("ambiguous") <= 0.10 * len(KINDS)


def test_capture(dfepe):
    """The three entries make no host synchronisation: a captured call replays to the bits of the eager one."""
    m = torch.as_tensor(np.stack([hc.pair(n) for n in hc.FAMILIES[:4]]), device=DEV)
    Hg = torch.eye(3, dtype=torch.float64, device=DEV).expand(4, 3, 3).contiguous()
    th = torch.tensor([1.0, 3.0, 5.0], dtype=torch.float64, device=DEV)
    eager = dfepe.ops.ransac_homography(m, max_iters=64)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dfepe.ops.ransac_homography(m, max_iters=64)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o = dfepe.ops.ransac_homography(m, max_iters=64)
        d = dfepe.ops.homography_transfer(o["H"], m)
        c = dfepe.ops.homography_corners(o["H"], Hg, hc.HEIGHT, hc.WIDTH, th)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(o["H"], eager["H"]) and torch.equal(o["mask"], eager["mask"])
    de, ce = dfepe.ops.homography_transfer(eager["H"], m), dfepe.ops.homography_corners(eager["H"], Hg, hc.HEIGHT, hc.WIDTH, th)
    assert torch.equal(d[0], de[0]) and torch.equal(d[1], de[1]) and torch.equal(c[1], ce[1])


def test_transfer_and_corners(dfepe):
    """dist to half an fp32 ulp of the fp64 value; the booleans exact outside a band of 64 eps (fp64 evaluation) around the
    threshold; rows past n_valid 0; the all-zero H of a pair without a model gives NaN and 0."""
    names = ("synth_30_5_4", "projective", "w_zero", "noise")
    mats = [hc.pair(n) for n in names]
    Hs = [hc.ref(n)["H_out"] for n in names[:3]] + [np.zeros((3, 3))]
    Hs[2] = np.array([[1.0, 0.02, 3.0], [-0.01, 1.0, -2.0], [-1.0 / 128.0, 0.0, 1.0]])  # row 0 of w_zero has w = 0 exactly
    nv = [None, 37, None, None]
    H = torch.as_tensor(np.stack(Hs), device=DEV)
    m = torch.as_tensor(np.stack(mats), device=DEV)
    n_valid = torch.tensor([100 if n is None else n for n in nv], dtype=torch.int32, device=DEV)
    for epi in (1.0, 3.0, 5.0):
        dist, mask = (x.cpu().numpy() for x in dfepe.ops.homography_transfer(H, m, n_valid, epi))
        for b in range(4):
            n = 100 if nv[b] is None else nv[b]
            with np.errstate(all="ignore"):
                ref = hr.transfer_dist(Hs[b], mats[b][:n])
            fin = np.isfinite(ref)
            np.testing.assert_allclose(dist[b, :n][fin], ref[fin], rtol=hc.DIST_RTOL + 64 * hc.EPS)
            assert not np.isfinite(dist[b, :n][~fin]).any()
            sure = fin & (np.abs(ref - epi) > 64 * hc.EPS * epi)
            np.testing.assert_array_equal(mask[b, :n][sure], ref[sure] < epi)
            assert not mask[b, :n][~fin].any() and not mask[b, n:].any() and not dist[b, n:].any()
    th = torch.tensor([1.0, 3.0, 5.0], dtype=torch.float64, device=DEV)
    rng = np.random.default_rng(3)
    He = np.stack([hc.random_h(rng) for _ in range(300)] + [np.zeros((3, 3))])
    Hg = np.stack([h + rng.normal(0, 1, (3, 3)) * [[1e-3, 1e-3, 2.0], [1e-3, 1e-3, 2.0], [1e-6, 1e-6, 0.0]] for h in He])
    md, ok = (x.cpu().numpy() for x in dfepe.ops.homography_corners(torch.as_tensor(He, device=DEV), torch.as_tensor(Hg, device=DEV), hc.HEIGHT,
                                                                     hc.WIDTH, th))
    ref = np.array([hr.corner_mean_dist(a, b, hc.HEIGHT, hc.WIDTH) for a, b in zip(He, Hg)])
    assert np.isnan(md[-1]) and not ok[-1].any()
    np.testing.assert_allclose(md[:-1], ref[:-1], rtol=64 * hc.EPS, atol=64 * hc.EPS * hc.WIDTH)
    assert 30 < ok[:-1, 1].sum() < 290  # the thresholds cut through the sample
    for j, tj in enumerate((1.0, 3.0, 5.0)):
        sure = np.abs(ref[:-1] - tj) > 64 * hc.EPS * hc.WIDTH
        np.testing.assert_array_equal(ok[:-1, j][sure], ref[:-1][sure] <= tj)


def test_find_homography_layout(dfepe):
    C = dfepe.compat
    m = hc.pair("synth_30_5_4")
    r = hc.ref("synth_30_5_4", max_iters=64)
    H, mask = C.utils_opencv.findHomography(m[:, :2], m[:, 2:], 8, 3.0, maxIters=64)
    assert H.shape == (3, 3) and H.dtype == np.float64 and mask.shape == (100, 1) and mask.dtype == np.uint8 and H[2, 2] == 1.0
    np.testing.assert_array_equal(mask[:, 0], r["mask"])
    assert hr.max_transfer_diff(H, r["H_out"], m[r["mask"] > 0]) <= hc.tol_refine(r["kappa_refit"]) + r["lm_slack"]
    H2, _ = C.findHomography(m[:, None, :2], m[:, None, 2:], 8, 3.0, 64)  # cv2 also takes [N,1,2]
    assert np.array_equal(H, H2)
    m0 = hc.pair("synth_0_5_1")
    H0, mask0 = C.utils_opencv.findHomography(m0[:, :2], m0[:, 2:], 0)
    r0 = hc.ref("synth_0_5_1", max_iters=1, flags=hr.ALL_POINTS)
    assert mask0.all() and hr.max_transfer_diff(H0, r0["H_out"], m0) <= hc.tol_refine(r0["kappa_refit"]) + r0["lm_slack"]
    c = hc.pair("collinear", 50)
    Hn, maskn = C.utils_opencv.findHomography(c[:, :2], c[:, 2:], 8, maxIters=3)
    assert Hn is None and maskn.shape == (50, 1) and not maskn.any()
    np.testing.assert_array_equal(C.get_inliers_cv(m), C.utils_opencv.findHomography(m[:, :2], m[:, 2:])[1].flatten())
    d = hr.transfer_dist(r["H_out"], m)
    sure = np.abs(d - 3.0) > 1e-9
    np.testing.assert_array_equal(C.get_inliers(m, r["H_out"], 3)[sure], d[sure] < 3.0)


def _planted(seed, n_match, n_extra, H, noise):
    """Unit descriptors with planted mutual neighbours: match i of image 1 and of image 2 share a direction (plus a little
    noise); the extra keypoints of either image get directions of their own."""
    rng = np.random.default_rng(seed)
    D = 64
    base = rng.standard_normal((n_match + 2 * n_extra, D))
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    d1 = np.r_[base[:n_match], base[n_match:n_match + n_extra]]
    d2 = np.r_[base[:n_match] + 0.01 * rng.standard_normal((n_match, D)), base[n_match + n_extra:]]
    d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
    xy1 = np.c_[rng.uniform(0, hc.WIDTH - 1, n_match + n_extra), rng.uniform(0, hc.HEIGHT - 1, n_match + n_extra)]
    xy2 = np.r_[hc.warp(H, xy1[:n_match]) + noise * rng.standard_normal((n_match, 2)),
                np.c_[rng.uniform(0, hc.WIDTH - 1, n_extra), rng.uniform(0, hc.HEIGHT - 1, n_extra)]]
    perm = rng.permutation(n_match + n_extra)  # image 2 lists its keypoints in another order
    prob = lambda xy: np.c_[xy, rng.uniform(0.1, 1.0, len(xy))]  # noqa: E731
    return {"prob": prob(xy1), "warped_prob": prob(xy2[perm]), "desc": d1.astype(np.float32), "warped_desc": d2[perm].astype(np.float32),
            "homography": H}, perm


def test_compute_homography(dfepe):
    C = dfepe.compat.descriptor_evaluation
    H = hc.H_PROJECTIVE
    data, perm = _planted(1, 80, 20, H, 0.3)
    out = C.compute_homography(data, correctness_thresh=[1, 3, 5])
    assert set(out) == {"correctness", "keypoints1", "keypoints2", "matches", "inliers", "homography"}
    np.testing.assert_array_equal(out["keypoints1"], data["prob"][:, [1, 0]])
    mt = out["matches"]
    inv = np.argsort(perm)
    planted = {(i, int(inv[i])) for i in range(80)}
    got = {(int(a), int(b)) for a, b in mt}
    assert planted <= got and np.all(np.diff(mt[:, 0]) > 0) and out["inliers"].shape == (len(mt),) and out["inliers"].dtype == np.uint8
    is_planted = np.array([(int(a), int(b)) in planted for a, b in mt])
    assert out["inliers"][is_planted].sum() >= 75 and out["inliers"][~is_planted].sum() == 0
    # the estimate against the restatement on the same matches
    m = np.c_[data["prob"][mt[:, 0], :2], data["warped_prob"][mt[:, 1], :2]].astype(np.float32)
    r = hr.estimate(m, None, 3.0, 0.995, 2000, 0)
    assert r["ambiguous"] is None
    np.testing.assert_array_equal(out["inliers"], r["mask"])
    assert hr.max_transfer_diff(out["homography"], r["H_out"], m[r["mask"] > 0]) <= hc.tol_refine(r["kappa_refit"]) + r["lm_slack"]
    md = hr.corner_mean_dist(r["H_out"], H, hc.HEIGHT, hc.WIDTH)
    assert min(abs(md - t) for t in (1, 3, 5)) > 1e-6  # the thresholds are not at rounding distance
    np.testing.assert_array_equal(out["correctness"], [md <= 1, md <= 3, md <= 5])
    assert out["correctness"][2]
    assert C.compute_homography(data, correctness_thresh=5)["correctness"] is True
    # an estimate that is not the true homography: the corner error decides
    far = dict(data, homography=np.array([[1, 0, 40.0], [0, 1, 0], [0, 0, 1.0]]) @ H)
    assert not C.compute_homography(far, correctness_thresh=[1, 3, 5])["correctness"].any()
    assert np.allclose(C.homography_estimation([data, far], correctness_thresh=[1, 3, 5]), (out["correctness"].astype(float)) / 2)
    # no model: every match on one line
    rng = np.random.default_rng(2)
    d = rng.standard_normal((30, 64)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    t = np.arange(30.0)
    line = {"prob": np.c_[2 * t + 1, t + 3, np.ones(30)], "warped_prob": np.c_[t + 5, 3 * t + 2, np.ones(30)], "desc": d, "warped_desc": d,
            "homography": np.eye(3)}
    none = C.compute_homography(line)
    assert len(none["matches"]) == 30 and none["correctness"] == 0 and np.array_equal(none["homography"], np.eye(3)) and not none["inliers"].any()
