"""The batched LMedS estimators (csrc/lmeds.hip) against the fp64 restatement of tests/lmeds_ref.py.

Every device result goes through one comparison (check_pair): the median table, iteration by iteration as sorted medians, within
the restatement's derived bound; the restatement's rule applied to the device's own table must reproduce best_hyp, min_median,
sigma and iters_run exactly; the mask is err <= (float)sigma^2 outside the bound's band; F or E is the winning root to 1e-5 in
unit(); the NaN-masked copy; and the same call with the table in the workspace is bit-identical.  A pair is "ambiguous" -- only its
table is checked against the restatement -- when two medians of the restatement lie within their summed bounds of the minimum; at
most 1 pair in 8 of the module may be.  Below 14 correspondences (10 for E) every pair is: ranks N/2 - 1 and N/2 then lie among
the errors of the sample's own points, every median is rounding noise (1e-27 px^2) and the winner is the implementation's, so
those sizes get one pair each.  The cases sit on the edges of the launches: N = 8 (minimum, even, the sigma floor), the
64-lane and register-ladder tails, the LDS attribute path (16 N + 3712 > 65536 from N = 3865 for F, 16 N + 38592 from N = 1685
for E), N = 4096, the 16-iteration chunks of the median grid and the 64-iteration stride of the select kernel, niters against
max_iters, confidence 0 and 1, a median inside a run of equal errors, a sample missing at k = 1 and at k = 0."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lmeds_ref as ref  # noqa: E402
import ransac5_ref as ref5  # noqa: E402
import ransac_ref as ref7  # noqa: E402
from test_ransac_edges_gpu import KINDS, _pairs  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U64 = (1 << 64) - 1
KITTI_K = np.array([[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1.0]])
TALLY = {"exact": 0, "ambiguous": 0}
OUT_KEYS = ("mask", "n_inliers", "iters_run", "best_hyp", "min_median", "sigma", "masked")
# iterations whose roots cannot be compared one for one (another number of roots on the two sides, or a sample on a double
# root): for F the 0.1 % + 1 of test_ransac_edges_gpu.py for root differences, and as much again for the probe solve; for E two
# fp64 five-point solves of the same sample differ for about one sample in eight on these scenes (test_ransac5_cpu.py), twice
# that is allowed
SKIP_CAP = {7: lambda n: 0.002 * n + 2, 5: lambda n: 0.25 * n + 2}


def unit(F):
    f = np.asarray(F, np.float64).ravel()
    f = f / np.linalg.norm(f)
    return f * np.sign(f[np.argmax(np.abs(f))])


def _bits(x):
    x = x.detach().cpu().contiguous()
    return x.view(torch.uint8) if x.is_floating_point() else x


def _np(out):
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}


def run(dfepe, m, confidence, max_iters, seed, K=None):
    """Device result with the table and the NaN-masked copy; the same call with the table in the workspace must be bit-identical."""
    md = torch.from_numpy(np.ascontiguousarray(m)).to(DEV)
    kw = dict(confidence=confidence, max_iters=max_iters, seed=seed)
    if K is None:
        fn, name = (lambda **k: dfepe.ops.lmeds_fundamental(md, **k)), "F"
    else:
        Kd = torch.from_numpy(np.broadcast_to(np.asarray(K, np.float32), (m.shape[0], 3, 3)).copy()).to(DEV)
        fn, name = (lambda **k: dfepe.ops.lmeds_essential(md, Kd, **k)), "E"
    out = fn(want_hyp_medians=True, want_masked=True, **kw)
    ws = fn(want_masked=True, **kw)
    torch.cuda.synchronize()
    assert ws["hyp_medians"] is None
    for k in (name,) + OUT_KEYS:
        assert torch.equal(_bits(out[k]), _bits(ws[k])), k
    return _np(out)


def check_pair(m, out, b, confidence, seed, max_iters, K=None, models=None):
    """The device result of pair b against the restatement.  Returns "exact" | "ambiguous"."""
    five = K is not None
    mp, roots, name = (5, 10, "E") if five else (7, 3, "F")
    pts = np.asarray(m[b], np.float32)
    N = pts.shape[0]
    niters = ref.num_iters(mp, confidence, max_iters)
    tab = out["hyp_medians"][b]
    assert tab.shape == (niters, roots)
    x = ref5.normalize(pts, K) if five else pts.astype(np.float64)
    if models is None:
        models = ref.models_e(x, seed, niters) if five else ref.models_f(pts, seed, niters)
    med, bnd = ref.median_table(models, x, roots, five)

    # 1. the table: every compared entry within the restatement's bound
    skipped = []
    for k in range(niters):
        row = tab[k]
        if models[k] is None:
            assert (row == ref.NO_SAMPLE).all(), (b, k, row)
            continue
        assert (row != ref.NO_SAMPLE).all(), (b, k, row)
        dev = sorted(float(v) for v in row if v >= 0)
        assert (row[len(dev):] == ref.NO_ROOT).all(), (b, k, row)  # roots first, absent ones after
        assert all(float(np.float32(v)) == v for v in dev), (b, k, row)  # a median is an fp32 value (or +inf)
        want = sorted(float(v) for v in med[k] if v >= 0)
        bk_ = max([0.0] + [float(v) for v in bnd[k][:len(want)]])
        if len(dev) != len(want) or not np.isfinite(bk_):
            skipped.append(k)
            continue
        for a, c in zip(dev, want):
            assert a == c or abs(a - c) <= bk_, (b, k, a, c, bk_)
    assert len(skipped) <= SKIP_CAP[mp](niters), (b, len(skipped), niters)

    # 2a. the restatement's rule over the device's own table gives the device's outputs exactly
    best, bk, br, it = ref.select(tab, niters)
    sg = ref.sigma_of(best, N, mp) if bk >= 0 else 0.0
    nb, dk, dr = int(out["n_inliers"][b]), int(out["best_hyp"][b, 0]), int(out["best_hyp"][b, 1])
    assert int(out["iters_run"][b]) == it, (b, out["iters_run"][b], it)
    assert float(out["min_median"][b]) == best and float(out["sigma"][b]) == sg, (b, out["min_median"][b], best, out["sigma"][b], sg)
    M = out[name][b].astype(np.float64)
    mask = out["mask"][b]
    if bk < 0:
        assert (nb, dk, dr) == (0, -1, -1) and (M == 0).all() and (mask == 0).all(), b
    else:
        assert (dk, dr) == (bk, br) and nb >= mp, (b, (dk, dr), (bk, br), nb)  # the sample's own points fit its model: always >= m

    # 2b. the rule over the restatement's table.  An iteration that was not compared is left out on both sides when neither side
    #     would take it (all its medians above that side's minimum); otherwise the pair is ambiguous.
    med_c, bnd_c = med.copy(), bnd.copy()
    lost = True
    for k in skipped:
        med_c[k], bnd_c[k] = ref.NO_ROOT, 0.0
    rbest, rk, rr, rit = ref.select(med_c, niters)
    for k in skipped:
        if k < rit:
            lost &= all(v > rbest for v in med[k] if v >= 0) and all(v > best for v in tab[k] if v >= 0)
    exact = lost and not ref.is_ambiguous(med_c, bnd_c, niters)
    assert rit == it, (b, rit, it)  # where the loop ends depends on the samples alone
    if exact:
        assert dk == rk, (b, dk, rk)
        if rk >= 0:
            assert abs(best - rbest) <= bnd_c[rk, rr], (b, best, rbest, bnd_c[rk, rr])

    # 3. the winner: the restatement root of iteration best_hyp[0] nearest to it, to 1e-5 in unit() (an ambiguous pair's winner
    #    is the implementation's, often a badly conditioned sample: only its table is checked)
    if bk >= 0 and exact:
        cand = models[dk]
        assert cand, (b, dk)
        dist = [np.linalg.norm(unit(M) - unit(Mr)) for Mr, _ in cand]
        j = int(np.argmin(dist))
        assert dist[j] < 1e-5, (b, dk, dist)
        Mw, dMw = cand[j]
        if not five and Mw[2, 2] == 1.0:
            assert M[2, 2] == 1.0, (b, M)
        # 4. the mask: err <= (float)sigma^2 of the device's sigma, outside the bound's band around it
        if dMw is not None:
            e = ref.e_errors(Mw, x) if five else ref.f_errors(Mw, x)
            thr = float(ref.bound32(float(out["sigma"][b])))
            sure = np.abs(np.where(np.isfinite(e), e, np.inf) - thr) > ref.error_bounds(Mw, dMw, x, five)
            assert ((mask == 1) == (ref.to_f32(e) <= np.float32(thr)))[sure].all(), b
    assert int(mask.sum()) == nb, b
    masked = out["masked"][b]
    nan_rows = np.isnan(masked).all(-1)
    assert (np.isnan(masked).any(-1) == nan_rows).all(), b
    assert (nan_rows == (mask == 0)).all(), b
    assert np.array_equal(masked[mask == 1].view(np.uint32), pts[mask == 1].view(np.uint32)), b
    verdict = "exact" if exact else "ambiguous"
    TALLY[verdict] += 1
    return verdict


# ---- the case matrix ------------------------------------------------------------------------------------------------------
NOISE_FREE = (0.0, 0.0)
# (id, N, scene kinds, max_iters, confidence, seed): one edge or rule branch per line; max_iters small where the edge is N
CASES_F = [
    ("N8", 8, [NOISE_FREE], 40, 0.99, 3),
    ("N9", 9, KINDS[1:2], 40, 0.99, 3),
    ("N14", 14, KINDS[:3], 300, 0.99, 0),
    ("N15", 15, KINDS[:3], 40, 0.99, 3),
    ("N63", 63, KINDS[:3], 33, 0.99, 0),
    ("N64", 64, KINDS[:3], 32, 0.99, 3),
    ("N65", 65, KINDS[:4], 31, 0.99, U64),
    ("N127", 127, KINDS[:2], 17, 0.99, 3),
    ("N128", 128, KINDS[1:3], 16, 0.99, 3),
    ("N129", 129, KINDS[:2], 15, 0.99, 3),
    ("N1000", 1000, KINDS[1:3], 33, 0.99, 3),
    ("N3864", 3864, KINDS[1:2], 17, 0.99, 3),   # 16 N + 3712 = 65536: the last N without the LDS attribute
    ("N3865", 3865, KINDS[1:2], 17, 0.99, 3),
    ("N4096", 4096, KINDS[1:3], 17, 0.99, U64),
    ("it1", 100, KINDS[:3], 1, 0.99, 3),
    ("it2", 100, KINDS[:2], 2, 0.99, 3),
    ("it63", 100, KINDS[:2], 63, 0.99, 0),
    ("it64", 100, KINDS[:2], 64, 0.99, 3),
    ("it65", 100, KINDS[:2], 65, 0.99, U64),
    ("it299", 50, KINDS[:2], 299, 0.99, 3),
    ("it300", 50, KINDS[:2], 300, 0.99, 3),
    ("it1000", 50, KINDS[:2], 1000, 0.99, 0),   # niters = 300 < max_iters
    ("p0", 100, KINDS[:2], 100, 0.0, 3),        # niters = 0: no model
    ("p1", 100, KINDS[:2], 70, 1.0, 3),         # niters = max_iters
]
CASES_E = [
    ("N6", 6, KINDS[1:2], 20, 0.999, 3),
    ("N10", 10, KINDS[:2], 20, 0.999, 3),       # the first N whose median is not among the sample's own errors
    ("N63", 63, KINDS[:2], 17, 0.999, 0),
    ("N64", 64, KINDS[:2], 16, 0.999, 3),
    ("N65", 65, KINDS[:2], 15, 0.999, U64),
    ("N129", 129, KINDS[:2], 17, 0.999, 3),
    ("N1684", 1684, KINDS[1:2], 17, 0.999, 3),  # 16 N + 38592 = 65536
    ("N1685", 1685, KINDS[1:2], 17, 0.999, 3),
    ("N4096", 4096, KINDS[1:2], 17, 0.999, 3),
    ("it1", 100, KINDS[:2], 1, 0.999, 3),
    ("it65", 100, KINDS[:2], 65, 0.999, 0),
    ("it1000", 50, KINDS[:2], 1000, 0.999, 3),  # niters < max_iters
    ("p0", 100, KINDS[:2], 50, 0.0, 3),
    ("p1", 100, KINDS[:2], 33, 1.0, 3),
]


def case_pairs(dfepe, name, kinds, N):
    return _pairs(dfepe, kinds, N, sum(map(ord, name)))


@pytest.mark.parametrize("case", CASES_F, ids=[c[0] for c in CASES_F])
def test_fundamental_case_matrix_against_the_restatement(dfepe, case):
    name, N, kinds, max_iters, confidence, seed = case
    m = case_pairs(dfepe, name, kinds, N)
    out = run(dfepe, m, confidence, max_iters, seed)
    verdicts = [check_pair(m, out, b, confidence, seed, max_iters) for b in range(m.shape[0])]
    print(f"[lmeds] F {name}: {verdicts}")
    niters = ref.num_iters(7, confidence, max_iters)
    assert niters == {"it299": 299, "it300": 300, "it1000": 300, "p0": 0, "p1": 70}.get(name, min(max_iters, 300))
    assert (out["iters_run"] == niters).all()
    if name == "p0":
        assert (out["n_inliers"] == 0).all() and (out["min_median"] == ref.DBL_MAX).all()
    if name == "N8":
        assert float(out["sigma"][0]) == 0.001 and int(out["n_inliers"][0]) >= 7  # the noise-free pair hits the floor


@pytest.mark.parametrize("case", CASES_E, ids=[c[0] for c in CASES_E])
def test_essential_case_matrix_against_the_restatement(dfepe, case):
    name, N, kinds, max_iters, confidence, seed = case
    m = case_pairs(dfepe, "E" + name, kinds, N)
    out = run(dfepe, m, confidence, max_iters, seed, K=KITTI_K)
    verdicts = [check_pair(m, out, b, confidence, seed, max_iters, K=KITTI_K) for b in range(m.shape[0])]
    print(f"[lmeds] E {name}: {verdicts}")
    assert (out["iters_run"] == ref.num_iters(5, confidence, max_iters)).all()
    if name == "p0":
        assert (out["n_inliers"] == 0).all()


def test_median_inside_a_run_of_equal_errors(dfepe):
    base = case_pairs(dfepe, "dup", [(0.0, 0.5)], 11)[0]
    m = np.tile(base, (4, 1))[None]  # 44 correspondences: every one four times; ranks 20..23 are one value, the median's 21 and 22 too
    out = run(dfepe, m, 0.99, 40, 3)
    check_pair(m, out, 0, 0.99, 3, 40)
    tab = out["hyp_medians"][0]
    e = [ref.to_f32(ref.f_errors(F, m[0])) for row in ref.models_f(m[0], 3, 40) if row for F, _ in row]
    assert all(np.sort(x)[21] == np.sort(x)[22] for x in e) and (tab >= 0).any()


def test_sampler_failure_after_the_first_iteration_ends_the_loop(dfepe):
    # the six-locations construction of test_ransac_edges_gpu.py: iteration 0 has a sample, iteration 1 has none
    g = np.random.default_rng(0)
    locs = g.uniform(50, 900, (7, 2))
    x1 = np.r_[np.repeat(locs[:6], 25, 0), locs[6:]]
    m = np.c_[x1, g.uniform(0, 1000, (151, 2))].astype(np.float32)[None]
    seed, max_iters = 1, 8
    models = ref.models_f(m[0], seed, max_iters)
    assert models[0] is not None and models[1] is None and any(r is not None for r in models[2:])
    out = run(dfepe, m, 0.99, max_iters, seed)
    assert int(out["iters_run"][0]) == 1 and int(out["best_hyp"][0, 0]) == 0
    assert (out["hyp_medians"][0][2:] != ref.NO_SAMPLE).any()  # the table holds the later iterations; the rule does not read them
    check_pair(m, out, 0, 0.99, seed, max_iters, models=models)


def test_all_collinear_pair_has_no_model(dfepe):
    g = np.random.default_rng(1)
    t = g.permutation(1000)[:30].astype(np.float64)  # integers: the line is exact in fp32 and every cross product is exactly 0
    m = np.c_[t, 2.0 * t + 10.0, g.uniform(0, 1000, (30, 2))].astype(np.float32)[None]  # image 1 on one line: no sample at k = 0
    out = run(dfepe, m, 0.99, 3, 0)
    assert (out["hyp_medians"][0] == ref.NO_SAMPLE).all()
    assert int(out["iters_run"][0]) == 0 and int(out["n_inliers"][0]) == 0 and (out["best_hyp"][0] == -1).all()
    assert (out["F"][0] == 0).all() and (out["mask"][0] == 0).all() and np.isnan(out["masked"][0]).all()
    assert float(out["min_median"][0]) == ref.DBL_MAX and float(out["sigma"][0]) == 0.0


def _same(a, b, rows_a=None, rows_b=None):
    for k in a:
        x, y = (_bits(t).reshape(t.shape[0], -1) for t in (a[k], b[k]))  # rows of bytes: one per pair
        x = x if rows_a is None else x[rows_a]
        y = y if rows_b is None else y[rows_b]
        assert torch.equal(x, y), k


@pytest.mark.parametrize("five", [False, True], ids=["F", "E"])
def test_deterministic_and_batch_invariant(dfepe, five):
    N = 14 if not five else 50
    m = torch.from_numpy(_pairs(dfepe, [KINDS[i % 3] for i in range(64)], N, 11)).to(DEV)
    K = torch.from_numpy(KITTI_K.astype(np.float32)).to(DEV).expand(64, 3, 3).contiguous()
    kw = dict(max_iters=100, seed=9, want_hyp_medians=True, want_masked=True)
    call = (lambda mm, KK: dfepe.ops.lmeds_essential(mm, KK, **kw)) if five else (lambda mm, KK: dfepe.ops.lmeds_fundamental(mm, **kw))
    a, b, c = call(m, K), call(m, K), call(m[17:18].contiguous(), K[:1])
    torch.cuda.synchronize()
    _same(a, b)
    _same(a, c, slice(17, 18), slice(0, 1))


@pytest.mark.parametrize("B,N,max_iters", [(4096, 14, 1000), (65535, 8, 2)], ids=["4096x14", "65535x8"])
def test_large_batch_is_permutation_equivariant_and_matches_the_restatement(dfepe, B, N, max_iters):
    sc = dfepe.synth.make_scene(B, N, seed=B + N, outlier_ratio=0.3, noise_px=0.5)
    m = sc["matches_xy_ori"].numpy()
    g = np.random.default_rng(B)
    perm = g.permutation(B)
    md = torch.from_numpy(m).to(DEV)
    kw = dict(max_iters=max_iters, seed=5, want_hyp_medians=True, want_masked=True)
    a = dfepe.ops.lmeds_fundamental(md, **kw)
    p = dfepe.ops.lmeds_fundamental(md[torch.from_numpy(perm).to(DEV)].contiguous(), **kw)
    torch.cuda.synchronize()
    _same(a, p, torch.from_numpy(perm), None)
    out = _np(a)
    for b in g.choice(B, 4 if N >= 14 else 2, replace=False):
        check_pair(m, out, int(b), 0.99, 5, max_iters)


def test_seed_minus_one_is_the_top_64_bit_seed(dfepe):
    m = torch.from_numpy(_pairs(dfepe, KINDS[:3], 14, 7)).to(DEV)
    kw = dict(max_iters=40, want_hyp_medians=True, want_masked=True)
    a = dfepe.ops.lmeds_fundamental(m, seed=-1, **kw)
    b = dfepe.ops.lmeds_fundamental(m, seed=U64, **kw)
    c = dfepe.ops.lmeds_fundamental(m, seed=(1 << 63) - 1, **kw)
    torch.cuda.synchronize()
    _same(a, b)
    assert not torch.equal(a["hyp_medians"], c["hyp_medians"])


@pytest.mark.parametrize("five", [False, True], ids=["lmeds_pose", "lmeds_essential_pose"])
def test_pose_step_is_the_unchanged_cheirality_on_the_masked_matches(dfepe, five):
    sc = dfepe.synth.make_scene(6, 14, seed=21, outlier_ratio=0.2, noise_px=0.5)
    m, K = sc["matches_xy_ori"].to(DEV), sc["Ks"].to(DEV)
    uo = dfepe.compat.utils_opencv
    Kp = uo.recover_pose_camera(K)
    out = dfepe.ops.lmeds_essential_pose(m, K) if five else dfepe.ops.lmeds_pose(m, K, K_pose=Kp)
    _, win, cnt = dfepe.ops.cheirality(out["E"], Kp, out["masked"], 50.0, fp64_only=True)
    torch.cuda.synchronize()
    assert torch.equal(win, out["winner"]) and torch.equal(cnt, out["counts"])
    o = _np(out)
    assert (o["n_inliers"] >= (5 if five else 7)).all()
    for b in range(6):
        w = int(o["winner"][b])
        assert int(o["in_front"][b].sum()) == (int(o["counts"][b, w]) if w >= 0 else 0)
        assert not (o["in_front"][b].astype(bool) & (o["mask"][b] == 0)).any()


# ---- compat ---------------------------------------------------------------------------------------------------------------
def _compat_scene(dfepe, N):
    sc = dfepe.synth.make_scene(1, N, seed=33, outlier_ratio=0.0, noise_px=0.05)
    return sc, sc["matches_xy_ori"][0].numpy(), sc["Ks"][0].double().numpy()


def test_recover_camera_opencv_takes_lmeds_below_15_correspondences(dfepe):
    uo = dfepe.compat.utils_opencv
    sc, m, K = _compat_scene(dfepe, 14)
    gt_inv = np.linalg.inv(sc["delta_Rtijs_4_4"][0].double().numpy())
    M, err, mask2, (E, F) = uo.recover_camera_opencv(K, m[:, :2], m[:, 2:], gt_inv, show_result=False)
    assert M.shape == (3, 4) and mask2.shape == (14,) and mask2.dtype == bool and E.shape == (3, 3) and F.shape == (3, 3)
    assert mask2.any() and err[0] < 1.0, err  # 0.05 px of noise, no outliers: the rotation is recovered to below a degree
    M2, err2, mask22, (E2, F2) = uo.recover_camera_lmeds(K, m[:, :2], m[:, 2:], gt_inv, show_result=False)
    assert np.array_equal(M, M2) and err == err2 and np.array_equal(mask2, mask22) and np.array_equal(F, F2) and np.array_equal(E, E2)
    M5, err5, mask5, E5 = uo.recover_camera_lmeds(K, m[:, :2], m[:, 2:], gt_inv, five_point=True, show_result=False)
    assert M5.shape == (3, 4) and mask5.shape == (14,) and E5.shape == (3, 3) and abs(np.linalg.norm(E5) - 1.0) < 1e-6
    with pytest.raises(dfepe._lib.DfepeError):  # 7 correspondences: OpenCV's direct 7-point path is still not built
        uo.recover_camera_opencv(K, m[:7, :2], m[:7, 2:], gt_inv, show_result=False)
    with pytest.raises(NotImplementedError):
        uo.recover_camera_opencv(K, m[:, :2], m[:, 2:], gt_inv, five_point=True, show_result=False)
    with pytest.raises(dfepe._lib.DfepeError, match="LMedS"):
        dfepe.ops.ransac_fundamental(torch.from_numpy(m[None]).to(DEV))
    with pytest.raises(dfepe._lib.DfepeError, match="at least 8"):
        dfepe.ops.lmeds_fundamental(torch.from_numpy(m[None, :7]).to(DEV))


@pytest.mark.parametrize("baseline,tag,key", [("lmeds", "_lmeds", "lmeds_8p"), ("lmeds_five_point", "_lmeds5p", "lmeds_5p")])
def test_validation_summary_accepts_the_lmeds_baselines(dfepe, baseline, tag, key):
    tg = dfepe.compat.train_good_utils
    sc = dfepe.synth.make_scene(4, 14, seed=41, outlier_ratio=0.0, noise_px=0.05)
    d = {k: sc[k].to(DEV) for k in ("Ks", "matches_xy_ori", "E_gt", "F_gt", "delta_Rtijs_4_4")}
    summary, pairs = tg.validation_summary(d["Ks"], d["matches_xy_ori"], d["E_gt"], d["F_gt"], d["F_gt"], d["delta_Rtijs_4_4"], baseline=baseline)
    torch.cuda.synchronize()
    assert key in summary
    for k in ("err_R_deg", "err_t_deg", "Rt_cam", "winner", "E", "F", "inlier_mask", "epi_dists"):
        assert k + tag in pairs, k
    assert pairs["F" + tag].shape == (4, 3, 3) and pairs["inlier_mask" + tag].shape == (4, 14)
    assert float(pairs["err_R_deg" + tag].median()) < 1.0


def test_module_compared_most_pairs_exactly():
    """Runs last in the module: at most 1 pair in 8 may fall in the ambiguous class."""
    n = TALLY["exact"] + TALLY["ambiguous"]
    print(f"[lmeds] module: {n} pairs, {TALLY['exact']} compared exactly, {TALLY['ambiguous']} ambiguous")
    if n:
        assert TALLY["ambiguous"] <= n / 8
