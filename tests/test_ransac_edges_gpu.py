"""The batched RANSAC estimator (csrc/ransac.hip) at its launch edges, against the fp64 restatement of tests/ransac_ref.py.

Every device result goes through one comparison (check_pair): the count table per iteration as multisets (the device's null-space
basis comes from a Householder QR, the restatement's from an SVD, so the order of the roots within an iteration is the
implementation's), the selection rule run on the restatement's own table, the winner as the restatement root whose count is the
device's n_inliers, the inlier mask and the NaN-masked copy, and the same call with the table in the workspace.  The cases sit on
the edges of the launches: the 64-lane sweep and 256-lane mask tails, the 64-iteration chunks of the count grid and windows of the
select kernel, 4 pairs per select workgroup, the LDS attribute path (N >= 3169), kMaxN, kMaxPairs, and the branches of the rule
(a sample missing after k = 0, confidence 0 and 1, 64-bit seeds).  The in-front mask of the pose step is held to a
per-correspondence triangulation (oracle.triangulate_dlt) of the pose the device reports."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_ref as ref  # noqa: E402
from cheirality_cases import scaled_y as _scaled_y  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAND = 1e-4   # relative band around t^2 inside which a decision may differ from the fp64 restatement (as test_ransac_gpu.py)
U64 = (1 << 64) - 1
TALLY = {"exact": 0, "ambiguous": 0}  # pairs of this module compared exactly / falling in the ambiguous class


def unit(F):
    f = np.asarray(F, np.float64).ravel()
    f = f / np.linalg.norm(f)
    return f * np.sign(f[np.argmax(np.abs(f))])


def _bits(x):
    x = x.detach().cpu().contiguous()
    return x.view(torch.uint8) if x.is_floating_point() else x


def _np(out):
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}


# ---- scenes ---------------------------------------------------------------------------------------------------------------
# a kind: (outlier ratio, noise px) of synth.make_scene, or "noise": uniform matches (many small models, the whole table read)
KINDS = [(0.0, 0.05), (0.3, 0.5), (0.6, 0.5), "noise", (0.3, 0.05), (0.0, 0.5), (0.6, 0.05)]


def _pairs(dfepe, kinds, N, seed):
    rows = []
    for i, kd in enumerate(kinds):
        if kd == "noise":
            g = np.random.default_rng(seed * 1000 + i)
            rows.append(np.c_[g.uniform(0, 1241, (N, 1)), g.uniform(0, 376, (N, 1)), g.uniform(0, 1241, (N, 1)),
                              g.uniform(0, 376, (N, 1))].astype(np.float32))
        else:
            sc = dfepe.synth.make_scene(1, N, seed=seed * 1000 + i, outlier_ratio=kd[0], noise_px=kd[1])
            rows.append(sc["matches_xy_ori"][0].numpy())
    return np.stack(rows)


# ---- the device call ------------------------------------------------------------------------------------------------------
def run(dfepe, m, threshold, confidence, max_iters, seed):
    """Device result with the table and the NaN-masked copy; the same call with the table in the workspace must give bit-identical
    outputs."""
    md = torch.from_numpy(np.ascontiguousarray(m)).to(DEV)
    kw = dict(threshold=threshold, confidence=confidence, max_iters=max_iters, seed=seed)
    out = dfepe.ops.ransac_fundamental(md, want_hyp_counts=True, want_masked=True, **kw)
    ws = dfepe.ops.ransac_fundamental(md, want_masked=True, **kw)
    torch.cuda.synchronize()
    assert ws["hyp_counts"] is None
    for k in ("F", "mask", "n_inliers", "iters_run", "best_hyp", "masked"):
        assert torch.equal(_bits(out[k]), _bits(ws[k])), k
    return _np(out)


# ---- the comparison -------------------------------------------------------------------------------------------------------
def _rule_is_decided(ref_tab, bands, N, confidence, max_iters):
    """True when no entry the sequential rule reads up to its stop can change its (best count, winning iteration, iterations).
    ref_tab [max_iters, 3]: the restatement's counts; bands [max_iters, 3]: correspondences within BAND t^2 of t^2 for each root,
    -1 for every root of an iteration whose number of roots differs from the device's.

    How one iteration moves the rule's state (best, niters, last iteration taken) depends on the multiset of its counts only:
    best becomes the largest count above max(best, 6), and the chain of RANSACUpdateNumIters calls collapses to
    min(niters, rint(log(1 - p) / log(1 - (1 - ep)^7))) of that largest count (the value is monotone in the count), so the double
    update of two roots taken in one iteration gives what a single update of the larger one gives, in either order: root order
    alone cannot make the two sides differ.  A root whose count may be off by its band (the device's root of the same sample
    decides differently only inside it) changes nothing while its count plus its band stays at or below both the threshold the
    iteration starts with and the largest count of the iteration that has no band: it is then never the largest count above the
    threshold, on either side.  Otherwise (a band that could matter, or a different number of roots) the pair is ambiguous."""
    best, niters, k = 0, max_iters, 0
    while k < niters:
        if ref_tab[k][0] == ref.NO_SAMPLE:
            break
        if (bands[k] < 0).any():
            return False
        thr = max(best, 6)
        sure = max([thr] + [int(c) for c, bd in zip(ref_tab[k], bands[k]) if c >= 0 and bd == 0])
        if any(c >= 0 and bd > 0 and c + bd > sure for c, bd in zip(ref_tab[k], bands[k])):
            return False
        for r in range(3):
            c = int(ref_tab[k][r])
            if c > max(best, 6):
                best = c
                niters = ref.update_num_iters(confidence, (N - c) / N, niters)
        k += 1
    return True


def check_pair(m, out, b, threshold, confidence, seed, max_iters, hyps=None):
    """The device result of pair b against the restatement.  Returns ("exact" | "ambiguous", iterations whose counts were
    compared root for root)."""
    pts = m[b]
    N = pts.shape[0]
    t2 = threshold * threshold
    if hyps is None:
        hyps = ref.hypotheses(pts, seed, max_iters)
    tab = out["hyp_counts"][b]
    assert tab.shape == (max_iters, 3)

    # 1. the table, iteration by iteration, as multisets of counts
    ref_tab = np.full((max_iters, 3), ref.NO_ROOT, np.int64)
    bands = np.zeros((max_iters, 3), np.int64)  # per root: correspondences within BAND t^2 of t^2; -1: the number of roots differs
    n_rootdiff = 0
    with np.errstate(divide="ignore", invalid="ignore"):
        for k, (idx, Fs) in enumerate(hyps):
            row = tab[k]
            if idx is None:
                assert (row == ref.NO_SAMPLE).all(), (b, k, row)
                ref_tab[k] = ref.NO_SAMPLE
                continue
            assert (row != ref.NO_SAMPLE).all(), (b, k, row)
            dev = sorted(int(c) for c in row if c >= 0)
            assert (row[len(dev):] == ref.NO_ROOT).all(), (b, k, row)  # roots first, absent ones after
            e = [ref.errors(F, pts) for F in Fs]
            cnt = [int((x <= t2).sum()) for x in e]
            ref_tab[k, :len(cnt)] = cnt
            bands[k, :len(e)] = [int((np.abs(x - t2) <= BAND * t2).sum()) for x in e]
            if len(dev) != len(Fs):
                n_rootdiff += 1
                bands[k] = -1
                continue
            band = int(bands[k].max())
            assert all(abs(a - c) <= band for a, c in zip(dev, sorted(cnt))), (b, k, dev, sorted(cnt), band)
    assert n_rootdiff <= 0.001 * max_iters + 1, (b, n_rootdiff)

    nb, dk, dr, it = int(out["n_inliers"][b]), int(out["best_hyp"][b, 0]), int(out["best_hyp"][b, 1]), int(out["iters_run"][b])
    # 2a. the rule over the device's own table gives the device's outputs, the root index included
    assert ref.select(tab, N, confidence, max_iters) == (nb, dk, dr, it), b
    # 2b. the rule over the restatement's table: best count, winning iteration and iterations consumed do not depend on the order
    #     of the roots within an iteration (see _rule_is_decided), so they must agree exactly unless an entry it reads is ambiguous
    best, bk, _, iters = ref.select(ref_tab, N, confidence, max_iters)
    exact = _rule_is_decided(ref_tab, bands, N, confidence, max_iters)
    if exact:
        assert (nb, dk, it) == (best, bk, iters), (b, (nb, dk, it), (best, bk, iters))

    # 3. the winner: the restatement root of iteration best_hyp[0] whose count is n_inliers
    F = out["F"][b].astype(np.float64)
    mask = out["mask"][b]
    if nb == 0:
        assert (dk, dr) == (-1, -1) and (F == 0).all() and (mask == 0).all(), b
        Fw = None
    else:
        assert nb > 6 and 0 <= dk < max_iters and 0 <= dr < 3, (b, nb, dk, dr)
        idx, Fs = hyps[dk]
        assert idx is not None and Fs, (b, dk)
        if exact:
            cand = [Fr for Fr, c in zip(Fs, ref_tab[dk]) if int(c) == nb]
        elif (bands[dk] < 0).any():
            cand = list(Fs)
        else:
            cand = [Fr for Fr, c, bd in zip(Fs, ref_tab[dk], bands[dk]) if abs(int(c) - nb) <= bd]
        assert cand, (b, dk, nb, ref_tab[dk])
        dist = [np.linalg.norm(unit(F) - unit(Fr)) for Fr in cand]
        Fw = cand[int(np.argmin(dist))]
        assert min(dist) < 1e-5, (b, dk, dist)
        if Fw[2, 2] == 1.0:
            assert F[2, 2] == 1.0, (b, F)

    # 4. the mask: the winner's inlier test outside the band (the mask kernel works from the fp64 winner, so the fp64 restatement
    #    root stands for it: the fp32 F output would move errors near t^2 at t = 0.1 px by more than the band), its row sum, and the
    #    NaN-masked copy: NaN rows exactly where the mask is 0, every other row bit-identical to the input
    if Fw is not None:
        with np.errstate(divide="ignore", invalid="ignore"):
            e = ref.errors(Fw, pts)
        sure = np.abs(e - t2) > BAND * t2
        assert ((mask == 1) == (e <= t2))[sure].all(), b
    assert int(mask.sum()) == nb, b
    masked = out["masked"][b]
    nan_rows = np.isnan(masked).all(-1)
    assert (np.isnan(masked).any(-1) == nan_rows).all(), b
    assert (nan_rows == (mask == 0)).all(), b
    assert np.array_equal(masked[mask == 1].view(np.uint32), pts[mask == 1].view(np.uint32)), b

    verdict = "exact" if exact else "ambiguous"
    TALLY[verdict] += 1
    return verdict, int(((bands[:, 0] >= 0) & (ref_tab[:, 0] != ref.NO_SAMPLE)).sum())


def _report(name, verdicts):
    ne = sum(v == "exact" for v in verdicts)
    print(f"[ransac edges] {name}: {len(verdicts)} pairs, {ne} compared exactly, {len(verdicts) - ne} ambiguous")
    return ne


# ---- the case matrix ------------------------------------------------------------------------------------------------------
# (id, N, scene kinds, max_iters, threshold, confidence, seed): a deliberate list, one edge or rule branch per line
CASES = [
    # N: minimum, sweep tails (64 lanes), mask tails (256 lanes), 64 KiB of LDS exactly (16 N + 14848 = 65536), the first N on the
    # hipFuncSetAttribute path, kMaxN.  max_iters small where the edge is N.
    ("N15", 15, KINDS[:3], 129, 1.0, 0.99, 3),
    ("N16", 16, KINDS[1:2], 65, 1.0, 0.99, 3),
    ("N63", 63, KINDS[:5], 65, 1.0, 0.99, 0),
    ("N64", 64, KINDS[1:2], 64, 1.0, 0.99, 3),
    ("N65", 65, KINDS[:7], 63, 1.0, 0.99, U64),
    ("N255", 255, KINDS[:3], 65, 1.0, 0.99, 3),
    ("N256", 256, KINDS[2:3], 64, 3.0, 0.99, 0),
    ("N257", 257, KINDS[:5], 129, 1.0, 0.99, 3),
    ("N1000", 1000, KINDS[1:2], 65, 1.0, 0.99, 3),
    ("N3168", 3168, KINDS[1:2], 65, 1.0, 0.99, 3),
    ("N3169", 3169, KINDS[:3], 65, 1.0, 0.99, 3),
    ("N4096", 4096, KINDS[1:4], 129, 1.0, 0.99, U64),
    # max_iters around the count grid's 64-iteration chunks and the select kernel's 64-iteration windows; confidence 1 (niters
    # never shrinks: the whole table is read) and 0 (the first model sets niters = 0) on the way
    ("it1", 200, KINDS[:5], 1, 1.0, 0.99, 3),
    ("it2", 200, KINDS[:3], 2, 1.0, 1.0, 3),
    ("it63", 200, KINDS[:7], 63, 1.0, 1.0, 0),
    ("it64", 300, KINDS[:3], 64, 1.0, 0.5, 3),
    ("it65", 300, KINDS[:5], 65, 1.0, 1.0, U64),
    ("it128", 300, KINDS[:3], 128, 1.0, 0.0, 3),
    ("it129", 300, KINDS[:7], 129, 1.0, 1.0, 3),
    ("it1000", 300, KINDS[2:5], 1000, 1.0, 0.5, 0),
    # thresholds at the validation's 1000 iterations: 0.1 px (the validation's: every pair reads the whole table), 1 px, 3 px
    # (early stop after a few models)
    ("t0.1", 1000, [(0.3, 0.05), (0.0, 0.05), (0.6, 0.05)], 1000, 0.1, 0.99, 0),
    ("t1", 1000, KINDS[:3], 1000, 1.0, 0.99, U64),
    ("t3", 1000, KINDS[:3], 1000, 3.0, 0.99, 3),
    # confidence: 0 (niters -> 0 after the first model: the remaining roots of that iteration still count), 0.5, 1 (never shrinks)
    ("p0", 500, KINDS[:7], 200, 1.0, 0.0, 3),
    ("p0-noise", 300, ["noise", "noise", "noise"], 64, 3.0, 0.0, 0),
    ("p0.5", 500, KINDS[:5], 300, 1.0, 0.5, U64),
    ("p1", 500, KINDS[:3], 300, 3.0, 1.0, 0),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_case_matrix_against_the_restatement(dfepe, case):
    name, N, kinds, max_iters, threshold, confidence, seed = case
    m = _pairs(dfepe, kinds, N, sum(map(ord, name)))
    out = run(dfepe, m, threshold, confidence, max_iters, seed)
    verdicts = [check_pair(m, out, b, threshold, confidence, seed, max_iters)[0] for b in range(m.shape[0])]
    _report(name, verdicts)


def test_seed_minus_one_is_the_top_64_bit_seed(dfepe):
    m = torch.from_numpy(_pairs(dfepe, KINDS[:3], 300, 7)).to(DEV)
    kw = dict(threshold=1.0, max_iters=129, want_hyp_counts=True, want_masked=True)
    a = dfepe.ops.ransac_fundamental(m, seed=-1, **kw)
    b = dfepe.ops.ransac_fundamental(m, seed=U64, **kw)
    c = dfepe.ops.ransac_fundamental(m, seed=(1 << 63) - 1, **kw)  # differs from 2^64 - 1 only in the top bit
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
    assert not torch.equal(a["hyp_counts"], c["hyp_counts"])


def test_sampler_failure_after_the_first_iteration_ends_the_loop(dfepe):
    # image 1: six locations 25 times each and one single point.  A sample of 7 distinct indices that repeats a location fails the
    # collinearity test, so a sample needs the single point and one point of every location: about half the iterations find one
    # within the 1000 attempts.
    g = np.random.default_rng(0)
    locs = g.uniform(50, 900, (7, 2))
    x1 = np.r_[np.repeat(locs[:6], 25, 0), locs[6:]]
    m = np.c_[x1, g.uniform(0, 1000, (151, 2))].astype(np.float32)[None]
    seed, max_iters = 1, 8
    hyps = ref.hypotheses(m[0], seed, max_iters)
    assert hyps[0][0] is not None and hyps[1][0] is None  # the precondition: iteration 0 has a sample, iteration 1 none
    assert any(h[0] is not None for h in hyps[2:])        # and later ones have again: the device table holds them, the rule stops
    out = run(dfepe, m, 1.0, 0.99, max_iters, seed)
    assert int(out["iters_run"][0]) == 1
    assert check_pair(m, out, 0, 1.0, 0.99, seed, max_iters, hyps)[0] == "exact"
    assert int(out["best_hyp"][0, 0]) == 0 and int(out["n_inliers"][0]) >= 7  # the sample's own seven fit its model exactly


# ---- large batches: permutation, and a sample of pairs through the comparison ---------------------------------------------
@pytest.mark.parametrize("B,N,max_iters,threshold", [(4096, 100, 1000, 0.1), (65535, 15, 2, 1.0)], ids=["4096x100", "65535x15"])
def test_large_batch_is_permutation_equivariant_and_matches_the_restatement(dfepe, B, N, max_iters, threshold):
    sc = dfepe.synth.make_scene(B, N, seed=B + N, outlier_ratio=0.3, noise_px=0.5)  # the pairs DESIGN 3.8 times
    m = sc["matches_xy_ori"].numpy()
    g = np.random.default_rng(B)
    perm = g.permutation(B)
    md = torch.from_numpy(m).to(DEV)
    kw = dict(threshold=threshold, max_iters=max_iters, seed=5, want_hyp_counts=True, want_masked=True)
    a = dfepe.ops.ransac_fundamental(md, **kw)
    p = dfepe.ops.ransac_fundamental(md[torch.from_numpy(perm).to(DEV)].contiguous(), **kw)
    torch.cuda.synchronize()
    pi = torch.from_numpy(perm)
    for k in a:
        assert torch.equal(_bits(a[k])[pi], _bits(p[k])), k
    out = _np(a)
    assert (out["iters_run"] <= max_iters).all()
    if threshold < 1:
        assert (out["iters_run"] == max_iters).all()  # 0.1 px on 0.5 px noise: no pair stops early, the select kernel reads it all
    picks = g.choice(B, 16, replace=False)
    verdicts = [check_pair(m, out, int(b), threshold, 0.99, 5, max_iters)[0] for b in picks]
    ne = _report(f"{B}x{N}", verdicts)
    assert ne >= 0.9 * len(verdicts)


# ---- the in-front mask against a per-correspondence triangulation ---------------------------------------------------------
def _candidates(E):
    """The four poses of E in fp64 (numpy SVD; the order follows its sign gauge, so the device's pose is found by value)."""
    U, _, Vt = np.linalg.svd(np.asarray(E, np.float64))
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    Rs = []
    for Wm in (W, W.T):
        R = U @ Wm @ Vt
        Rs.append(-R if np.linalg.det(R) < 0 else R)
    t = U[:, 2] / np.linalg.norm(U[:, 2])
    return [(R, s * t) for R in Rs for s in (1.0, -1.0)]


def check_in_front(oracle, E, Kp, m, Rt_cam, mask, depth_thres=50.0):
    """Device in-front mask [N] of one pair against triangulate_dlt in fp64.  m: the matches the device saw (NaN rows: 0).
    The pose is the device's Rt_cam (R = Rt_cam[:, :3]^T, t = -R Rt_cam[:, 3]); its fp32 rounding moves the depth of a
    low-parallax point by more than the band, so the fp64 pose of the device's fp32 E that Rt_cam rounds is used.
    Returns the number of correspondences decided (outside the band)."""
    Rc = np.asarray(Rt_cam, np.float64)
    Rd = Rc[:, :3].T
    td = -Rd @ Rc[:, 3]
    d = [np.linalg.norm(R - Rd) + np.linalg.norm(t - td) for R, t in _candidates(E)]
    assert min(d) < 1e-4, d
    R, t = _candidates(E)[int(np.argmin(d))]
    Kp = np.asarray(Kp, np.float64)
    P1 = Kp @ np.c_[np.eye(3), np.zeros(3)]
    P2 = Kp @ np.c_[R, t]
    m = np.asarray(m, np.float64)
    fin = np.isfinite(m).all(1)
    want = np.zeros(len(m), bool)
    sure = np.ones(len(m), bool)
    if fin.any():
        X = oracle.triangulate_dlt(P1, P2, m[fin, :2], m[fin, 2:])
        w = X[3]
        with np.errstate(divide="ignore", invalid="ignore"):
            z1 = X[2] / w
            z2 = (R[2] @ X[:3]) / w + t[2]
        want[fin] = (z1 > 0) & (z1 < depth_thres) & (z2 > 0) & (z2 < depth_thres)
        tol = 1e-6 * depth_thres
        near = (np.abs(w) <= 1e-9 * np.linalg.norm(X, axis=0))
        for z in (z1, z2):
            near |= (np.abs(z) <= tol) | (np.abs(z - depth_thres) <= tol)
        sure[fin] = ~near
    got = np.asarray(mask) == 1
    assert (got == want)[sure].all(), np.nonzero((got != want) & sure)[0][:10]
    return int(sure.sum())


@pytest.mark.parametrize("N,B,camera", [(15, 3, "K"), (63, 70, "pose_camera"), (64, 1, "identity"), (65, 3, "K"),
                                        (1000, 3, "pose_camera"), (4096, 1, "K")])
def test_ransac_pose_in_front_mask_against_triangulation(dfepe, oracle, N, B, camera):
    uo = dfepe.compat.utils_opencv
    sc = dfepe.synth.make_scene(B, N, seed=N + B, outlier_ratio=0.2, noise_px=0.5)
    m, K = _scaled_y(sc)
    md, Kd = m.to(DEV), K.to(DEV)
    Kp = {"K": None, "pose_camera": uo.recover_pose_camera(Kd), "identity": torch.eye(3, device=DEV).expand(B, 3, 3).contiguous()}[camera]
    out = dfepe.ops.ransac_pose(md, Kd, threshold=1.0, max_iters=200, seed=2, K_pose=Kp)
    torch.cuda.synchronize()
    o = _np(out)
    Kpn = (K if Kp is None else Kp.cpu()).double().numpy()
    if camera == "pose_camera":
        assert not np.allclose(Kpn, K.double().numpy())  # the pose camera differs from K (fy != fx)
    n_sure = n_all = 0
    for b in range(B):
        # E = K^T F K projected onto singular values (1, 1, 0), in fp64 from the fp32 F and K
        Kb = K[b].double().numpy()
        U, _, Vt = np.linalg.svd(Kb.T @ o["F"][b].astype(np.float64) @ Kb)
        E_ref = U @ np.diag([1.0, 1.0, 0.0]) @ Vt
        assert np.linalg.norm(o["E"][b] - E_ref) <= 1e-5 * np.linalg.norm(E_ref), b
        if int(o["winner"][b]) < 0:
            assert (o["in_front"][b] == 0).all()
            continue
        assert int(o["in_front"][b].sum()) == int(o["counts"][b, o["winner"][b]])
        n_sure += check_in_front(oracle, o["E"][b], Kpn[b], o["masked"][b], o["Rt_cam"][b], o["in_front"][b])
        n_all += N
        assert not (o["in_front"][b].astype(bool) & (o["mask"][b] == 0)).any()
    assert n_sure >= 0.99 * n_all


@pytest.mark.parametrize("N,normalized", [(15, False), (64, False), (1000, False), (4096, False), (1000, True)])
def test_recover_camera_opencv_e_given_in_front_mask_against_triangulation(dfepe, oracle, N, normalized):
    uo = dfepe.compat.utils_opencv
    sc = dfepe.synth.make_scene(1, N, seed=3 * N + normalized, outlier_ratio=0.2, noise_px=0.5)
    m, K = _scaled_y(sc)
    m, K = m[0].numpy(), K[0].double().numpy()
    E_given = sc["E_gt"][0].numpy()
    M, err, mask2, (E, F) = uo.recover_camera_opencv(K, m[:, :2], m[:, 2:], np.eye(4)[:3], E_given=E_given, show_result=False,
                                                     if_normalized=normalized)
    assert F is None and mask2.shape == (N,)
    assert np.array_equal(E, E_given.astype(np.float32).astype(np.float64))
    Kp = np.eye(3) if normalized else np.array([[K[0, 0], 0, K[0, 2]], [0, K[0, 0], K[1, 2]], [0, 0, 1.0]], np.float32).astype(np.float64)
    assert normalized or not np.allclose(Kp, K)
    if not mask2.any():
        assert err == uo.FAILED
        return
    R, t = M[:, :3], M[:, 3]  # scene motion: the camera is [R^T | -R^T t]
    Rt_cam = np.c_[R.T, -R.T @ t]
    n_sure = check_in_front(oracle, E, Kp, m, Rt_cam, mask2.astype(np.uint8))
    assert n_sure >= 0.99 * N


def test_module_compared_most_pairs_exactly():
    """Runs last in the module: how many pairs of the module fell in each class."""
    n = TALLY["exact"] + TALLY["ambiguous"]
    print(f"[ransac edges] module: {n} pairs, {TALLY['exact']} compared exactly, {TALLY['ambiguous']} ambiguous")
    if n:
        assert TALLY["exact"] >= 0.9 * n
