"""Shared inputs of the detector-evaluation tests and the one check() that the host build of csrc/detector_eval_math.h and the GPU
kernels both go through.  A job is a batch: kp1 [B,N1,C], kp2 [B,N2,C], H [B,3,3], n1, n2 ([B] or None), height, width, keep_k and
the thresholds; the restatement (tests/detector_eval_ref.py) is computed once per job and shared.

Held exactly: kept1, kept2, n_unwarped, count1, count2, the AP's integer counts, repeatability (one division of exact integers)
and the matching score.  Held within TOL times the restatement's bound: loc_err and the AP.  The seeded families are chosen so
that the restatement alone finds no decision (inside / outside, min <= thresh) within TOL bounds of its edge: check() asserts
that the undecided count is zero -- a condition on the inputs, not a tolerance.

The size edges: 1, 63, 64, 65 (a wavefront), 255, 256, 257 (a workgroup, the lanes of every kernel), 1023, 1024, 1025 (kTile of
csrc/detector_eval.hip: the LDS tile of the nearest-point sweep and of the rank count)."""
import functools

import numpy as np

import detector_eval_ref as dr

HEIGHT, WIDTH = 120, 160
EDGES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)


def homography(rng, scale=1.0):
    """A projective H near the identity: a few percent of shear and scale, a few pixels of shift, a perspective row that moves
    w by about a percent across the image."""
    a = rng.uniform(-0.04, 0.04, (2, 2)) * scale
    t = rng.uniform(-6.0, 6.0, 2) * scale
    p = rng.uniform(-6e-5, 6e-5, 2) * scale
    return np.array([[1 + a[0, 0], a[0, 1], t[0]], [a[1, 0], 1 + a[1, 1], t[1]], [p[0], p[1], 1.0]])


def seeded_pair(seed, n1, n2, C=3, levels=None, spill=0.12):
    """kp1 [n1,C], kp2 [n2,C], H: image-1 points uniform over the image and a margin of `spill` around it; the first image-2 points
    are image-1 points warped by H plus up to 4 px of noise (so that minima fall on both sides of the thresholds), the rest
    uniform.  Probabilities: a random permutation of distinct values, or drawn from `levels` equal values."""
    rng = np.random.default_rng(seed)
    H = homography(rng)
    lo, hi = np.array([-spill * WIDTH, -spill * HEIGHT]), np.array([(1 + spill) * WIDTH, (1 + spill) * HEIGHT])
    xy1 = rng.uniform(lo, hi, (n1, 2))
    m = min(n1, n2) * 2 // 3
    hom = np.concatenate([xy1[:m], np.ones((m, 1))], 1) @ H.T
    xy2 = np.concatenate([hom[:, :2] / hom[:, 2:] + rng.uniform(-4.0, 4.0, (m, 2)), rng.uniform(lo, hi, (n2 - m, 2))], 0)
    xy2 = xy2[rng.permutation(n2)]

    def prob(n):
        if levels is not None:
            return rng.choice(np.asarray(levels, np.float64), n)
        return (rng.permutation(n) + 1.0) / (n + 1.0)

    if C == 2:
        return xy1, xy2, H
    return np.concatenate([xy1, prob(n1)[:, None]], 1), np.concatenate([xy2, prob(n2)[:, None]], 1), H


def lattice_pair(shift):
    """Integer and half-integer coordinates under H = the translation by the integer `shift` (the identity for (0, 0)): every warp
    is exact, every distance the root of an exact multiple of 1/4.  Image-1 points sit on and around every edge of both inside
    rules (x = -1, 0, w - 1, w - 0.5, w and the same in y, in the warped frame); image-2 points stand at offsets (0, 3), (3, 4),
    (0, 0), (1, 1), (0, 6) and (5, 12) from warped image-1 points, so that minima of exactly 3 and exactly 5 meet the thresholds 3
    and 5 on their `<=` edge, and at the half-integer w - 0.5, which the half-open rule keeps and the closed rule drops."""
    sx, sy = shift
    H = np.array([[1.0, 0, sx], [0, 1.0, sy], [0, 0, 1.0]])
    w, h = float(WIDTH), float(HEIGHT)
    edge_x = [-1.0, 0.0, 1.0, w - 1, w - 0.5, w]
    edge_y = [-1.0, 0.0, 1.0, h - 1, h - 0.5, h]
    warped = [(x, y) for x in edge_x for y in edge_y]                           # where image-1 points land
    warped += [(20.0 + 25 * i, 30.0 + 20 * j) for i in range(5) for j in range(3)]  # interior anchors, far apart
    warped = np.array(warped)
    xy1 = warped - np.array([sx, sy], np.float64)
    offs = [(0, 3), (3, 4), (0, 0), (1, 1), (0, 6), (5, 12), (-3, 0), (4, -3), (2, 2), (0, 5), (-5, 0), (6, 8), (0, 4), (1, 0), (7, 0)]
    anchors = warped[-15:]
    xy2 = [tuple(a + np.array(o, np.float64)) for a, o in zip(anchors, offs)]
    # image-2 points are tested on their warp by adj(H) = the translation back: put them on the edges of the image-1 frame
    xy2 += [(x + sx, y + sy) for x in edge_x for y in (0.0, h - 0.5)] + [(5.0 + sx, y + sy) for y in edge_y]
    xy2 = np.array(xy2)
    p1 = (np.arange(len(xy1)) * 7 % len(xy1) + 1.0)
    p2 = (np.arange(len(xy2)) * 5 % len(xy2) + 1.0)
    return np.concatenate([xy1, p1[:, None]], 1), np.concatenate([xy2, p2[:, None]], 1), H


def _stack(pairs, n1=None, n2=None):
    """Pairs of equal C, padded with NaN rows to the longest (padding is past n1 / n2, which are then given)."""
    B = len(pairs)
    C = pairs[0][0].shape[1]
    N1, N2 = max(len(p[0]) for p in pairs), max(len(p[1]) for p in pairs)
    kp1, kp2 = np.full((B, N1, C), np.nan), np.full((B, N2, C), np.nan)
    for b, (a, c, _) in enumerate(pairs):
        kp1[b, :len(a)], kp2[b, :len(c)] = a, c
    ragged = any(len(p[0]) != N1 or len(p[1]) != N2 for p in pairs)
    if n1 is None and ragged:
        n1, n2 = [len(p[0]) for p in pairs], [len(p[1]) for p in pairs]
    H = np.stack([p[2] for p in pairs])
    return kp1, kp2, H, None if n1 is None else np.asarray(n1, np.int32), None if n2 is None else np.asarray(n2, np.int32)


def _job(name, pairs, keep_k, thresh, n1=None, n2=None, height=HEIGHT, width=WIDTH):
    kp1, kp2, H, n1, n2 = _stack(pairs, n1, n2)
    return {"name": name, "kp1": kp1, "kp2": kp2, "H": H, "n1": n1, "n2": n2, "height": height, "width": width, "keep_k": keep_k,
            "thresh": [float(t) for t in thresh]}


def _outside(seed, n):
    a, b, H = seeded_pair(seed, n, n)
    a[:, :2] += 10 * WIDTH
    b[:, :2] -= 10 * WIDTH
    return a, b, H


@functools.lru_cache(maxsize=None)
def jobs():
    """name -> job.  Built once."""
    out = []
    out.append(_job("lattice", [lattice_pair((0, 0)), lattice_pair((3, -2)), lattice_pair((-7, 11))], 300, (1, 3, 5, 13)))
    out.append(_job("lattice_k", [lattice_pair((0, 0))], 20, (3, 5)))
    out.append(_job("lattice_b1", [lattice_pair((2, 5))], 300, (3,)))
    out.append(_job("projective", [seeded_pair(11 + b, 70, 65) for b in range(3)], 300, (1, 3, 5)))
    out.append(_job("projective_k", [seeded_pair(21 + b, 70, 65) for b in range(3)], 25, (3,)))
    out.append(_job("ties", [seeded_pair(31 + b, 50, 60, levels=(0.1, 0.2, 0.3)) for b in range(3)], 20, (3,)))
    out.append(_job("ties_all_equal", [seeded_pair(35, 40, 40, levels=(0.5,))], 7, (3,)))
    out.append(_job("ties_signed_zero_nan_inf", [seeded_pair(36, 40, 40, levels=(0.0, -0.0, np.nan, np.inf, -np.inf, 1.0))], 11, (3,)))
    out.append(_job("two_columns", [seeded_pair(41 + b, 45, 50, C=2) for b in range(3)], 10, (3, 5)))
    for k in (0, 1, 29, 30, 31):
        # spill = -0.2: every point well inside the image and H close to the identity, so that all 30 are kept and k is about n
        pr = seeded_pair(50, 30, 30, spill=-0.2)
        out.append(_job(f"select_k{k}", [pr], k, (3,)))
    e2, e3 = np.zeros((0, 2)), np.zeros((0, 3))
    a, b, H = seeded_pair(61, 20, 20)
    out.append(_job("empty_1", [(e3, b, H)], 300, (3,)))
    out.append(_job("empty_2", [(a, e3, H)], 300, (3,)))
    out.append(_job("empty_both", [(e3, e3, H)], 300, (3,)))
    out.append(_job("empty_both_two_columns", [(e2, e2, H)], 300, (3,)))
    out.append(_job("outside", [_outside(62, 20), seeded_pair(63, 20, 20)], 300, (3,)))
    out.append(_job("no_thresholds", [seeded_pair(64, 20, 25)], 300, ()))
    out.append(_job("ragged", [seeded_pair(71 + b, 40, 40) for b in range(3)], 15, (3, 5), n1=[40, 17, 0], n2=[5, 40, 33]))
    out.append(_job("ragged_sizes", [seeded_pair(75, 64, 10), seeded_pair(76, 3, 65), seeded_pair(77, 30, 30)], 300, (3,)))
    for n in EDGES:
        out.append(_job(f"edge_{n}", [seeded_pair(100 + n, n, n)], max(n // 2, 1), (3,)))
    out.append(_job("edge_mixed", [seeded_pair(90, 257, 1025), seeded_pair(91, 1025, 63)], 300, (3,)))
    return {j["name"]: j for j in out}


def pair_inputs(job, b):
    n1 = job["kp1"].shape[1] if job["n1"] is None else int(np.clip(job["n1"][b], 0, job["kp1"].shape[1]))
    n2 = job["kp2"].shape[1] if job["n2"] is None else int(np.clip(job["n2"][b], 0, job["kp2"].shape[1]))
    return job["kp1"][b, :n1], job["kp2"][b, :n2], job["H"][b]


@functools.lru_cache(maxsize=None)
def ref(name):
    """The restatement of every pair of the job, computed once and left unchanged."""
    job = jobs()[name]
    out = []
    for b in range(len(job["H"])):
        a, c, H = pair_inputs(job, b)
        out.append(dr.repeatability_pair(a, c, H, job["height"], job["width"], job["keep_k"], job["thresh"]))
    return out


def check(got, name, b, what=""):
    """got: dict(kept1, kept2, n_unwarped: ints; count1, count2, repeatability, loc_err: [T]) of pair b of the job."""
    r = ref(name)[b]
    tag = f"{what} {name}[{b}]"
    assert r["undecided"] == 0, f"{tag}: the restatement leaves {r['undecided']} decisions undecided: pick another seed"
    for key in ("kept1", "kept2", "n_unwarped"):
        assert int(got[key]) == r[key], (tag, key, int(got[key]), r[key])
    T = len(jobs()[name]["thresh"])
    for key in ("count1", "count2"):
        assert np.array_equal(np.asarray(got[key]).reshape(T).astype(np.int64), r[key]), (tag, key, got[key], r[key])
    rep, loc = np.asarray(got["repeatability"], np.float64).reshape(T), np.asarray(got["loc_err"], np.float64).reshape(T)
    assert np.array_equal(rep, r["repeatability"]), (tag, rep, r["repeatability"])
    for t in range(T):
        if r["count1"][t] + r["count2"][t] == 0:
            assert rep[t] == 0.0 and loc[t] == -1.0, (tag, t, rep[t], loc[t])
        else:
            assert abs(loc[t] - r["loc_err"][t]) <= dr.TOL * r["loc_err_bound"][t], (tag, t, loc[t], r["loc_err"][t], r["loc_err_bound"][t])


# ---- average precision -----------------------------------------------------------------------------------------------------------
def ap_vector(seed, m, kind):
    """(labels [m] uint8, scores [m] float64).  kind: 'untied' distinct scores; 'tied' scores from five values; 'all_tied';
    'no_pos'; 'all_pos'."""
    rng = np.random.default_rng(seed)
    lab = (rng.uniform(size=m) < 0.4).astype(np.uint8)
    if kind in ("untied", "no_pos", "all_pos"):
        sc = rng.permutation(m) / max(m, 1) + 0.5 * lab * rng.uniform(size=m)  # positives tend to score higher
        sc = sc + np.arange(m) * 1e-9                                         # and no two scores are equal
    elif kind == "tied":
        sc = rng.choice(np.array([0.0, 0.25, 0.5, 0.75, 1.0]), m) + 0.25 * lab * (rng.uniform(size=m) < 0.5)
    else:
        sc = np.full(m, 0.7)
    if kind == "no_pos":
        lab[:] = 0
    if kind == "all_pos":
        lab[:] = 1
    return lab, np.asarray(sc, np.float64)


@functools.lru_cache(maxsize=None)
def ap_jobs():
    """name -> (labels [B,M] uint8, scores [B,M] float64, n_valid [B] or None)."""
    out = {}

    def add(name, vecs, n_valid=None):
        M = max(len(v[0]) for v in vecs)
        lab, sc = np.zeros((len(vecs), M), np.uint8), np.zeros((len(vecs), M))
        for b, (l, s) in enumerate(vecs):
            lab[b, :len(l)], sc[b, :len(s)] = l, s
        out[name] = (lab, sc, None if n_valid is None else np.asarray(n_valid, np.int32))

    add("kinds", [ap_vector(1, 50, k) for k in ("untied", "tied", "all_tied")])
    add("no_pos_all_pos", [ap_vector(2, 40, "no_pos"), ap_vector(3, 40, "all_pos"), ap_vector(4, 40, "tied")])
    add("one_entry", [(np.array([1], np.uint8), np.array([0.3])), (np.array([0], np.uint8), np.array([0.3]))])
    add("no_entry", [(np.zeros(0, np.uint8), np.zeros(0))])
    add("ragged", [ap_vector(5, 90, "tied"), ap_vector(6, 90, "untied"), ap_vector(7, 90, "tied")], n_valid=[90, 0, 37])
    for m in EDGES:
        add(f"edge_{m}", [ap_vector(200 + m, m, "tied" if m % 2 else "untied")])
    return out


@functools.lru_cache(maxsize=None)
def ap_ref(name):
    lab, sc, nv = ap_jobs()[name]
    return [dr.average_precision(lab[b, :lab.shape[1] if nv is None else nv[b]], sc[b, :sc.shape[1] if nv is None else nv[b]])
            for b in range(len(lab))]


def check_ap(got, name, b, what=""):
    """got: dict(ap, n_pos, tp_at [M], cnt_at [M]) of pair b; the counts past n_valid must be 0."""
    r = ap_ref(name)[b]
    tag = f"{what} ap {name}[{b}]"
    n = len(r["tp_at"])
    assert int(got["n_pos"]) == r["n_pos"], (tag, got["n_pos"], r["n_pos"])
    for key in ("tp_at", "cnt_at"):
        g = np.asarray(got[key]).astype(np.int64)
        assert np.array_equal(g[:n], r[key]) and not g[n:].any(), (tag, key)
    assert abs(float(got["ap"]) - r["ap"]) <= dr.TOL * r["ap_bound"], (tag, got["ap"], r["ap"], r["ap_bound"])
    if r["n_pos"] == 0:
        assert float(got["ap"]) == 0.0, tag


# ---- what the golden file is made from (tests/golden/make_golden_repeatability.py) -----------------------------------------
def golden_inputs():
    """(kp1, kp2, H, height, width, keep_k, thresh) of a dozen small pairs with distinct probabilities, the empty cases included."""
    out = []
    for i, (n1, n2, k, th) in enumerate(((40, 35, 300, 3), (40, 35, 12, 3), (25, 50, 0, 3), (30, 30, 5, 5), (60, 20, 300, 5), (33, 47, 20, 5))):
        a, b, H = seeded_pair(300 + i, n1, n2)
        out.append((a, b, H, HEIGHT, WIDTH, k, th))
    a, b, H = seeded_pair(310, 30, 28, C=2)
    out.append((a, b, H, HEIGHT, WIDTH, 300, 3))
    a, b, H = seeded_pair(311, 20, 20)
    e = np.zeros((0, 3))
    out += [(e, b, H, HEIGHT, WIDTH, 300, 3), (a, e, H, HEIGHT, WIDTH, 300, 3), (e, e, H, HEIGHT, WIDTH, 300, 3)]
    a, b, H = _outside(312, 15)
    out.append((a, b, H, HEIGHT, WIDTH, 300, 3))
    a, b, H = lattice_pair((3, -2))
    out.append((a, b, H, HEIGHT, WIDTH, 300, 5))
    return out


def golden_ap_inputs():
    return [ap_vector(400, 30, "untied"), ap_vector(401, 30, "tied"), ap_vector(402, 64, "tied"), ap_vector(403, 20, "all_tied"),
            ap_vector(404, 12, "all_pos"), (np.array([1], np.uint8), np.array([0.3])), ap_vector(405, 257, "tied")]
