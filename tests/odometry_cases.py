"""Shared inputs of the odometry tests and the one check() that the CPU tests (host build of csrc/odometry_math.h, deliberately
wrong results) and the GPU tests (the kernels) both go through.  The yardstick and the bounds are tests/odometry_ref.py.

A case is a dict.  kind "chain": rel [S,n_max,12], lengths [S], cam2body (None, [S,12] with stride 0, or [S,n_max,12] with stride
12); a result is abs [S,n_max+1,12] in a buffer that held SENTINEL everywhere before.  kind "snippet": est, gt [S,m,12], windows
[S], L, compensate; a result is a dict of errors [S,W,2] float32, scale [S,W], aligned [S,W,12], stats [S,4] and, optionally,
compensated [S,W,L,12], all but stats pre-filled with SENTINEL.  References are computed once per case (lru_cache) and never
modified.

Inputs.  Chain: rotations with a uniformly random axis and an angle uniform in [0, pi) -- composing them in the wrong order is a
gross error, not a rounding one -- and translations ~ N(0, 1), all rounded to float32 and widened, so every 3x3 is a rotation
only to 6e-8 and the rigid inverse is wrong by that much; the "sheared" cases add 1e-3 N(0, 1) to every entry of the 3x3.
Snippets: a trajectory of 130 poses from motions like the golden file's, a ground truth that is a perturbed copy at 1.7 times the
scale; kappa = sum|est_t gt_t| / |sum est_t gt_t| of every non-degenerate window is asserted below 1e3 (seen: <= 1.01).
"""
import functools
import zlib

import numpy as np

import odometry_ref as R

SENTINEL = -7777.25
THREADS, CHUNK = 256, 8  # the shipped launch plan of dfepe_pose_chain (_lib.POSE_CHAIN_THREADS / _CHUNK; asserted by the tests)
TILE = THREADS * CHUNK
WAVE_CAP = 64 * CHUNK

# name -> (lengths, cam2body kind, sheared)
CHAIN_CASES = {f"n{n}": ((n,), None, False) for n in (0, 1, 2, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, WAVE_CAP - 1, WAVE_CAP,
                                                      WAVE_CAP + 1, 1591, TILE - 1, TILE, TILE + 1)}
CHAIN_CASES.update({
    "ragged": ((0, 65, 300), None, False),
    "ragged_c2b_seq": ((0, 65, 300), "seq", True),
    "ragged_c2b_pose": ((0, 65, 300), "pose", True),
    "n513_c2b_pose": ((WAVE_CAP + 1,), "pose", False),
    "n2049_c2b_seq": ((TILE + 1,), "seq", False),
})

SNIP_M = 130
# name -> (L, windows, compensate, stationary ground truth from pose .. to pose)
SNIPPET_CASES = {
    "L1": (1, (0, 1, 64, 65, SNIP_M - 1), True, None),  # a compensated snippet of one pose is 0 / 0: all windows degenerate
    "L1_as_given": (1, (0, 1, 64, 65, SNIP_M - 1), False, None),
    "L2": (2, (0, 1, 64, 65, SNIP_M - 2), True, None),
    "L5": (5, (0, 1, 64, 65, SNIP_M - 5), True, None),
    "L5_as_given": (5, (0, 1, 64, 65, SNIP_M - 5), False, None),
    "L5_stationary_gt": (5, (SNIP_M - 5,), True, (10, 15)),
    "L64": (64, (0, 1, 64, 65, SNIP_M - 64), True, None),
}


def rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def pose12(Rm, t):
    return np.concatenate([Rm, np.asarray(t, np.float64).reshape(3, 1)], axis=1).reshape(12)


def random_poses(g, n, max_angle=np.pi, t_sigma=1.0, shear=0.0):
    out = np.zeros((n, 12))
    for i in range(n):
        ax = g.randn(3)
        Rm = rodrigues(ax / np.linalg.norm(ax) * g.uniform(0.0, max_angle)) + shear * g.randn(3, 3)
        out[i] = pose12(Rm, t_sigma * g.randn(3))
    return out.astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def chain_case(name):
    lengths, c2b_kind, sheared = CHAIN_CASES[name]
    g = np.random.RandomState(zlib.crc32(name.encode()))
    S, n_max = len(lengths), max(lengths)
    rel = np.stack([random_poses(g, n_max, shear=1e-3 if sheared else 0.0) for _ in range(S)]).reshape(S, n_max, 12)
    c2b, stride = None, 0
    if c2b_kind == "seq":
        c2b = random_poses(g, S, max_angle=1.0)
    elif c2b_kind == "pose":
        c2b, stride = np.stack([random_poses(g, n_max, max_angle=1.0) for _ in range(S)]).reshape(S, n_max, 12), 12
    seq, tree = [], []
    for s, n in enumerate(lengths):
        c = None if c2b is None else (c2b[s] if stride == 0 else c2b[s, :n])
        seq.append(R.chain_sequential(rel[s, :n], c))
        tree.append(R.chain_tree(rel[s, :n], c))
    case = {"kind": "chain", "name": name, "rel": rel, "lengths": np.array(lengths, np.int32), "cam2body": c2b, "c2b_stride": stride,
            "seq": seq, "bound": [R.chain_bound(a, b) for a, b in zip(seq, tree)],
            "spread": [R.chain_spread(a, b) for a, b in zip(seq, tree)]}
    for v in (rel, c2b):
        if v is not None:
            v.setflags(write=False)
    return case


def trajectory(seed, n=SNIP_M - 1):
    """-> est, gt [n+1,12]: a trajectory like the golden file's and its perturbed ground truth at 1.7 times the scale"""
    g = np.random.RandomState(seed)
    w = 0.03 * g.randn(n, 3)
    t = g.randn(n, 3) * np.array([0.05, 0.02, 1.0]) + np.array([0.0, 0.0, 1.0])
    rel = np.stack([pose12(rodrigues(w[i]), t[i]) for i in range(n)]).astype(np.float32).astype(np.float64)
    rel_gt = np.stack([pose12(rodrigues(w[i] + 0.002 * g.randn(3)), 1.7 * rel[i, 3::4] + 0.01 * g.randn(3)) for i in range(n)])
    return R.chain_sequential(rel), R.chain_sequential(rel_gt).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def snippet_case(name):
    L, windows, compensate, still = SNIPPET_CASES[name]
    S = len(windows)
    pairs = [trajectory(300 + 11 * s + L) for s in range(S)]
    est, gt = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    if still is not None:
        gt[:, still[0]:still[1]] = gt[:, still[0]:still[0] + 1]  # the vehicle of the ground truth stands still for a window
    ref = [R.snippet_errors(est[s], gt[s], windows[s], L, compensated=compensate) for s in range(S)]
    for r in ref:
        ok = ~r["degenerate"]
        assert (r["kappa"][ok] < 1e3).all(), (name, r["kappa"][ok].max())
    if still is not None:
        assert ref[0]["degenerate"][still[0]] and ref[0]["degenerate"].sum() == 1
    est.setflags(write=False)
    gt.setflags(write=False)
    return {"kind": "snippet", "name": name, "est": est, "gt": gt, "windows": np.array(windows, np.int32), "L": L,
            "compensate": compensate, "W": max(windows), "ref": ref}


def expected(case, with_compensated=True):
    """The reference's answer in the layout of a result (SENTINEL where nothing is written): what a perfect kernel returns."""
    if case["kind"] == "chain":
        S, n_max = case["rel"].shape[:2]
        out = np.full((S, n_max + 1, 12), SENTINEL)
        for s, n in enumerate(case["lengths"]):
            out[s, :n + 1] = case["seq"][s]
        return out
    S, W, L = len(case["windows"]), case["W"], case["L"]
    out = {"errors": np.full((S, W, 2), SENTINEL, np.float32), "scale": np.full((S, W), SENTINEL),
           "aligned": np.full((S, W, 12), SENTINEL), "stats": np.zeros((S, 4))}
    if with_compensated:
        out["compensated"] = np.full((S, W, L, 12), SENTINEL)
    for s, nw in enumerate(case["windows"]):
        r = case["ref"][s]
        out["errors"][s, :nw], out["scale"][s, :nw], out["aligned"][s, :nw] = r["errors"], r["scale"], r["aligned"]
        if with_compensated:
            out["compensated"][s, :nw] = r["compensated"]
        out["stats"][s] = R.stats(r["errors"])
    return out


def _same_specials(a, b, what):
    assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: NaN pattern differs"
    assert np.array_equal(np.isposinf(a), np.isposinf(b)) and np.array_equal(np.isneginf(a), np.isneginf(b)), f"{what}: inf pattern differs"


def check_chain(case, got):
    S, n_max = case["rel"].shape[:2]
    got = np.asarray(got, np.float64).reshape(S, -1, 12)
    assert got.shape == (S, n_max + 1, 12), got.shape
    fig = {"worst_ratio": 0.0, "max_diff": 0.0, "max_spread": 0.0, "max_entry": 0.0}
    for s, n in enumerate(case["lengths"]):
        assert np.array_equal(got[s, 0], np.array(R.IDENT)), f"{case['name']}[{s}]: entry 0 is not the identity"
        assert np.array_equal(got[s, n + 1:], np.full((n_max - n, 12), SENTINEL)), f"{case['name']}[{s}]: wrote past its length"
        assert np.isfinite(got[s, :n + 1]).all()
        d = np.abs(got[s, :n + 1] - case["seq"][s]).max(axis=1)
        b = case["bound"][s]
        bad = np.nonzero(d > b)[0]
        assert len(bad) == 0, f"{case['name']}[{s}]: pose {bad[0]} is {d[bad[0]]:.3e} from the sequential result, bound {b[bad[0]]:.3e}"
        if n:
            fig["worst_ratio"] = max(fig["worst_ratio"], float((d[1:] / b[1:]).max()))
            fig["max_diff"] = max(fig["max_diff"], float(d.max()))
            fig["max_spread"] = max(fig["max_spread"], float(case["spread"][s].max()))
            fig["max_entry"] = max(fig["max_entry"], float(np.abs(case["seq"][s]).max()))
    return fig


def check_snippet(case, got):
    S, W, L = len(case["windows"]), case["W"], case["L"]
    err = np.asarray(got["errors"])
    assert err.dtype == np.float32 and err.shape == (S, W, 2), (err.dtype, err.shape)
    scale, aligned = np.asarray(got["scale"], np.float64), np.asarray(got["aligned"], np.float64).reshape(S, -1, 12)
    assert scale.shape == (S, W) and aligned.shape == (S, W, 12), (scale.shape, aligned.shape)
    comp = got.get("compensated")
    fig = {"err_ratio": 0.0, "scale_ratio": 0.0, "kappa": 0.0, "stats_ratio": 0.0, "degenerate": 0}
    for s, nw in enumerate(case["windows"]):
        r = case["ref"][s]
        what = f"{case['name']}[{s}]"
        assert np.array_equal(err[s, nw:], np.full((W - nw, 2), SENTINEL, np.float32)), f"{what}: errors written past the last window"
        assert np.array_equal(scale[s, nw:], np.full(W - nw, SENTINEL)) and np.array_equal(aligned[s, nw:], np.full((W - nw, 12), SENTINEL)), \
            f"{what}: scale / aligned written past the last window"
        e, sc, al = err[s, :nw].astype(np.float64), scale[s, :nw], aligned[s, :nw]
        deg, ok = r["degenerate"], ~r["degenerate"]
        fig["degenerate"] += int(deg.sum())
        with np.errstate(all="ignore"):
            # only exactly-degenerate windows are exempt from the bounds, and they must show the reference's NaN / inf pattern
            _same_specials(e[deg], r["errors"][deg].astype(np.float64), what + " errors (degenerate)")
            _same_specials(sc[deg], r["scale"][deg], what + " scale (degenerate)")
            _same_specials(al[deg], r["aligned"][deg], what + " aligned (degenerate)")
            assert np.isfinite(e[ok]).all() and np.isfinite(sc[ok]).all() and np.isfinite(al[ok]).all(), what
            er = np.abs(e[ok] - r["errors"][ok].astype(np.float64)) / R.error_tol(r["errors"][ok])
            sr = np.abs(sc[ok] - r["scale"][ok]) / (R.scale_tol(r["kappa"][ok]) * np.abs(r["scale"][ok]))
            ar = np.abs(al[ok] - r["aligned"][ok]) / (R.scale_tol(r["kappa"][ok])[:, None] * np.abs(r["aligned"][ok]) + 1e-300)
        assert np.array_equal(al[ok][:, [0, 1, 2, 4, 5, 6, 8, 9, 10]], r["aligned"][ok][:, [0, 1, 2, 4, 5, 6, 8, 9, 10]]), \
            f"{what}: the aligned pose's rotation is the estimate's, bit for bit"
        for name, ratio in (("errors", er), ("scale", sr), ("aligned", ar)):
            assert ratio.size == 0 or ratio.max() <= 1.0, f"{what}: {name} off by {ratio.max():.3g} times its bound"
        if ok.any():
            fig["err_ratio"] = max(fig["err_ratio"], float(er.max()))
            fig["scale_ratio"] = max(fig["scale_ratio"], float(sr.max()), float(ar.max()))
            fig["kappa"] = max(fig["kappa"], float(r["kappa"][ok].max()))
        if comp is not None:
            c = np.asarray(comp, np.float64).reshape(S, W, L, 12)
            assert np.array_equal(c[s, nw:], np.full((W - nw, L, 12), SENTINEL)), f"{what}: compensated written past the last window"
            # a compensated entry is a sum of three products: 8 roundings of the window's largest entry cover any order of them
            if nw:
                tol = 8 * R.U * np.abs(r["compensated"]).reshape(nw, L * 12).max(axis=1)
                assert (np.abs(c[s, :nw] - r["compensated"]).reshape(nw, L * 12).max(axis=1) <= tol).all(), f"{what}: compensated poses"
        # the statistics: against the fp64 two-pass reduction over the SAME float32 errors the result holds
        st, want = np.asarray(got["stats"], np.float64)[s], R.stats(err[s, :nw])
        _same_specials(st, want, what + " stats")
        if np.isfinite(want).all():
            tol = R.stats_tol(err[s, :nw])
            x = np.abs(err[s, :nw].astype(np.float64)).max(0)
            for k in (1, 3):
                assert want[k] == 0.0 or want[k] >= x[k // 2] / 1e3, "stats_tol's premise: the spread is not tiny against the values"
            ratio = np.abs(st - want) / np.maximum(tol, 1e-300)
            assert (np.abs(st - want) <= tol).all(), f"{what}: stats {st} against {want}, bound {tol}"
            fig["stats_ratio"] = max(fig["stats_ratio"], float(ratio[np.abs(st - want) > 0].max(initial=0.0)))
    return fig


def check(case, got):
    """Hold a result to the yardstick; raises AssertionError, returns the figures seen (for printing)."""
    return check_chain(case, got) if case["kind"] == "chain" else check_snippet(case, got)
