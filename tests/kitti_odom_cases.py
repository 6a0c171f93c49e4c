"""Shared inputs of the KITTI odometry-table tests and the one check() that the CPU tests (the restatement in its other order,
deliberately wrong results) and the GPU tests (the kernels) both go through.  The yardstick and the bounds are
tests/kitti_odom_ref.py; the golden trajectories come from tests/golden/kitti_odom.npz.

A case is a dict: est, gt [S,n_max,12] float64 (rows past a sequence's own length hold NaN), est_len, gt_len [S], step, mode.  A
result is a dict of numpy arrays in the C ABI's layout: est, gt [S,n_max,12], rtc [S,13], dist [S,n_max], rows [S,F,8,5],
valid [S,F,8], count [S], summary [S,5]; the buffers held SENTINEL (valid: 7) before the launch.

Synthetic trajectories: a vehicle that moves about 1 m per frame (forward motion 1 +- 0.05, small lateral and vertical motion,
yaw ~ N(0, 0.03^2), pitch and roll a tenth of that, so the path is not planar; the planar cases say so); the
estimate chains the same motions perturbed (rotation vector + N(0, 0.002^2), translation x 0.6 + N(0, 0.01^2)), a monocular
estimate at the wrong scale.  Everything is rounded to float32 and widened.  No (first, len) pair of any case may be undecided
(kitti_odom_ref.undecided); the CPU test asserts the margins.
"""
import functools
import os
import zlib

import numpy as np

import kitti_odom_ref as K
from odometry_cases import rodrigues

SENTINEL = -7777.25
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kitti_odom.npz")
RUNS, SEQS = ("deepFEPE", "deepF"), ("09", "10")

# name -> (gt lengths, est lengths or None (= gt's), step, kind)
CASES = {
    "n1": ((1,), None, 10, "plain"),
    "n2": ((2,), None, 10, "plain"),
    "short_of_100m": ((100,), None, 10, "short"),   # 99 steps of 0.99 m: no segment at all
    "past_100m": ((104,), None, 10, "unit"),        # 103 steps of 1 m: first = 0, len = 100 and nothing else
    "n255": ((255,), None, 10, "plain"),
    "n256": ((256,), None, 10, "plain"),
    "n257": ((257,), None, 10, "plain"),
    "n513": ((513,), None, 10, "plain"),            # 52 first frames, 416 pairs: no multiple of the lanes
    "n513_step7": ((513,), None, 7, "plain"),       # 74 first frames, 592 pairs
    "n257_step1": ((257,), None, 1, "plain"),       # 2056 pairs: eight and a bit per lane
    "ragged": ((513, 120, 257), None, 10, "plain"),
    "m_lt_n": ((400, 300), (300, 150), 10, "plain"),  # segments with last >= m are dropped; ATE and RPE over m frames
    "mirrored": ((300,), None, 10, "mirrored"),     # det(U) det(V^T) < 0: the S flip
    "same_motion": ((300,), None, 10, "same"),      # est == gt: tr E_R rounds past 3, the clamp decides; RPE angles of exactly 0
    "stationary_est": ((150,), None, 10, "stationary"),  # sigma_x^2 = 0
    "collinear": ((300,), None, 10, "collinear"),   # Umeyama's rotation undetermined; scale_7dof still decided
    # exactly planar translations (y = 0 in every frame): C has rank 2, Umeyama's rotation is still determined
    "planar": ((300,), None, 10, "planar"),         # both trajectories in the plane: a zero row and a zero column of C
    "planar_est": ((300,), None, 10, "planar_est"),  # a zero column of C
    "planar_gt": ((300,), None, 10, "planar_gt"),   # a zero row of C
    # the path length leaves LDS past 4096 frames (_lib.KITTI_DIST_LDS): the last size inside, the first outside, and KITTI 02's
    "n4096": ((4096,), None, 10, "plain"),
    "n4097": ((4097,), None, 10, "plain"),
    "n4661": ((4661,), None, 10, "plain"),
}
# where dist is kept does not depend on the alignment: the long cases run in the default mode, the longest also in 7dof
ONLY_MODES = {"n4096": ("scale_7dof",), "n4097": ("scale_7dof",), "n4661": ("scale_7dof", "7dof")}
# A trajectory whose translations are collinear (n <= 2 frames, a straight line, a stationary estimate) leaves Umeyama's rotation
# undetermined: 7dof and 6dof on such input are outside the contract and not run; scale_7dof is decided and is.
NO_ROTATION = ("n1", "n2", "past_100m", "short_of_100m", "stationary_est", "collinear")


def modes(name):
    if name in ONLY_MODES:
        return ONLY_MODES[name]
    return K.MODES[:3] if name in NO_ROTATION else K.MODES


RUNS_OF_CASES = [(name, mode) for name in CASES for mode in modes(name)]


def _chain(rot_vecs, trans):
    T, out = np.eye(4), []
    for w, t in zip(rot_vecs, trans):
        out.append(T[:3].reshape(12).copy())
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = rodrigues(w), t
        T = T @ M
    return np.array(out).reshape(-1, 12)


def trajectory(g, n, kind="plain"):
    """-> est, gt [n,12]"""
    w = g.randn(n, 3) * np.array([0.003, 0.03, 0.003])
    t = g.randn(n, 3) * np.array([0.02, 0.02, 0.05]) + np.array([0.0, 0.0, 1.0])
    if kind == "short":
        w, t = w * 0.0, np.tile([0.0, 0.0, 0.99], (n, 1))
    if kind == "unit":
        w, t = w * 0.0, np.tile([0.0, 0.0, 1.0], (n, 1))
    if kind == "collinear":
        w, t = w * 0.0, t * np.array([0.0, 0.0, 1.0])
    in_plane = np.array([1.0, 0.0, 1.0])  # yaw only and no vertical motion: products with exact zeros keep y = 0 exactly
    if kind in ("planar", "planar_gt"):
        w, t = w * (1.0 - in_plane), t * in_plane
    gt = _chain(w, t)
    we, te = w + 0.002 * g.randn(n, 3), 0.6 * t + 0.01 * g.randn(n, 3)
    if kind == "collinear":
        we, te = w, te * np.array([0.0, 0.0, 1.0])
    if kind in ("planar", "planar_est"):
        we, te = we * (1.0 - in_plane), te * in_plane
    est = _chain(we, te)
    if kind == "mirrored":
        est[:, 3] = -est[:, 3]
    if kind == "same":
        est = gt.copy()
    if kind == "stationary":
        est = np.tile(est[:1], (n, 1))
    # start somewhere else than the identity, so that re-basing does something
    M0 = np.eye(4)
    M0[:3, :3], M0[:3, 3] = rodrigues(np.array([0.1, -0.4, 0.05])), [3.0, -1.0, 7.0]
    if kind.startswith("planar"):
        M0 = np.eye(4)  # re-basing on the identity is exact: the plane stays a plane to the last bit
    place = lambda P: np.array([(M0 @ np.vstack([p.reshape(3, 4), [0, 0, 0, 1]]))[:3].reshape(12) for p in P])
    return place(est).astype(np.float32).astype(np.float64), place(gt).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def case(name, mode="scale_7dof"):
    gl, el, step, kind = CASES[name]
    el = gl if el is None else el
    g = np.random.RandomState(zlib.crc32(name.encode()))
    S, n_max = len(gl), max(gl)
    est, gt = np.full((S, n_max, 12), np.nan), np.full((S, n_max, 12), np.nan)
    for s in range(S):
        e, t = trajectory(g, gl[s], kind)
        est[s, :el[s]], gt[s, :gl[s]] = e[:el[s]], t
    return _finish({"name": name, "est": est, "gt": gt, "est_len": np.array(el, np.int32), "gt_len": np.array(gl, np.int32),
                    "step": step, "mode": mode})


@functools.lru_cache(maxsize=None)
def golden_case(mode="scale_7dof", step=10):
    """the four shipped trajectories as one padded batch: deepFEPE 09, deepFEPE 10, deepF 09, deepF 10"""
    z = np.load(GOLDEN, allow_pickle=False)
    keys = [(r, q) for r in RUNS for q in SEQS]
    lens = [len(z[f"gt_{q}"]) for _, q in keys]
    est, gt = np.full((4, max(lens), 12), np.nan), np.full((4, max(lens), 12), np.nan)
    for s, (r, q) in enumerate(keys):
        est[s, :lens[s]] = z[f"est_{r}_{q}"].astype(np.float64).reshape(-1, 12)
        gt[s, :lens[s]] = z[f"gt_{q}"].reshape(-1, 12)
    return _finish({"name": "golden", "est": est, "gt": gt, "est_len": np.array(lens, np.int32), "gt_len": np.array(lens, np.int32),
                    "step": step, "mode": mode, "keys": keys})


def _finish(c):
    c["F"] = -(-c["est"].shape[1] // c["step"])
    c["ref"] = [K.reference(c["est"][s, :c["est_len"][s]], c["gt"][s, :c["gt_len"][s]], c["mode"], c["step"]) for s in range(len(c["est"]))]
    for a in (c["est"], c["gt"], c["est_len"], c["gt_len"]):
        a.setflags(write=False)
    return c


def blank(c):
    """the output buffers as they are before a launch"""
    S, n_max, F = c["est"].shape[0], c["est"].shape[1], c["F"]
    f = lambda *shape: np.full(shape, SENTINEL)
    return {"est": f(S, n_max, 12), "gt": f(S, n_max, 12), "rtc": f(S, 13), "dist": f(S, n_max), "rows": f(S, F, 8, 5),
            "valid": np.full((S, F, 8), 7, np.uint8), "count": np.full(S, -7, np.int32), "summary": f(S, 5)}


def expected(c, which=0):
    """what a faultless kernel leaves in the buffers according to the yardstick (which = 0) or to its other order (which = 1)"""
    out = blank(c)
    for s, r3 in enumerate(c["ref"]):
        e = r3[which]
        m, n = int(c["est_len"][s]), int(c["gt_len"][s])
        out["est"][s, :m], out["gt"][s, :n] = e["align"]["est"], e["align"]["gt"]
        out["rtc"][s] = np.concatenate([e["align"]["r"].reshape(9), e["align"]["t"], [e["align"]["c"]]])
        out["dist"][s, :n] = e["seg"]["dist"]
        k = len(e["seg"]["first"])
        out["rows"][s].reshape(-1, 5)[:k] = e["seg"]["rows"]
        out["valid"][s].reshape(-1)[:k] = e["seg"]["valid"]
        out["count"][s], out["summary"][s] = e["count"], e["summary"]
    return out


def assert_published(got, want, run, seq):
    """half a unit of the last printed digit plus slack: 5.5e-4"""
    tol = np.full(5, 5.5e-4)
    if (run, seq) == ("deepF", "10"):
        tol[3] = 1e-3  # the one written exception: RPE (m) restates to 0.25242, the file prints 0.253
    assert (np.abs(got - want) <= tol).all(), (got, want)


def _frac(got, want, tol, what):
    """largest |got - want| / tol; where the yardstick is not finite the result must not be finite either"""
    got, want, tol = np.asarray(got, np.float64), np.asarray(want, np.float64), np.broadcast_to(tol, np.shape(want))
    fin = np.isfinite(want)
    assert not np.isfinite(got[~fin]).any(), f"{what}: finite where the yardstick is not"
    if not fin.any():
        return 0.0
    with np.errstate(all="ignore"):
        ratio = np.abs(got[fin] - want[fin]) / tol[fin]
    assert np.isfinite(got[fin]).all(), f"{what}: not finite where the yardstick is"
    worst = float(ratio.max())
    assert worst <= 1.0, f"{what}: {worst:.3g} times its bound"
    return worst


def _rank_deficient(al):
    """C of rank < 2 (a collinear or a stationary trajectory) leaves Umeyama's rotation, and with it t, undetermined"""
    if "sums" not in al or not np.isfinite(al["sums"]["C"]).all():
        return "sums" in al
    D = np.linalg.svd(al["sums"]["C"])[1]
    return D[1] <= 1e-9 * D[0] or D[0] == 0.0


def check(c, got):
    """Hold a result to the yardstick.  -> dict of the achieved fractions of the bounds.  r and t of the alignment are outside
    the contract, and not compared, where the trajectory is collinear or stationary."""
    fig = {k: 0.0 for k in ("poses", "rtc", "dist", "seg_r", "seg_t", "summary")}
    fig["pairs"] = 0
    for s, (ref, _, b) in enumerate(c["ref"]):
        m, n = int(c["est_len"][s]), int(c["gt_len"][s])
        seg = ref["seg"]
        assert len(K.undecided(seg)) == 0, "an undecided (first, len) pair in a test input"
        assert np.all(got["est"][s, m:] == SENTINEL) and np.all(got["gt"][s, n:] == SENTINEL), f"sequence {s}: a pose written past its length"
        assert np.all(got["dist"][s, n:] == SENTINEL), f"sequence {s}: dist written past its length"
        fig["poses"] = max(fig["poses"], _frac(got["est"][s, :m], ref["align"]["est"], b["est"], "aligned estimate"),
                           _frac(got["gt"][s, :n], ref["align"]["gt"], b["gt"], "re-based ground truth"))
        want = np.concatenate([ref["align"]["r"].reshape(9), ref["align"]["t"], [ref["align"]["c"]]])
        deficient = _rank_deficient(ref["align"])
        assert not (deficient and c["mode"] in ("7dof", "6dof")), "7dof / 6dof on a collinear trajectory is outside the contract"
        sel = slice(12, 13) if deficient else slice(0, 13)
        fig["rtc"] = max(fig["rtc"], _frac(got["rtc"][s, sel], want[sel], b["rtc"][sel], "alignment"))
        fig["dist"] = max(fig["dist"], _frac(got["dist"][s, :n], seg["dist"], max(K.dist_bound(seg["dist"]), 1e-300), "dist"))
        k = len(seg["first"])
        rows, valid = got["rows"][s].reshape(-1, 5), got["valid"][s].reshape(-1)
        assert np.all(rows[k:] == SENTINEL) and np.all(valid[k:] == 7), f"sequence {s}: a row written past the last first frame"
        assert np.array_equal(valid[:k], seg["valid"].astype(np.uint8)), f"sequence {s}: the scored pairs differ"
        assert int(got["count"][s]) == ref["count"], f"sequence {s}: count {got['count'][s]} against {ref['count']}"
        v = seg["valid"]
        assert not rows[:k][~v].any(), "a pair that is not scored has a row"
        if v.any():
            r, w = rows[:k][v], seg["rows"][v]
            assert np.array_equal(r[:, 0], w[:, 0]) and np.array_equal(r[:, 3], w[:, 3]), "first frame or length differ"
            _frac(r[:, 4], w[:, 4], 4 * K.U * w[:, 4], "speed")  # the same end frame: one division and one product
            fig["seg_r"] = max(fig["seg_r"], _frac(r[:, 1], w[:, 1], b["seg_r"][v] / seg["len"][v] + 2 * K.U * np.abs(w[:, 1]), "segment rotation"))
            fig["seg_t"] = max(fig["seg_t"], _frac(r[:, 2], w[:, 2], b["seg_t"][v] / seg["len"][v] + 2 * K.U * np.abs(w[:, 2]), "segment translation"))
        fig["pairs"] += int(v.sum())
        fig["summary"] = max(fig["summary"], _frac(got["summary"][s], ref["summary"], np.maximum(b["summary"], 1e-300), "summary"))
    return fig


def report(name, fig):
    return (f"{name}: {fig['pairs']} segments; fractions of the bounds: poses {fig['poses']:.2f}, alignment {fig['rtc']:.2f}, dist "
            f"{fig['dist']:.2f}, segment r {fig['seg_r']:.2f}, segment t {fig['seg_t']:.2f}, summary {fig['summary']:.2f}")
