"""Shared pieces of the GPU cheirality tests: scene builders, the CPU twin of the kernel's ambiguity rule, and the one comparison
(check_cheirality) of a device result with the fp64 restatement of tests/cheirality_ref.py."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cheirality_ref as cref  # noqa: E402

WAVE = 64


def scaled_y(sc, s=1.25):
    """The scene seen by a camera with fy = s fx: y pixel coordinates and K's second row scaled by s (F and the pose unchanged
    in the normalised frame)."""
    m = sc["matches_xy_ori"].clone()
    m[..., 1] *= s
    m[..., 3] *= s
    K = sc["Ks"].clone()
    K[:, 1] *= s
    return m.contiguous(), K.contiguous()


def unit_E(sc):
    return (sc["E_gt"] / sc["E_gt"].flatten(1).norm(dim=1)[:, None, None]).float()


def far_scene(dfepe, B, N, seed, zmin=200.0, zmax=1e7, noise_px=0.5, exact_inf=0.0):
    """Low-parallax pairs: the motions, cameras and E of make_scene(B, 8, seed), N points per pair at depths log-uniform in
    [zmin, zmax] m, projected into both views, `noise_px` of Gaussian noise, rounded to fp32.  `exact_inf`: that share of the rows
    (the last ones) are points at infinity without noise.  fp32 cannot tell which side of the camera such a point is on; fp64 can.
    Returns (E [B,3,3], K [B,3,3], matches [B,N,4]) fp32 CPU tensors."""
    sc = dfepe.synth.make_scene(B, 8, seed=seed)
    g = np.random.default_rng(seed)
    K = sc["Ks"].double().numpy()
    M = sc["delta_Rtijs_4_4"].double().numpy()
    uv = np.stack((g.uniform(0, 1241, (B, N)), g.uniform(0, 376, (B, N)), np.ones((B, N))), -1)
    ray = np.einsum("bij,bnj->bni", np.linalg.inv(K), uv)
    z = np.exp(g.uniform(np.log(zmin), np.log(zmax), (B, N)))
    n_inf = int(exact_inf * N)
    X1 = ray * z[..., None]
    X2 = np.einsum("bij,bnj->bni", M[:, :3, :3], X1) + M[:, None, :3, 3]
    if n_inf:
        X2[:, N - n_inf:] = np.einsum("bij,bnj->bni", M[:, :3, :3], ray[:, N - n_inf:])
    x2 = np.einsum("bij,bnj->bni", K, X2)
    x2 = x2[..., :2] / x2[..., 2:]
    noise = noise_px * g.standard_normal((B, N, 4))
    if n_inf:
        noise[:, N - n_inf:] = 0.0
    m = np.concatenate((uv[..., :2], x2), -1) + noise
    return unit_E(sc), sc["Ks"].float(), torch.from_numpy(m.astype(np.float32))


def predicted_ambiguous(E, K, matches, depth_thres):
    """[N] bool: the correspondences the kernel's fast path is expected to queue for its fp64 route -- its margin rule
    (cheirality_body.h; scripts/proto_cheirality_margin.py is the prototype) evaluated with EXACT eigenvectors of the unit-trace
    fp64 normal matrix: dl = max(3.2e-7 / gapprod, 1e-6) |X| with gapprod = (l1 - l4)(l2 - l4)(l3 - l4); ambiguous when, for either
    rotation candidate, |X3| < dl, |z1n| < dl, |z2n| < 2 dl, ||z1n| - thr |X3|| < (1 + thr) dl or ||z2n| - thr |X3|| < (2 + thr) dl.
    The kernel evaluates the rule on its fp32 vector, so single correspondences near the margin may differ: callers keep a factor
    of two between this prediction and what they need."""
    K = np.asarray(K, np.float32).astype(np.float64)
    m = np.asarray(matches, np.float32).astype(np.float64)
    thr = float(np.float32(depth_thres))
    cands = cref.candidates(np.asarray(E, np.float32).astype(np.float64))
    P1 = K @ np.c_[np.eye(3), np.zeros(3)]
    amb = np.zeros(len(m), bool)
    for R, t in (cands[0], cands[2]):
        P2 = K @ np.c_[R, t]
        A = np.stack((m[:, 0, None] * P1[2] - P1[0], m[:, 1, None] * P1[2] - P1[1],
                      m[:, 2, None] * P2[2] - P2[0], m[:, 3, None] * P2[2] - P2[1]), 1)
        S = np.einsum("nki,nkj->nij", A, A)
        lam, V = np.linalg.eigh(S / np.trace(S, axis1=1, axis2=2)[:, None, None])
        X = V[:, :, 0]
        gap = (lam[:, 1] - lam[:, 0]) * (lam[:, 2] - lam[:, 0]) * (lam[:, 3] - lam[:, 0])
        dl = np.maximum(3.2e-7 / np.maximum(gap, 1e-30), 1e-6)
        w, z1n = X[:, 3], X[:, 2]
        z2n = X[:, :3] @ R[2] + t[2] * w
        aw = thr * np.abs(w)
        amb |= (~(gap > 0) | (np.abs(w) < dl) | (np.abs(z1n) < dl) | (np.abs(z2n) < 2 * dl) |
                (np.abs(np.abs(z1n) - aw) < (1 + thr) * dl) | (np.abs(np.abs(z2n) - aw) < (2 + thr) * dl))
    return amb


def per_wavefront(amb, nw):
    """Ambiguous correspondences per wavefront: group g of 64 belongs to wavefront g mod nw."""
    grp = np.arange(len(amb)) // WAVE
    return [int(amb[grp % nw == w].sum()) for w in range(nw)]


def predicted_drains(amb, nw):
    """Per wavefront, the carry (entries left behind) of every full drain of its queue: the kernel appends a group's ambiguous
    correspondences and, from 64 queued on, sends the first 64 through the fp64 route and moves the rest to the front."""
    grp = amb[: len(amb) // WAVE * WAVE].reshape(-1, WAVE).sum(1).tolist() + ([int(amb[len(amb) // WAVE * WAVE:].sum())] if len(amb) % WAVE else [])
    out = []
    for w in range(nw):
        qn, carries = 0, []
        for n in grp[w::nw]:
            qn += n
            if qn >= WAVE:
                qn -= WAVE
                carries.append(qn)
        out.append(carries)
    return out


def wavefronts(B, N):
    """Wavefronts per pair of the stand-alone launch: one from 2048 pairs on, else min(groups of 64, 4)."""
    return 1 if B >= 2048 else min((N + WAVE - 1) // WAVE, 4)


# ---- the comparison -------------------------------------------------------------------------------------------------------
def new_tally():
    return {"exact": 0, "undecided": 0, "skipped": 0, "n_undecided": 0, "n_tests": 0}


def check_pair(r, Rt, win, cnt, masks, tally=None, where=""):
    """One pair of a device result against its restatement r (cheirality_ref.reference).  Rt [3,4], win, cnt [4]: the outputs
    of the cheirality kernel; masks [4,N] bool: ransac_in_front with winner = 0, 1, 2, 3.

    The device's candidate c = 2 rr + s and the restatement's differ by the SVD gauge only: a swap of R1 / R2 and / or a global
    sign of t, i.e. c -> c ^ x with x in 0..3.  x comes from the POSE the device reports for its winner (never from counts);
    without a winner, from the intervals.  Returns x."""
    cnt = np.asarray(cnt).astype(np.int64)
    win = int(win)
    Rt = np.asarray(Rt, np.float64)
    lo, hi = r["lo"], r["hi"]
    # the counts are the row sums of the per-correspondence masks, and the vote over them is the reference's
    assert (masks.sum(1) == cnt).all(), (where, cnt, masks.sum(1))
    assert cref.select(cnt) == win, (where, cnt, win)
    if win >= 0:
        assert np.isfinite(Rt).all(), where
        Rd = Rt[:, :3].T
        td = -Rd @ Rt[:, 3]
        d = [np.linalg.norm(R - Rd) + np.linalg.norm(t - td) for R, t in r["cands"]]
        j = int(np.argmin(d))
        assert d[j] < 1e-4, (where, d)
        x = win ^ j
    else:
        assert (Rt == 0).all(), (where, Rt)
        fits = [x for x in range(4) if all(lo[c ^ x] <= cnt[c] <= hi[c ^ x] for c in range(4))]
        assert fits, (where, cnt, lo, hi)
        x = fits[0]
    perm = [c ^ x for c in range(4)]
    inf, und = r["in_front"][perm], r["undecided"][perm]
    bad = (masks != inf) & ~und
    assert not bad.any(), (where, "candidate, correspondence:", np.argwhere(bad)[:8].tolist())
    lo, hi = lo[perm], hi[perm]
    assert ((lo <= cnt) & (cnt <= hi)).all(), (where, cnt, lo, hi)
    top = int(np.argmax(lo))
    if lo[top] > 0 and all(lo[top] > hi[k] for k in range(4) if k != top):  # the vote is decided whatever the band holds
        assert win == top, (where, win, top, cnt)
        np.testing.assert_allclose(Rt, cref.inverse_pose(*r["cands"][perm[top]]), atol=2e-5, err_msg=where)
    if tally is not None:
        n_und = int(und.sum())
        tally["undecided" if n_und else "exact"] += 1
        tally["n_undecided"] += n_und
        tally["n_tests"] += und.size
    return x


def device_masks(dfepe, E, K, m, thr):
    """[4,B,N] bool: ransac_in_front for winner = 0, 1, 2, 3 (E: the fp32 matrix that is decomposed; pre is not taken here)."""
    B = m.shape[0]
    out = []
    for c in range(4):
        w = torch.full((B,), c, dtype=torch.int32, device=m.device)
        out.append(dfepe.ops.ransac_in_front(E, K, m, w, thr))
    return torch.stack(out).cpu().numpy().astype(bool)


def check_cheirality(dfepe, ref, E, K, m, thr, out, pre=None, tally=None, where="", src=None):
    """The device result out = (Rt_cam, winner, counts) of ops.cheirality(E, K, m, thr, pre=pre) (device tensors in, device
    tensors out) against the restatement, pair by pair.  ref: None (computed here from the fp32 inputs) or one restatement per
    batch slot (tiled batches hand the same object to every copy of a source pair).  With pre, the masks are taken from the
    fp32 E that ops.congruence forms (dfepe_ransac_in_front takes no pre) and the restatement from pre^T F pre in fp64.
    src [B]: the source pair of every slot of a tiled batch; slots of one source whose E, K and pre have the same bits share one
    restatement (their matches are the source's by construction).  Returns (restatements, gauges x) per slot."""
    Rt, win, cnt = (t.cpu().numpy() for t in out)
    B = m.shape[0]
    Ed = E if pre is None else dfepe.ops.congruence(E, pre)
    masks = device_masks(dfepe, Ed, K, m, thr)
    torch.cuda.synchronize()
    En, Kn, mn = E.cpu().numpy(), K.cpu().numpy(), m.cpu().numpy()
    pn = None if pre is None else pre.cpu().numpy()
    refs, xs, cache = [], [], {}
    for b in range(B):
        if ref is not None:
            r = ref[b]
        else:
            key = None if src is None else (int(src[b]), En[b].tobytes(), Kn[b].tobytes(), None if pn is None else pn[b].tobytes())
            r = cache.get(key) if key is not None else None
            if r is None:
                r = cref.reference(En[b], Kn[b], mn[b], thr, None if pn is None else pn[b])
                if key is not None:
                    cache[key] = r
        xs.append(check_pair(r, Rt[b], win[b], cnt[b], masks[:, b], tally, f"{where} pair {b}"))
        refs.append(r)
    return refs, xs


def hold_lapack_counts(r, x, dev_cnt, counts, where=""):
    """counts [4] of the same algorithm run with a LAPACK SVD (the golden file of the unmodified reference, or
    oracle.cheirality_select): they share the restatement's gauge, so they lie in its intervals candidate by candidate, and
    where the restatement leaves nothing undecided the device's counts are those numbers under the device's gauge x."""
    counts = np.asarray(counts).astype(np.int64)
    assert ((r["lo"] <= counts) & (counts <= r["hi"])).all(), (where, counts, r["lo"], r["hi"])
    if not r["undecided"].any():
        assert [int(dev_cnt[c]) for c in range(4)] == [int(counts[c ^ x]) for c in range(4)], (where, dev_cnt, counts, x)
