"""Shared inputs of the DSAC tests and the one check() that the host build (tests/test_dsac_ref_cpu.py) and the GPU
(tests/test_dsac_gpu.py) both go through.  tests/dsac_ref.py is the fp64 restatement and says what each bound is.

The "scene" family is a calibrated two-view scene (fx != fy, different per pair) with 0.3 px noise and a share of gross outliers;
thresh = 100, beta = 0.02 are the settings at which the reference's float32 run and a float64 run agree (tests/golden/dsac.npz has
the figures); with thresh ~ 1 nearly every weight underflows and every refit is rank-deficient, which is the "saturated" edge here
and nothing else.  A decided case asserts that at most a quarter of its hypotheses are undecided for E; the seeds below were chosen
on the CPU so that the restatement alone stays within that.
"""
import functools

import numpy as np

import dsac_ref as dr

F32 = np.float32
THRESH, BETA, ALPHA = 100.0, 0.02, 0.1
OUT_KEYS = ("E_sample", "soft", "sampson", "score", "E_refit", "loss", "quality", "counts", "best", "exp_loss", "top_loss")


def _rodrigues(v):
    th = np.linalg.norm(v)
    k = v / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def scene(B, N, seed, outliers=0.2, noise=0.3):
    """X, Y [B,N,2] pixels and K [B,3,3], float32."""
    rng = np.random.default_rng(seed)
    X, Y, K = np.zeros((B, N, 2)), np.zeros((B, N, 2)), np.zeros((B, 3, 3))
    for b in range(B):
        K[b] = [[700.0 + 40 * b + rng.uniform(-20, 20), 0, 610 + rng.uniform(-15, 15)], [0, 640.0 - 25 * b, 190 + rng.uniform(-10, 10)],
                [0, 0, 1]]
        P = np.stack((rng.uniform(-6, 6, N), rng.uniform(-2, 2, N), rng.uniform(5, 25, N)), 1)
        R = _rodrigues(rng.normal(0, 0.04, 3) + 1e-3)
        t = np.array([0.8, 0.05, 0.4]) + rng.normal(0, 0.1, 3)
        p1, p2 = P @ K[b].T, (P @ R.T + t) @ K[b].T
        X[b], Y[b] = p1[:, :2] / p1[:, 2:], p2[:, :2] / p2[:, 2:]
        X[b] += rng.normal(0, noise, (N, 2))
        Y[b] += rng.normal(0, noise, (N, 2))
        bad = rng.permutation(N)[:int(round(outliers * N))]
        Y[b, bad] = np.stack((rng.uniform(0, 1241, len(bad)), rng.uniform(0, 376, len(bad))), 1)
    return X.astype(F32), Y.astype(F32), K.astype(F32)


def draw(B, N, H, S, seed):
    rng = np.random.default_rng(seed + 77)
    return np.stack([np.stack([rng.permutation(N)[:S] for _ in range(H)]) for _ in range(B)]).astype(np.int32)


def make(name, B, N, H, S=10, seed=0, outliers=0.2, thresh=THRESH, beta=BETA, loss_kind=1, decided=True, noise=0.3):
    X, Y, K = scene(B, N, seed, outliers, noise)
    return {"name": name, "B": B, "N": N, "H": H, "S": S, "X": X, "Y": Y, "K": K, "idx": draw(B, N, H, S, seed), "thresh": thresh,
            "beta": beta, "alpha": ALPHA, "loss_kind": loss_kind, "decided": decided, "seed": seed, "outliers": outliers}


def name_of(case):
    return f"{case['name']}-B{case['B']}-N{case['N']}-H{case['H']}-S{case['S']}"


def size_cases(hyps_per_block=4, vote_chunk=256):
    """The smallest sizes at which each path can go wrong: the N ladder of the fit kernels (16-lane rows; 129 crosses
    DFEPE_W8PT16_MAX_N), the hypothesis counts around a workgroup's share and a wavefront's stride, the vote's chunk, every S."""
    P, V = hyps_per_block, vote_chunk
    cases = [
        make("scene", 1, 10, P - 1, S=8, seed=11, outliers=0.0),
        make("scene", 3, 11, 1, seed=2, outliers=0.0),
        make("scene", 1, 16, 2, S=16, seed=3, outliers=0.0),     # N = S = 16
        make("scene", 3, 17, P, S=16, seed=4, outliers=0.1),
        make("scene", 1, 63, 15, seed=5, outliers=0.2),
        make("scene", 3, 64, 16, seed=6, outliers=0.3, loss_kind=2),
        make("scene", 1, 65, 17, seed=7, outliers=0.2),
        make("scene", 3, 129, P + 1, seed=8, outliers=0.2),
        make("scene", 1, 64, 65, seed=9, outliers=0.1, loss_kind=2),
        make("scene", 1, V - 1, 2, seed=10),
        make("scene", 3, V, 3, S=8, seed=17),
        make("scene", 1, V + 1, 5, seed=12),
    ]
    return cases


def edge_cases():
    out = []
    c = make("n_equals_s", 1, 10, 6, seed=21, outliers=0.0)       # every hypothesis is the same set in another order
    out.append(c)
    c = make("beta0", 3, 40, 5, seed=22, beta=0.0)                # exact: soft = 0.5, score = N/2, best = 0
    out.append(c)
    c = make("unsampled", 1, 100, 2, S=8, seed=26)                # H S < N: correspondences never sampled
    out.append(c)
    c = make("ends", 3, 33, 4, seed=24)
    c["idx"][:, 0, :2] = [0, 32]                                  # indices 0 and N-1 sampled
    c["idx"][:, 0, 2:] = np.arange(5, 13)
    out.append(c)
    c = make("saturated", 1, 40, 4, seed=25, thresh=-1.0, beta=1e6, decided=False, outliers=0.5)  # d >> thresh: every weight is 0
    out.append(c)
    return out


def golden_cases():
    """What tests/golden/make_golden_dsac.py runs the reference's own float32 DSAC on: one pair each, 10 samples per hypothesis."""
    out = []
    for N, hyps, seed, outliers in ((10, 4, 31, 0.0), (33, 8, 32, 0.2), (64, 16, 33, 0.3), (65, 16, 34, 0.4)):
        X, Y, K = scene(1, N, seed, outliers)
        out.append({"N": N, "hyps": hyps, "seed": seed, "X": X[0], "Y": Y[0], "K": K[0], "thresh": THRESH, "beta": BETA, "alpha": ALPHA})
    return out


@functools.lru_cache(maxsize=None)
def _cached(kind):
    return tuple(size_cases() if kind == "size" else edge_cases())


def all_cases():
    return list(_cached("size")) + list(_cached("edge"))


def cpu_cases():
    """What the host build goes through: the small ones (the restatement's per-hypothesis SVDs dominate the time)."""
    return [c for c in all_cases() if c["B"] * c["H"] * c["N"] <= 6000]


def check_beta0(case, got):
    """beta = 0 is exact: every weight is 0.5, every score N/2 (a sum of halves has no rounding), the first hypothesis wins, the
    quality is N/2 wherever a correspondence was sampled, and every refit is the unweighted fit (a uniform weight changes nothing)."""
    B, N, H = case["B"], case["N"], case["H"]
    assert case["beta"] == 0.0
    assert (got["soft"] == 0.5).all() and (got["score"] == N / 2).all() and (got["best"] == 0).all()
    assert ((got["counts"] > 0) | (got["quality"] == 0)).all() and (got["quality"][got["counts"] > 0] == N / 2).all()
    xn, yn = dr.kinv_points(case["X"], case["K"]), dr.kinv_points(case["Y"], case["K"])
    for b in range(B):
        E64, term = dr.fit(xn[b], yn[b])
        assert dr.decided(term), (name_of(case), b, term)
        for h in range(H):
            assert dr.unit_diff(got["E_refit"][b, h], E64) <= dr.fit_bound(term), (name_of(case), b, h)


def check(case, got, stages=(1, 2, 3, 4, 5)):
    """got: dict of numpy arrays named as ops.dsac names them (E_* as [B,H,3,3]).  Every stage is checked on the previous stage's
    outputs AS THE KERNEL WROTE THEM.  Returns the figures (largest error / bound per output, undecided counts)."""
    X, Y, K, idx = case["X"], case["Y"], case["K"], case["idx"]
    B, N, H = case["B"], case["N"], case["H"]
    tag = name_of(case)
    fig = {}

    def fits(E, E64, term, what):
        und, worst = 0, 0.0
        for b in range(B):
            for h in range(H):
                assert np.isfinite(E[b, h]).all(), (tag, what, b, h, "not finite")
                if not dr.decided(term[b, h]):
                    und += 1
                    continue
                err, bnd = dr.unit_diff(E[b, h], E64[b, h]), dr.fit_bound(term[b, h])
                worst = max(worst, err / bnd)
                assert err <= bnd, (tag, what, b, h, err, bnd, term[b, h])
        fig[what + "_ratio"], fig[what + "_undecided"] = worst, und
        print(f"{tag}: {what} largest err/bound {worst:.3g}, undecided {und}/{B * H}")
        if case["decided"]:
            assert 4 * und <= B * H, (tag, what, und, B * H)
        return und

    def within(x, ref, bound, what):
        x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
        both_nan = np.isnan(x) & np.isnan(ref)
        err = np.where(both_nan, 0.0, np.abs(x - ref))
        ok = (err <= bound) | both_nan
        ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0))) if err.size else 0.0
        fig[what + "_ratio"] = ratio
        print(f"{tag}: {what} largest err/bound {ratio:.3g}")
        assert ok.all(), (tag, what, float(err[~ok].max()), float(np.asarray(bound)[~ok].min()))

    if 1 in stages:
        E64, term = dr.stage1(X, Y, K, idx)
        fits(got["E_sample"], E64, term, "E_sample")
    s2 = dr.stage2(got["E_sample"], X, Y, K, case["thresh"], case["beta"])
    if 2 in stages:
        within(got["sampson"], s2["sampson"], s2["sampson_bound"], "sampson")
        within(got["soft"], s2["soft"], s2["soft_bound"], "soft")
        within(got["score"], s2["score"], s2["score_bound"], "score")
    if 3 in stages:
        E64, term = dr.stage3(got["soft"], X, Y, K)
        fits(got["E_refit"], E64, term, "E_refit")
    if 4 in stages:
        loss, bound = dr.stage4(got["E_refit"], X, Y, K, case["loss_kind"])
        within(got["loss"], loss, bound, "loss")
    if 5 in stages:
        s5 = dr.stage5(got["score"], idx, N, got["loss"].astype(np.float64), case["alpha"], s2["score"], s2["score_bound"])
        assert got["quality"].dtype == F32 and got["counts"].dtype == F32
        assert np.array_equal(got["quality"].view(np.uint32), s5["quality"].view(np.uint32)), (tag, "quality is not bitwise the sequential +=")
        assert np.array_equal(got["counts"], s5["counts"]), (tag, "counts")
        assert np.array_equal(got["best"], s5["best"]), (tag, "best", got["best"], s5["best"])
        for b in range(B):
            if got["best"][b] >= 0 and np.isfinite(s2["score"][b]).all():
                assert int(got["best"][b]) in s5["near"][b], (tag, "best is not within the bounds of the fp64 top score", b)
        within(got["exp_loss"], s5["exp_loss"], s5["exp_loss_bound"], "exp_loss")
        assert np.array_equal(got["top_loss"], s5["top_loss"]), (tag, "top_loss")
    return fig
