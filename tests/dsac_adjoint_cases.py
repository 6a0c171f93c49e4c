"""Shared cases of the DSAC adjoint (dfepe_dsac_bwd), their seeded upstream gradients, and the one check() that the host build
(tests/test_dsac_adjoint_ref_cpu.py) and the kernel (tests/test_dsac_adjoint_gpu.py) both go through.  tests/dsac_adjoint_ref.py is
the fp64 restatement and says what each bound is.

A case is a case of tests/dsac_cases.py (scene, index lists, thresh, beta, alpha, loss_kind) plus `up`, the names of the outputs that
get an upstream gradient.  check() takes the forward's outputs AS THE FORWARD WROTE THEM (`fwd`: E_sample, soft, score, E_refit, loss,
counts) and what the adjoint wrote (`got`: the five stage totals, the two fit adjoints' point gradients out of the workspace, g_X,
g_Y), and checks every stage on the previous stage's totals as written.

A hypothesis is DECIDED when both of its fits meet eight_point_adjoint_cases' condition, (lam_8 - lam_9) / lam_1 >= 1e-6.  Every size
case has all hypotheses decided (asserted in check()).  With dsac_cases' own settings (20-30 % gross outliers at beta = 0.02) that does
not always hold -- refits whose weights are nearly all 0 fall below -- so the seeds, beta and the outlier share below were chosen on
the CPU, with the restatement alone (test_settings_hold_for_the_restatement_alone), such that it does.  Four size cases keep
beta = 0.02 with gross outliers and have float32 `soft` entries that are exactly 0 (asserted there too).
"""
import functools

import numpy as np

import dsac_adjoint_ref as ar
import dsac_cases as dc
import dsac_ref as dr
import eight_point_adjoint_cases as ec

F32 = np.float32
ALL_UP = ("E_sample", "score", "E_refit", "loss", "quality", "exp_loss")
FIT_BOUND = ec.BOUND      # 2^-22 max |g_ref| per problem and tensor: the rule dfepe_eight_point_bwd is held to
MIN_GAP = ar.MIN_GAP
TOTALS = ("t_score", "t_loss", "t_E_refit", "t_w", "t_E_sample")

# (B, N, H, S, loss_kind, seed, outliers, beta, up, must have exact-zero weights)
SIZES = (
    (1, 8, 2, 8, 1, 104, 0.0, 0.002, ALL_UP, False),          # N = S = 8: both fits take the exact-null-vector rule
    (1, 10, 3, 8, 1, 101, 0.0, 0.02, ALL_UP, False),
    (3, 11, 1, 10, 1, 102, 0.0, 0.02, ("exp_loss",), False),
    (1, 16, 2, 16, 1, 3, 0.0, 0.02, ("quality",), False),
    (3, 17, 4, 16, 1, 4, 0.1, 0.002, ALL_UP, False),
    (1, 63, 15, 10, 1, 104, 0.2, 0.02, ALL_UP, True),
    (3, 64, 16, 10, 2, 318, 0.1, 0.02, ALL_UP, True),
    (1, 65, 17, 10, 1, 109, 0.2, 0.02, ("exp_loss", "quality"), True),
    (3, 129, 5, 10, 1, 101, 0.2, 0.002, ALL_UP, False),
    (1, 64, 65, 10, 2, 423, 0.1, 0.002, ALL_UP, False),
    (1, 255, 2, 10, 1, 10, 0.2, 0.02, ALL_UP, True),
    (3, 256, 3, 8, 1, 147, 0.2, 0.002, ALL_UP, False),
    (1, 257, 5, 10, 1, 12, 0.2, 0.002, ALL_UP, False),
)


def make(name, B, N, H, S=10, seed=0, outliers=0.2, beta=dc.BETA, loss_kind=1, up=ALL_UP, decided=True, zeros=False, **kw):
    c = dc.make(name, B, N, H, S=S, seed=seed, outliers=outliers, beta=beta, loss_kind=loss_kind, decided=decided, **kw)
    c["up"], c["zeros"] = tuple(up), zeros
    return c


def name_of(case):
    return dc.name_of(case) + "-" + ("all" if case["up"] == ALL_UP else "+".join(case["up"]))


def upstreams(case):
    """Seeded standard-normal float32 upstreams for the outputs the case names."""
    B, N, H = case["B"], case["N"], case["H"]
    rng = np.random.default_rng([case["seed"], 4242])
    shapes = {"E_sample": (B, H, 3, 3), "score": (B, H), "E_refit": (B, H, 3, 3), "loss": (B, H), "quality": (B, N), "exp_loss": (B,)}
    full = {k: rng.standard_normal(shapes[k]).astype(F32) for k in ALL_UP}   # every name is drawn, so one name's values never move
    return {k: full[k] for k in case["up"]}


@functools.lru_cache(maxsize=None)
def size_cases():
    return tuple(make("scene", B, N, H, S=S, seed=seed, outliers=o, beta=beta, loss_kind=kind, up=up, zeros=z)
                 for B, N, H, S, kind, seed, o, beta, up, z in SIZES)


@functools.lru_cache(maxsize=None)
def edge_cases():
    out = []
    out.append(make("beta0", 3, 40, 5, seed=22, beta=0.0, up=("quality",)))                    # c == 0: nothing reaches the points
    out.append(make("beta0", 3, 40, 5, seed=22, beta=0.0, up=ALL_UP))
    out.append(make("unsampled", 1, 100, 2, S=8, seed=26, beta=0.002, up=("quality",)))         # H S < N
    c = make("ends", 3, 33, 4, seed=24, beta=0.002)
    c["idx"][:, 0, :2] = [0, 32]                                                               # indices 0 and N-1 sampled
    c["idx"][:, 0, 2:] = np.arange(5, 13)
    out.append(c)
    out.append(make("n_equals_s", 1, 10, 6, seed=21, outliers=0.0))                            # every hypothesis is the same set
    out.append(make("zero_weights", 1, 40, 4, seed=127, outliers=0.2, beta=0.02, zeros=True))   # the reference's settings
    out.append(make("saturated", 1, 40, 4, seed=25, thresh=-1.0, beta=1e6, decided=False, outliers=0.5, zeros=True))
    c = make("undecided", 3, 33, 4, seed=78, outliers=0.0, beta=0.002, decided=False)
    for P in (c["X"], c["Y"]):                                                                 # pair 1, hypothesis 0: three of its ten
        P[1, c["idx"][1, 0, 1]] = P[1, c["idx"][1, 0, 0]]                                      # correspondences are one and the same,
        P[1, c["idx"][1, 0, 2]] = P[1, c["idx"][1, 0, 0]]                                      # so its rows have rank 8: no gap
    out.append(c)
    return tuple(out)


def all_cases():
    return list(size_cases()) + list(edge_cases())


def cpu_cases():
    return [c for c in all_cases() if c["B"] * c["H"] * c["N"] <= 6000]


def workspace_floats(B, N, H, S):
    """The documented layout (include/dfepe.h), section by section, in floats."""
    r4 = lambda n: (n + 3) // 4 * 4  # noqa: E731
    bn, bh = B * N, B * H
    sections = [("pn1", 2 * bn), ("pn2", 2 * bn), ("g1", 2 * bh * S), ("g2", 2 * bh * S), ("wts", bh * N), ("E_hb", 9 * bh), ("tE_hb", 9 * bh),
                ("t_score", bh), ("t_loss", bh), ("t_E_refit", 9 * bh), ("t_w", bh * N), ("t_E_sample", 9 * bh), ("gpn1", 2 * bn),
                ("gpn2", 2 * bn), ("gg1", 2 * bh * S), ("gg2", 2 * bh * S), ("Fd", 18 * bh), ("Md", 18 * bh),
                ("fit", 8 * bh * N if H > 1 else 0)]
    off, o = {}, 0
    for name, n in sections:
        off[name] = o
        o += r4(n)
    return o, off


def restated_forward(case):
    """The forward by the restatement of tests/dsac_ref.py, rounded to float32 where dfepe_dsac rounds: what the settings above were
    chosen on.  Returns `fwd` as check() takes it."""
    X, Y, K, idx = case["X"], case["Y"], case["K"], case["idx"]
    E1, _ = dr.stage1(X, Y, K, idx)
    E1 = E1.astype(F32)
    s2 = dr.stage2(E1, X, Y, K, case["thresh"], case["beta"])
    soft = s2["soft"].astype(F32)
    E3, _ = dr.stage3(soft, X, Y, K)
    E3 = E3.astype(F32)
    loss, _ = dr.stage4(E3, X, Y, K, case["loss_kind"])
    s5 = dr.stage5(s2["score"].astype(F32), idx, case["N"])
    return {"E_sample": E1, "soft": soft, "score": s2["score"].astype(F32), "E_refit": E3, "loss": loss.astype(F32), "counts": s5["counts"],
            "quality": s5["quality"]}


def gaps(case, fwd):
    """(lam_8 - lam_9) / lam_1 of every sample fit and every refit, [B,H] each, from the float32 inputs those fits read."""
    X, Y, K, idx = case["X"], case["Y"], case["K"], case["idx"]
    B, H = case["B"], case["H"]
    xn, yn = ar.kinv_points(X, K), ar.kinv_points(Y, K)
    w = ar.refit_weights(fwd["soft"])
    gs, gr = np.zeros((B, H)), np.zeros((B, H))
    with np.errstate(all="ignore"):
        for b in range(B):
            for h in range(H):
                ix = np.clip(idx[b, h], 0, case["N"] - 1)
                gs[b, h] = ar.er.problem(xn[b][ix], yn[b][ix], None, True, True, None, None).gap_lam
                gr[b, h] = ar.er.problem(xn[b], yn[b], w[b, h], True, True, None, None).gap_lam
    return np.nan_to_num(gs, nan=0.0), np.nan_to_num(gr, nan=0.0)


def check(case, fwd, got):
    """See the module docstring.  Returns the figures (largest error / bound per output)."""
    X, Y, K, idx = case["X"], case["Y"], case["K"], case["idx"]
    B, N, H, S = case["B"], case["N"], case["H"], case["S"]
    beta, alpha, kind = case["beta"], case["alpha"], case["loss_kind"]
    up = upstreams(case)
    tag = name_of(case)
    fig = {}

    def within(x, ref, bound, what):
        x = np.asarray(x)
        assert x.dtype == F32 and x.shape == np.shape(ref), (tag, what, x.dtype, x.shape, np.shape(ref))
        x, ref = x.astype(np.float64), np.asarray(ref, np.float64)
        ok_ref = np.isfinite(ref) & np.isfinite(bound)            # compared where the restatement is finite
        if case["decided"]:
            assert ok_ref.all(), (tag, what, "the restatement is not finite")
        err = np.where(ok_ref, np.abs(x - np.where(ok_ref, ref, 0.0)), 0.0)
        bnd = np.where(ok_ref, bound, 0.0)
        ratio = float(np.max(np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1.0), np.where(err > 0, np.inf, 0.0)))) if err.size else 0.0
        fig[what] = ratio
        print(f"{tag}: {what} largest err/bound {ratio:.3g}")
        assert (err <= bnd).all(), (tag, what, ratio)

    def fit_rows(x, ref, decided_rows, what):
        """|g - g_ref| <= 2^-22 max |g_ref| per leading index; rows of undecided fits are left out."""
        x = np.asarray(x)
        assert x.dtype == F32 and x.shape == ref.shape, (tag, what, x.dtype, x.shape, ref.shape)
        worst = 0.0
        for at in np.ndindex(*decided_rows.shape):
            if not decided_rows[at]:
                continue
            top = np.abs(ref[at]).max()
            err = np.abs(x[at].astype(np.float64) - ref[at]).max()
            assert np.isfinite(top) and err <= FIT_BOUND * top, (tag, what, at, float(err), float(top))
            worst = max(worst, err / (FIT_BOUND * top) if top > 0 else 0.0)
        fig[what] = worst
        print(f"{tag}: {what} largest err/bound {worst:.3g}")

    # stage 1
    t_loss, b_loss, t_score, b_score = ar.head(fwd["score"], fwd["loss"], fwd["counts"], idx, alpha, up.get("score"), up.get("loss"),
                                               up.get("quality"), up.get("exp_loss"))
    within(got["t_loss"], t_loss, b_loss, "t_loss")
    within(got["t_score"], t_score, b_score, "t_score")
    # stage 2, on the kernel's t_loss
    tE, bE = ar.loss_adjoint(fwd["E_refit"], X, Y, K, kind, got["t_loss"].astype(np.float64), up.get("E_refit"))
    within(got["t_E_refit"], tE, bE, "t_E_refit")
    # stage 3, on the kernel's t_E_refit
    xn, yn = ar.kinv_points(X, K), ar.kinv_points(Y, K)
    s = fwd["soft"].astype(np.float64)
    w = ar.refit_weights(s)
    fa = ar.fit_adjoint(xn, yn, np.ascontiguousarray(np.swapaxes(w, 0, 1)), fwd["E_refit"].astype(np.float64), got["t_E_refit"].astype(np.float64))
    sa_gap, _ = gaps(case, fwd)
    dec_r = np.nan_to_num(fa.gap_lam, nan=0.0) >= MIN_GAP            # [H,B]
    dec_s = sa_gap >= MIN_GAP                                        # [B,H]
    und_pairs = sorted(set(np.nonzero(~dec_r)[1].tolist()) | set(np.nonzero(~dec_s)[0].tolist()))
    fig["undecided"] = int((~dec_r).sum() + (~dec_s).sum())
    print(f"{tag}: undecided fits {int((~dec_s).sum())} sample + {int((~dec_r).sum())} refit of {B * H}, smallest gaps "
          f"{sa_gap.min():.3g} {np.nan_to_num(fa.gap_lam, nan=0.0).min():.3g}")
    if case["decided"]:
        assert not und_pairs, (tag, "every hypothesis of this case must be decided")
    if case["name"] == "undecided":
        assert len(und_pairs) == 1 and fig["undecided"] >= 1, (tag, und_pairs)
    fit_rows(got["t_w"], fa.gw, dec_r, "t_w")
    pair_ok = dec_r.all(0)
    fit_rows(got["gpn1"], fa.gX, pair_ok, "refit g_x")
    fit_rows(got["gpn2"], fa.gY, pair_ok, "refit g_y")
    # stage 4, on the kernel's t_score and t_w
    c = ar.score_coeff(beta, s, w, got["t_score"].astype(np.float64), np.swapaxes(got["t_w"].astype(np.float64), 0, 1))
    if case["zeros"]:                                                # c is exactly 0 wherever the float32 weight is: no inf * 0
        zero = fwd["soft"] == 0
        assert zero.any(), (tag, "no float32 soft weight is exactly 0")
        assert (c[zero & np.isfinite(np.swapaxes(got["t_w"], 0, 1))] == 0).all(), (tag, "c != 0 at a zero weight")
    tS, bS = ar.score_adjoint(fwd["E_sample"], X, Y, K, c, up.get("E_sample"))
    within(got["t_E_sample"], tS, bS, "t_E_sample")
    # stage 5, on the kernel's t_E_sample
    sa = ar.sample_adjoint(ar.gather(xn, idx), ar.gather(yn, idx), fwd["E_sample"].astype(np.float64), got["t_E_sample"].astype(np.float64))
    fit_rows(got["gg1"].reshape(B * H, S, 2), sa.gX, dec_s.reshape(-1), "sample g_x")
    fit_rows(got["gg2"].reshape(B * H, S, 2), sa.gY, dec_s.reshape(-1), "sample g_y")
    # stage 6, on the kernel's fit-adjoint outputs and totals
    gX, bX, gY, bY = ar.points(X, Y, K, idx, fwd["E_sample"], fwd["E_refit"], kind, c, got["t_loss"].astype(np.float64),
                               got["gpn1"], got["gpn2"], got["gg1"], got["gg2"])
    if case["name"] == "undecided":                                   # the pair with the undecided fit is left out, and only it
        keep = [b for b in range(B) if b not in und_pairs]
        within(got["g_X"][keep], gX[keep], bX[keep], "g_X")
        within(got["g_Y"][keep], gY[keep], bY[keep], "g_Y")
    else:
        within(got["g_X"], gX, bX, "g_X")
        within(got["g_Y"], gY, bY, "g_Y")
    if case["decided"] or case["name"] == "zero_weights":
        assert np.isfinite(got["g_X"]).all() and np.isfinite(got["g_Y"]).all(), (tag, "the gradient is not finite")
    if case["name"] == "beta0":
        ge = up.get("E_sample")
        assert np.array_equal(got["t_E_sample"], np.zeros_like(got["t_E_sample"]) if ge is None else ge), (tag, "t_E_sample != g_E_sample")
        if case["up"] == ("quality",):
            assert (got["g_X"] == 0).all() and (got["g_Y"] == 0).all(), (tag, "a gradient reaches the points with beta = 0")
    return fig
