"""The cases of the sample-loss branch and the ONE check of each stage, shared by the host build (tests/test_sample_loss_ref_cpu.py)
and the GPU (tests/test_sample_loss_gpu.py).  Every stage is fed the previous stage's outputs as the device (or the host build)
wrote them, the way tests/dsac_cases.py does: a miss names its own stage.  Bounds come from tests/sample_loss_ref.py and
tests/epipolar_ref.py (derived there), never from the code under test; every figure is printed before it is asserted."""
import functools
import importlib

import numpy as np
import torch

import fit_adjoint_cases as fac
import sample_loss_ref as slr

IMAGE_SIZE = [376, 1241, 3]
T_HW = np.array([[2.0 / 1241, 0.0, -1.0], [0.0, 2.0 / 376, -1.0], [0.0, 0.0, 1.0]], np.float32)
NAN, INF = float("nan"), float("inf")


# ---- the draw ------------------------------------------------------------------------------------------------------------------------
def _weights(B, N, seed, special=False):
    rng = np.random.RandomState(seed)
    w = (rng.rand(B, N) ** 4).astype(np.float32) + np.float32(1e-6)
    if special:
        for k, v in enumerate((0.0, -1.0, NAN, INF, 1e-42, -0.0, -INF)):
            w[:, (3 + 5 * k) % N::37] = v
    return w


def draw_cases(chunk=1024):
    cases = []

    def add(tag, B, N, H, K, weights="plain", n_valid=None, seed=0x1234567890ABCDEF, offset=0, counter=None):
        w = None if weights is None else (weights if isinstance(weights, np.ndarray) else _weights(B, N, len(cases), weights == "special"))
        cases.append(dict(tag=tag, B=B, N=N, H=H, K=K, weights=w, n_valid=None if n_valid is None else np.array(n_valid, np.int32), seed=seed,
                          offset=offset, counter=counter))

    Hs = (1, 63, 64, 65, 100)
    for kk, K in enumerate((8, 20, 32)):  # every N with every K; B and H cycle so that each value meets each K
        for j, N in enumerate((K, K + 1, 63, 64, 65, chunk + 1)):
            add(f"grid K={K} N={N}", (1, 3)[(j + kk) % 2], N, Hs[(j + kk) % 5], K, "special" if j % 2 else "plain")
    for H in Hs:
        add(f"H={H}", 3, 65, H, 20)
    add("n_valid below K, above N, inside", 3, 80, 65, 20, "special", n_valid=[17, 90, 40])
    one = np.zeros((2, 70), np.float32)
    one[0, 33], one[1, 69] = 0.25, 1e-30
    add("all mass on one index", 2, 70, 64, 20, one)
    none = _weights(3, 64, 99)
    none[1] = np.array([0.0, -1.0, NAN, INF] * 16, np.float32)
    add("no drawable weight in pair 1", 3, 64, 65, 20, none)
    tiny = _weights(1, 64, 98)
    tiny[0, 10:20] = tiny[0].max() * np.float32(2.0 ** -31)  # q = 0 under the pair's largest
    add("weights below 2^-30 of the largest", 1, 64, 100, 20, tiny)
    add("an offset that wraps", 2, 64, 65, 20, offset=0xFFFFFFFF, counter=3)
    add("uniform", 3, 65, 65, 20, None, n_valid=[3, 65, 30])
    return cases


def check_draw(idx, fallback, case):
    want, fb, qs = slr.sample_multisets(case["B"], case["N"], case["H"], case["K"], case["seed"], case["offset"], case["counter"], case["weights"],
                                        case["n_valid"])
    idx, fallback = np.asarray(idx), np.asarray(fallback)
    bad = int((idx != want).sum())
    print(f"SAMPLE draw {case['tag']}: B={case['B']} N={case['N']} H={case['H']} K={case['K']}: {bad} cells differ, fallback {fallback.tolist()} (want {fb.tolist()})")
    assert bad == 0 and (fallback == fb).all(), case["tag"]
    for b, q in enumerate(qs):
        if q is not None and any(q):
            assert all(q[i] > 0 for i in idx[b].ravel()), (case["tag"], b)  # nothing undrawable was drawn


# ---- top-K ---------------------------------------------------------------------------------------------------------------------------
def topk_cases():
    cases = []
    for K in (20, 8):
        for N in (K, 63, 65, 257):
            rng = np.random.RandomState(N + K)
            x = rng.randn(4, N).astype(np.float32)
            x[1] = 0.5                                                # all equal
            x[2] = np.round(x[2] * 2) / 2                            # runs of ties, some across the K-th place
            x[2, ::7] = 0.0
            x[2, 3::7] = -0.0
            x[3, ::5] = NAN
            x[3, 1::11] = INF
            x[3, 2::13] = -INF
            x[3, 4::9] = 1e-42
            x[0, N // 2] = x[0].max()                                 # a tie for the first place
            cases.append(dict(tag=f"K={K} N={N}", K=K, x=x, n_valid=None))
            cases.append(dict(tag=f"K={K} N={N} n_valid", K=K, x=x, n_valid=np.array([K - 2, N + 5, max(K, N // 2), K], np.int32)))
    z = np.zeros((1, 40), np.float32)
    z[0, 1::2] = -0.0
    cases.append(dict(tag="+-0 only", K=20, x=z, n_valid=None))
    return cases


def check_topk(idx, case, values=None):
    want = slr.topk(case["x"], case["K"], case["n_valid"])
    bad = int((np.asarray(idx) != want).sum())
    print(f"SAMPLE topk {case['tag']}: {bad} cells differ")
    assert bad == 0, case["tag"]
    if values is not None:
        got = np.asarray(values, np.float32).view(np.uint32)
        assert (got == np.take_along_axis(case["x"], want.astype(np.int64), 1).view(np.uint32)).all(), case["tag"]


# ---- gather, accu, fits (one builder: scenes, logits ~ N(0, 0.5^2), the sets drawn by the restatement) -------------------------------
MIN_DISTINCT = 10


@functools.lru_cache(maxsize=None)
def fit_case(B, N, H, K, seed):
    """A scene of synth.make_scene with weights = softmax(logits), logits ~ N(0, 0.5^2), and idx [B,H,K] drawn by the restatement.
    Checked here, on the CPU: every set has at least MIN_DISTINCT distinct indices (so that no set is left out of a comparison)."""
    dfepe = importlib.import_module("pytorch-deepfepe_amd")
    oracle = importlib.import_module("oracle.deepf_oracle")
    sc = dfepe.synth.make_scene(B, N, seed=seed, outlier_ratio=0.2)
    g = torch.Generator().manual_seed(500 + seed)
    logits = 0.5 * torch.randn(B, N, generator=g)
    w = torch.softmax(logits, 1).contiguous()
    p1, p2, _ = oracle.normalize_hw(sc["matches_xy_ori"].contiguous(), IMAGE_SIZE)
    idx, fb, _ = slr.sample_multisets(B, N, H, K, seed=seed + 77, weights=w.numpy())
    distinct = np.array([[len(set(idx[b, h])) for h in range(H)] for b in range(B)])
    assert distinct.min() >= MIN_DISTINCT and not fb.any(), (B, N, H, K, seed, int(distinct.min()))
    return dict(B=B, N=N, H=H, K=K, seed=seed, pts1=p1.contiguous().numpy(), pts2=p2.contiguous().numpy(), logits=logits.numpy(), weights=w.numpy(),
                idx=idx, distinct=distinct, virt1=sc["pts1_virt_ori"].numpy(), virt2=sc["pts2_virt_ori"].numpy())


def fit_cases():
    return [fit_case(2, 64, 100, 20, 3), fit_case(3, 100, 100, 20, 4), fit_case(1, 100, 65, 20, 5)]


def gather_cases():
    """The copies and accu: a fit case; a set of 20 repeats; a pair whose products underflow float32 ((1000 * 5e-6)^20 = 1e-46)."""
    c = dict(fit_case(2, 64, 100, 20, 3))
    rep = dict(c, idx=c["idx"].copy())
    rep["idx"][0, 7] = 5
    rep["idx"][1, 0] = 63
    under = dict(c, weights=c["weights"].copy())
    under["weights"][1] = (under["weights"][1] * np.float32(3.2e-4)).astype(np.float32)  # ~5e-6 each: products ~1e-46, accu ~1e-36
    odd = fit_case(3, 100, 65, 20, 6)
    return [("fit case", c), ("a set of 20 repeats", rep), ("products below float32", under), ("H = 65", odd)]


def check_gather(p1_sel, p2_sel, w_sel, accu, case, tag):
    r1, r2, rw = slr.gather(case["pts1"], case["pts2"], case["weights"], case["idx"])
    exact = all((np.asarray(a).view(np.uint32) == b.view(np.uint32)).all() for a, b in ((p1_sel, r1), (p2_sel, r2), (w_sel, rw)))
    want, bound = slr.accu(case["weights"], case["idx"])
    err = np.abs(np.asarray(accu, np.float64).reshape(want.shape) - want)
    print(f"SAMPLE gather {tag}: copies exact {exact}; accu err / bound max {np.max(err / bound):.3f}, sums {want.sum(1)}")
    assert exact and (err <= bound).all(), tag
    if tag.startswith("products"):  # the case does what it says: float32 loses every product of pair 1, fp64 keeps them
        B, H, K = case["idx"].shape
        p32 = np.prod(np.float32(1000.0) * case["weights"][1][case["idx"][1]], axis=1, dtype=np.float32)
        assert (p32 < 2.0 ** -126).all() and (p32 == 0).any() and (np.asarray(accu).reshape(B, H)[1] > 0).all(), tag  # denormal or 0 in float32


def fit_bound(distinct):
    """tests/test_w8pt_gpu.py's forward bounds on |F/|F| - ref|_F: 1e-5 for near-minimal systems (< 12 correspondences), 2e-6 else --
    with the number of DISTINCT indices of the multiset in the place of N."""
    return np.where(distinct < 12, 1e-5, 2e-6)


def check_fits(F_sel, p1_sel, p2_sel, w_sel, case, tag):
    """F_sel [B,H,3,3] of the device against the float64 fit of the rows the device gathered.  Every set is compared."""
    ref = slr.fits(p1_sel, p2_sel, w_sel)
    err = slr.fit_error(np.asarray(F_sel).reshape(-1, 3, 3), ref)
    bound = fit_bound(case["distinct"].ravel())
    print(f"SAMPLE fits {tag}: {len(err)} sets, distinct {case['distinct'].min()}..{case['distinct'].max()}, err / bound max {np.max(err / bound):.3f} "
          f"(err max {err.max():.2e})")
    assert len(err) == case["B"] * case["H"] and (err < bound).all(), tag


def check_fit_adjoint(g_w, F_sel_dev, case, GF, tag):
    """d <F_sel, GF> / d weights through gather, fit and scatter against float64 autograd on the same sets.  The bound is
    fit_adjoint_cases.bound by the smallest number of distinct indices of a set (a multiset with repeats is a near-minimal system)."""
    t = lambda a: torch.from_numpy(np.asarray(a))
    w = t(case["weights"]).double().requires_grad_(True)
    F, _ = slr.fit_selected(t(case["pts1"]), t(case["pts2"]), w, case["idx"])
    s = torch.sign((F.detach() * t(F_sel_dev).double()).flatten(2).sum(2))[..., None, None]  # LAPACK's sign against the device's gauge
    (s * F * t(GF).double()).sum().backward()
    e = fac.relerr(g_w, w.grad.numpy())
    b = fac.bound(int(case["distinct"].min()), "weights", "homog_gF")
    print(f"SAMPLE fit adjoint {tag}: {e:.3e} (bound {b:.0e})")
    assert e < b, tag


# ---- the loss ------------------------------------------------------------------------------------------------------------------------
def loss_cases():
    """F_sel around each pair's true F (2 % noise: most points beyond the clamp, some hundreds below it), M in {1, 64, 65, 100, 129},
    H in {1, 65, 100}, T shared (T1 is T2) and per pair; and, last, a residual of exactly the clamp."""
    dfepe = importlib.import_module("pytorch-deepfepe_amd")
    cases = []
    for k, (M, H) in enumerate(((1, 1), (64, 65), (65, 100), (100, 100), (129, 1), (100, 65))):
        B = 3
        sc = dfepe.synth.make_scene(B, 32, seed=40 + k, outlier_ratio=0.0)
        rng = np.random.RandomState(k)
        v1 = np.tile(sc["pts1_virt_ori"].numpy(), (1, 2, 1))[:, :M].copy()
        v2 = np.tile(sc["pts2_virt_ori"].numpy(), (1, 2, 1))[:, :M].copy()
        v2[:, ::3, :2] += rng.randn(*v2[:, ::3, :2].shape).astype(np.float32) * 3.0   # some beyond the clamp, some below
        per_pair = k % 2 == 1
        T1 = np.stack([T_HW * np.float32(1 + 0.01 * b) for b in range(B)]) if per_pair else T_HW
        T2 = np.stack([T_HW * np.float32(1 - 0.01 * b) for b in range(B)]) if per_pair else T_HW
        Ti = np.linalg.inv(T_HW.astype(np.float64))
        F0 = np.einsum("ji,bjk,kl->bil", Ti, sc["F_gt"].numpy().astype(np.float64), Ti)  # the true F between the T-normalised points
        F0 = F0 / np.linalg.norm(F0.reshape(B, 9), axis=1)[:, None, None]
        F_sel = (F0[:, None] + 0.02 * rng.randn(B, H, 3, 3)).astype(np.float32)
        g = rng.randn(B, H).astype(np.float32)
        cases.append(dict(tag=f"M={M} H={H} {'per-pair T' if per_pair else 'T1 is T2'}", F_sel=F_sel, T1=T1, T2=T2, virt1=v1, virt2=v2, clamp=slr.CLAMP, g=g))
    # a residual of EXACTLY the clamp: x1 = x2 = (0,0,1) under T = I, F = e_33 t: l1 = l2 = (0,0,t), n = 0, dd = t,
    # d = |t| 2e6 in float64; t = 2^-20 and clamp_at = float32(2^-20 * 2e6) hits the bound exactly (the gradient passes AT it)
    t = 2.0 ** -20
    F = np.zeros((1, 2, 3, 3), np.float32)
    F[0, 0, 2, 2], F[0, 1, 2, 2] = t, 2 * t
    v = np.array([[[0.0, 0.0, 1.0]]], np.float32)
    clamp = float(t * (2.0 / 1e-6))
    assert float(np.float32(clamp)) == clamp
    cases.append(dict(tag="a residual of exactly the clamp", F_sel=F, T1=np.eye(3, dtype=np.float32), T2=np.eye(3, dtype=np.float32), virt1=v, virt2=v,
                      clamp=clamp, g=np.ones((1, 2), np.float32)))
    return cases


def check_loss(loss_sum, g_F, case):
    """Forward and adjoint against tests/epipolar_ref.py with its own bounds (derived there for float32 kernels; this one computes in
    float64 and rounds once, so it sits far inside)."""
    r = slr.floss(case["F_sel"], case["T1"], case["T2"], case["virt1"], case["virt2"], case["clamp"])
    want = r.loss_sum.T
    e = np.abs(np.asarray(loss_sum, np.float64) - want)
    bf = r.bound_loss_sum().T + 2.0 ** -149
    gw = r.g_F(g_loss_sum=case["g"].T).transpose(1, 0, 2, 3)
    eg = np.abs(np.asarray(g_F, np.float64) - gw)
    bg = r.bound_grad(G=np.abs(case["g"].T)).transpose(1, 0, 2, 3) + 2.0 ** -149
    near, sgn = r.flagged()
    print(f"SAMPLE loss {case['tag']}: fwd err / bound max {np.max(e / bf):.3f}, grad err / bound max {np.max(eg / bg):.3f}, "
          f"clamped {int((r.pt.d > r.pt.clamp_at).sum())} of {r.pt.d.size} points, flagged {int(near.sum())} + {int(sgn.sum())}")
    assert (e <= bf).all() and (eg <= bg).all(), case["tag"]
    if "exactly" in case["tag"]:
        assert want[0, 0] == case["clamp"] and want[0, 1] == case["clamp"]
        assert np.asarray(g_F)[0, 0, 2, 2] != 0 and np.asarray(g_F)[0, 1, 2, 2] == 0  # passes AT the bound, not beyond it


# ---- the scatter ---------------------------------------------------------------------------------------------------------------------
def scatter_cases(chunk=2048):
    """H K at the lane / LDS edges (the chunk of dfepe_sample_scatter_chunk), N around the workgroup; a correspondence drawn 0, 1 and
    2000 times."""
    cases = []
    for k, (B, N, H, K) in enumerate(((2, 64, 1, 8), (1, 255, chunk // 32, 32), (2, 256, chunk // 32 + 1, 32), (3, 257, 100, 20), (1, 100, 205, 20),
                                      (2, 1025, 63, 20))):
        rng = np.random.RandomState(60 + k)
        idx = rng.randint(0, N, size=(B, H, K)).astype(np.int32)
        idx[idx == 3] = 4          # correspondence 3: never drawn
        w = (rng.rand(B, N).astype(np.float32) + np.float32(0.05)) / np.float32(N)
        cases.append(dict(tag=f"B={B} N={N} H={H} K={K}", idx=idx, weights=w, g_w_sel=rng.randn(B, H, K).astype(np.float32),
                          g_accu=rng.randn(B, H).astype(np.float32), never=3))
    B, N, H, K = 2, 100, 100, 20
    rng = np.random.RandomState(70)
    idx = np.full((B, H, K), 11, np.int32)  # correspondence 11: all 2000 cells of pair 0
    idx[1] = rng.randint(0, N, size=(H, K))
    idx[1][idx[1] == 3] = 4
    idx[1][idx[1] == 50] = 51
    idx[1, 17, 5] = 50                      # correspondence 50 of pair 1: exactly once
    w = (rng.rand(B, N).astype(np.float32) + np.float32(0.5)) * np.float32(1e-3)
    cases.append(dict(tag="drawn 0, 1 and 2000 times", idx=idx, weights=w, g_w_sel=rng.randn(B, H, K).astype(np.float32),
                      g_accu=rng.randn(B, H).astype(np.float32), never=3))
    return cases


def check_scatter(g_w, case, accu32, with_accu):
    """Against the float64 sum with (occurrences) 2^-24 of the summed magnitudes (the device sums in float64 and rounds once)."""
    B, N = case["weights"].shape
    want, mag, occ = slr.scatter(case["g_w_sel"], case["g_accu"] if with_accu else None, case["weights"], accu32, case["idx"], N)
    g_w = np.asarray(g_w, np.float64)
    bound = np.maximum(occ, 1) * 2.0 ** -24 * mag
    err = np.abs(g_w - want)
    print(f"SAMPLE scatter {case['tag']} accu={with_accu}: err / bound max {np.max(err[occ > 0] / bound[occ > 0]):.3f}, occurrences up to {occ.max()}")
    assert (err <= bound).all(), case["tag"]
    assert (g_w[occ == 0] == 0).all() and (occ[:, case["never"]] == 0).all(), case["tag"]  # exact 0 where never drawn
