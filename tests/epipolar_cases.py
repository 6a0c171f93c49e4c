"""Inputs of the epipolar-residual tests, shared by the host test (tests/test_epipolar_ref_cpu.py) and the GPU test
(tests/test_epipolar_edges_gpu.py), with the float64 restatement (tests/epipolar_ref.py) of each computed once per process.

Scenes: synth.make_scene(B, 50, seed, M_virt=M).  T1 and T2 are ALWAYS different: each a scale of 2/W times 0.7..1.3, anisotropic,
about a centre shifted from the image centre, rounded to float32 -- what the compat model's Hartley normalisation produces per pair.
Three forms: "shared" (both [3,3]), "pair" (both [B,3,3], different for every pair), "mixed" (T1 [3,3], T2 [B,3,3]: the st1 != st2
branch of ops._t_arg / ops._floss_args).  F_l = normalised T2^-T F_gt T1^-1 + 0.003 (l + 1) randn, rounded to float32.
Clamps: 0.02 (about two thirds of the points gated), 0.5 (almost none), 1e30 (none), 0.0 (every sum and the F-loss gradient exactly 0).
Special cases: "exact" (the unperturbed F_l: every point sign-uncertain), "zero_layer" (one all-zero F layer among ordinary ones),
"epipole" (one virtual point of image 1 placed on the epipole of its own image: F x1 = 0 up to rounding, n2 ~ 0)."""
import functools
import importlib

import numpy as np

import epipolar_ref as er

IMAGE_W, IMAGE_H = 1241.0, 376.0
CLAMPS = (0.02, 0.5, 1e30, 0.0)
TFORMS = ("shared", "pair", "mixed")

# (L, B, M): the smallest shapes that reach each edge of floss_kernel (slot 2 of the cached path at 64/65, the re-reading path at 129,
# lanes < L at 9/10/16, partial workgroups of 4 pairs) ...
FLOSS_SHAPES = [(3, 5, M) for M in (1, 63, 64, 65, 100, 128, 129, 200)] + [(L, 5, 100) for L in (1, 9, 10, 16)] + \
               [(2, B, 37) for B in (1, 4, 5, 9)]
# ... and of tail_floss_row (every IT rung 1/2/4/7(/8) and its edges, partial workgroups of 16 pairs, the odd-L remainder of the
# two-at-a-time walk)
TAIL_SHAPES = [(3, 17, M) for M in (1, 16, 17, 32, 33, 64, 65, 112)] + [(3, B, 37) for B in (1, 15, 16, 33)] + \
              [(L, 17, 37) for L in (1, 2, 4, 5, 16)]
TAIL_ABI_SHAPES = [(3, 17, 113), (3, 17, 128)]
EMU_SHAPES = [(L, 6, M) for M in (1, 16, 17, 33, 65, 113, 128) for L in (1, 2, 3)]
SPECIALS = ("exact", "zero_layer", "epipole")


def _tform(g, B, per_pair):
    n = B if per_pair else 1
    s = (2.0 / IMAGE_W) * g.uniform(0.7, 1.3, (n, 2))
    c = np.array([IMAGE_W / 2, IMAGE_H / 2]) + g.uniform(-40.0, 40.0, (n, 2))
    T = np.zeros((n, 3, 3))
    T[:, 0, 0], T[:, 1, 1], T[:, 2, 2] = s[:, 0], s[:, 1], 1.0
    T[:, 0, 2], T[:, 1, 2] = -s[:, 0] * c[:, 0], -s[:, 1] * c[:, 1]
    T = T.astype(np.float32)
    return T if per_pair else T[0]


class Case:
    pass


@functools.lru_cache(maxsize=None)
def make_case(L, B, M, tform="pair", seed=0, special=None):
    """float32 numpy inputs of one case: F [L,B,3,3], T1, T2, K [B,3,3], v1 / v2 [B,M,3], upstream g_ls [L,B] (both signs, 0.5..1.5 in
    magnitude), g_E [L,B,3,3], and ground truth for the pose part (q_gt, t_gt, R_gt)."""
    dfepe = importlib.import_module("pytorch-deepfepe_amd")
    sc = dfepe.synth.make_scene(B, 50, seed=seed, M_virt=M)
    g = np.random.default_rng(1000 + seed)
    c = Case()
    c.L, c.B, c.M, c.tform, c.seed, c.special = L, B, M, tform, seed, special
    c.T1 = _tform(g, B, tform == "pair")
    c.T2 = _tform(g, B, tform != "shared")
    assert not np.array_equal(er.per_pair(c.T1, B), er.per_pair(c.T2, B))
    c.v1 = np.ascontiguousarray(sc["pts1_virt_ori"].numpy().astype(np.float32))
    c.v2 = np.ascontiguousarray(sc["pts2_virt_ori"].numpy().astype(np.float32))
    c.K = np.ascontiguousarray(sc["Ks"].numpy().astype(np.float32))
    T1i, T2i = np.linalg.inv(er.per_pair(c.T1, B)), np.linalg.inv(er.per_pair(c.T2, B))
    Fn = np.swapaxes(T2i, 1, 2) @ sc["F_gt"].double().numpy() @ T1i
    Fn = Fn / np.sqrt((Fn ** 2).sum((1, 2)))[:, None, None]
    noise = 0.0 if special == "exact" else 0.003
    c.F = np.stack([Fn + noise * (l + 1) * g.standard_normal((B, 3, 3)) for l in range(L)]).astype(np.float32)
    if special == "zero_layer":
        c.F[L // 2] = 0.0
    if special == "epipole":
        # the epipole of image 1 under layer 0 of pair 0 is the null vector of F (in transformed coordinates); its pixel is T1^-1 of it
        _, _, vt = np.linalg.svd(c.F[0, 0].astype(np.float64))
        e = T1i[0] @ vt[2]
        c.v1[0, M // 2] = (e / e[2]).astype(np.float32)
    c.g_ls = (g.uniform(0.5, 1.5, (L, B)) * np.where(g.uniform(size=(L, B)) < 0.5, -1.0, 1.0)).astype(np.float32)
    c.g_E = g.standard_normal((L, B, 3, 3)).astype(np.float32)
    c.q_gt = np.ascontiguousarray(sc["qs_cam"].numpy().reshape(B, 4).astype(np.float32))
    c.t_gt = np.ascontiguousarray(sc["ts_cam"].numpy().reshape(B, 3).astype(np.float32))
    c.R_gt = np.ascontiguousarray(np.swapaxes(sc["delta_Rtijs_4_4"].numpy()[:, :3, :3], 1, 2).astype(np.float32))
    return c


@functools.lru_cache(maxsize=None)
def reference(case, clamp_at):
    """The restatement of one case at one clamp, computed once and never modified."""
    return er.floss_ref(case.F, case.T1, case.T2, case.K, case.v1, case.v2, clamp_at)


def seed_of(L, B, M):
    return 7 * L + 3 * B + M


def shared_cases():
    """Every (L, B, M, tform, clamp, special) that both the CPU measurement of the two constants and the GPU tests run.  The T form
    and the clamp cycle over the shapes; (3, 5, 100) takes every T form with every clamp; the special cases come last."""
    out = []
    shapes = list(dict.fromkeys(FLOSS_SHAPES + TAIL_SHAPES + TAIL_ABI_SHAPES + EMU_SHAPES))
    for k, (L, B, M) in enumerate(shapes):
        out.append((L, B, M, TFORMS[k % 3], CLAMPS[k % 2], None))
    for tf in TFORMS:
        for cl in CLAMPS:
            out.append((3, 5, 100, tf, cl, None))
    for sp in SPECIALS:
        out.append((3, 5, 100, "pair", 0.02, sp))
    return list(dict.fromkeys(out))


def pick(L, B, M):
    """The shared case of a shape: (case, clamp)."""
    for (l, b, m, tf, cl, sp) in shared_cases():
        if (l, b, m) == (L, B, M) and sp is None:
            return make_case(L, B, M, tf, seed_of(L, B, M)), cl
    raise KeyError((L, B, M))


def get(L, B, M, tform, clamp, special=None):
    return make_case(L, B, M, tform, seed_of(L, B, M), special), clamp


# ---- an exactly representable point ON the gate ----------------------------------------------------------------------------------
def exact_gate_case(L=2, B=5, M=3):
    """Every operation of the fp32 evaluation is exact here, so d == clamp_at == 1 in fp32 on every point, and the gradient must pass
    (the convention d <= clamp_at): T = I, F = [[0,0,0],[0,0,-64],[0,64,s]], x1 = (0, 0, 1), x2 = (0, y2, 1) with small integers:
    l1 = F^T x2 = (0, 64, s - 64 y2), l2 = F x1 = (0, -64, s), dd = s - 64 y2 = +-32 by the choice of s, n1 = n2 = 64,
    64 + 1e-6 rounds to 64 in fp32 (half a spacing there is 3.8e-6), rcp(64) = 2^-6, d = 32 * 2^-5 = 1.
    In float64 d = 32 * 2 / 64.000001 < 1: the restatement passes the gate too, and flags every point as near the gate; the test that
    uses this case therefore holds the device to the restatement's own value with the live part of the bound only."""
    c = Case()
    c.L, c.B, c.M = L, B, M
    c.T1 = c.T2 = np.eye(3, dtype=np.float32)
    c.K = np.broadcast_to(np.eye(3, dtype=np.float32), (B, 3, 3)).copy()
    c.v1 = np.zeros((B, M, 3), dtype=np.float32)
    c.v1[..., 2] = 1.0
    c.v2 = np.zeros((B, M, 3), dtype=np.float32)
    c.v2[..., 2] = 1.0
    y2 = np.arange(B * M, dtype=np.float32).reshape(B, M) % 3 + 1.0
    y2[:, 1:] = y2[:, :1]  # one y2 per pair: s is per (layer, pair)
    c.v2[..., 1] = y2
    c.F = np.zeros((L, B, 3, 3), dtype=np.float32)
    c.F[:, :, 1, 2], c.F[:, :, 2, 1] = -64.0, 64.0
    sgn = np.where((np.arange(L)[:, None] + np.arange(B)[None]) % 2 == 0, 1.0, -1.0)
    c.F[:, :, 2, 2] = 64.0 * y2[None, :, 0] + 32.0 * sgn
    c.g_ls = np.ones((L, B), dtype=np.float32)
    return c


# ---- the one check of every entry point ------------------------------------------------------------------------------------------
RECORD = {}  # tag -> {quantity: largest observed ratio to its bound}, printed for the record; no bound is ever set from these


def _note(tag, what, ratio):
    d = RECORD.setdefault(tag, {})
    d[what] = max(d.get(what, 0.0), float(ratio))


def _ratio(err, bound):
    """Largest err / bound; an entry whose bound is 0 must be met exactly (ratio inf otherwise)."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(q.max()) if q.size else 0.0


def check(tag, r, loss_sum=None, g_F=None, g_ref=None, g_bound=None, E=None, extra_abs=None):
    """Hold what an entry point returned to the restatement `r` (epipolar_ref.Ref):
      loss_sum [L,B]     within sum of bound_fwd(C_FWD) over the pair's points; exactly 0 at clamp 0;
      g_F [L,B,3,3]      within g_bound (a bound_grad(...) of `r`, plus extra_abs where the caller's path adds roundings of its own)
                         of g_ref; an entry whose bound is 0 (clamp 0, an all-zero layer's dead entries) must be met exactly;
      E [L,B,3,3]        within one float32 spacing of |T2 K| |F| |T1 K| of float32(E_ref).
    Prints and records the largest ratio to each bound; returns them."""
    f = lambda t: np.asarray(t.detach().cpu() if hasattr(t, "detach") else t, dtype=np.float64)
    out = {}
    if loss_sum is not None:
        ls = f(loss_sum)
        assert np.isfinite(ls).all(), tag
        if r.pt.clamp_at == 0.0:
            assert (ls == 0.0).all(), f"{tag}: a sum at clamp 0 is not exactly 0"
        out["loss_sum"] = _ratio(np.abs(ls - r.loss_sum), r.bound_loss_sum())
    if g_F is not None:
        g = f(g_F)
        assert np.isfinite(g).all(), tag
        b = g_bound if extra_abs is None else g_bound + extra_abs
        out["g_F"] = _ratio(np.abs(g - g_ref), b)
    if E is not None:
        e = f(E)
        sp = np.spacing(r.E_scale.astype(np.float32)).astype(np.float64)[..., None, None]
        out["E"] = _ratio(np.abs(e - r.E.astype(np.float32).astype(np.float64)), sp)
    for k, v in out.items():
        _note(tag, k, v)
    print(f"EPI {tag}: " + "  ".join(f"{k} {v:.3f} of its bound" for k, v in out.items()))
    for k, v in out.items():
        assert v <= 1.0, f"{tag}: {k} is at {v:.3f} of its bound"
    return out
