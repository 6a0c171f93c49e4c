"""Bit-for-bit comparison of EVERY output of the robust estimators between two builds of libdfepe_hip.so: dfepe_ransac_fundamental,
dfepe_ransac_essential, dfepe_lmeds_fundamental, dfepe_lmeds_essential and dfepe_ransac_homography, the optional outputs and the
workspace included, at the launch edges of the code the four share (csrc/robust_dev.h, the solve_iteration of the math headers):
chunk and select-window edges of max_iters, four pairs per select workgroup, the first N on the LDS-attribute path, tables that
are read to the end, iterations without a sample, ragged pairs.  Every buffer is pre-filled with one byte pattern, so bytes a
build leaves unwritten compare equal and bytes only one build writes do not.
usage (GPU box): python scripts/ab_robust.py libA.so libB.so"""
import ctypes, importlib, os, sys
import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
d = importlib.import_module("pytorch-deepfepe_amd")
import homography_cases as hc  # noqa: E402

ENTRIES = ("dfepe_ransac_workspace_bytes", "dfepe_ransac_fundamental", "dfepe_ransac5_workspace_bytes", "dfepe_ransac_essential",
           "dfepe_lmeds_num_iters", "dfepe_lmeds_workspace_bytes", "dfepe_lmeds_fundamental", "dfepe_lmeds_essential",
           "dfepe_homography_workspace_bytes", "dfepe_ransac_homography")
libs = []
for path in sys.argv[1:3]:
    L = ctypes.CDLL(os.path.abspath(path))
    for name in ENTRIES:
        getattr(L, name).restype, getattr(L, name).argtypes = d._lib._SIGNATURES[name]
    libs.append(L)
st = torch.cuda.current_stream().cuda_stream
i32, f32, f64, u8 = torch.int32, torch.float32, torch.float64, torch.uint8
CONF = (0.99, 0.0, 1.0, 0.999, 0.5)  # cycled over the calls (a period no loop below shares): the rule's two ends among the usual values
SEEDS = (0, 12345, (1 << 64) - 1, 7)


def buf(dtype, *shape):
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    return torch.full((n,), 0x5A, dtype=u8, device="cuda").view(dtype).reshape(shape)


def ws_buf(nbytes):
    return buf(f64, (int(nbytes) + 15) // 16 * 2 + 2)


def pairs_f(B, N, seed, special=False):
    """B pairs of a rigid scene (30 % outliers, 0.5 px); special: pair 1 uniform noise (many small models: the rule reads the
    whole table), pair 2 with every point of image 1 on one line (no iteration draws a sample)."""
    sc = d.synth.make_scene(B, N, seed=seed, outlier_ratio=0.3, noise_px=0.5)
    m = sc["matches_xy_ori"].clone()
    if special:
        rng = np.random.default_rng(seed)
        m[1] = torch.as_tensor(rng.uniform(0, 376, (N, 4)).astype(np.float32))
        t = torch.arange(N, dtype=torch.float32)
        m[2, :, 0], m[2, :, 1] = t, 3 * t + 1
    return m.cuda().contiguous(), sc["Ks"].cuda().contiguous()


def ransac_f(L, B, N, T, conf, seed, special=False):
    m, _ = pairs_f(B, N, 7 * N + B, special)
    o = dict(ws=ws_buf(L.dfepe_ransac_workspace_bytes(B, N, T)), F=buf(f32, B, 9), mask=buf(u8, B, N), n_inliers=buf(i32, B),
             iters_run=buf(i32, B), best_hyp=buf(i32, B, 2), hyp_counts=buf(i32, B, T, 3), masked=buf(f32, B, N, 4))
    rc = L.dfepe_ransac_fundamental(m.data_ptr(), B, N, 0.5, conf, T, seed, *(o[k].data_ptr() for k in o), st)
    return rc, o


def ransac_e(L, B, N, T, conf, seed):
    m, K = pairs_f(B, N, 5 * N + B)
    o = dict(ws=ws_buf(L.dfepe_ransac5_workspace_bytes(B, N, T)), E=buf(f32, B, 9), mask=buf(u8, B, N), n_inliers=buf(i32, B),
             iters_run=buf(i32, B), best_hyp=buf(i32, B, 2), hyp_counts=buf(i32, B, T, 10), hyp_E=buf(f64, B, T, 10, 9),
             masked=buf(f32, B, N, 4))
    rc = L.dfepe_ransac_essential(m.data_ptr(), K.data_ptr(), B, N, 1.0, conf, T, seed, *(o[k].data_ptr() for k in o), st)
    return rc, o


def lmeds(L, essential, B, N, T, conf, seed):
    m, K = pairs_f(B, N, 3 * N + B)
    mp, roots = (5, 10) if essential else (7, 3)
    niters = L.dfepe_lmeds_num_iters(mp, conf, T)
    o = dict(ws=ws_buf(L.dfepe_lmeds_workspace_bytes(B, mp, conf, T)), M=buf(f32, B, 9), mask=buf(u8, B, N), n_inliers=buf(i32, B),
             iters_run=buf(i32, B), best_hyp=buf(i32, B, 2), min_median=buf(f64, B), sigma=buf(f64, B),
             hyp_medians=buf(f64, B, max(niters, 1), roots), masked=buf(f32, B, N, 4))
    tail = (B, N, conf, T, seed, *(o[k].data_ptr() for k in o), st)
    rc = L.dfepe_lmeds_essential(m.data_ptr(), K.data_ptr(), *tail) if essential else L.dfepe_lmeds_fundamental(m.data_ptr(), *tail)
    return rc, o


def homography(L, N, T, flags, conf, seed):
    """Seven pairs: homographies with outliers at n_valid = N, 0, 4, 5 (or N) and past N, a collinear pair (no sample), and
    homography_cases' sampler_stop pair (at N = 200 and seed 0: a model at iteration 0, no sample at iteration 1)."""
    names = ["synth_30_5_4", "synth_30_5_1", "synth_0_0_0", "synth_60_5_7", "noise", "collinear", "sampler_stop"]
    m = torch.as_tensor(np.stack([hc.pair(name, N) for name in names]), device="cuda")
    nv = torch.tensor([N, 0, 4, min(5, N), N + 3, N, N], dtype=i32, device="cuda")
    B = len(names)
    o = dict(ws=ws_buf(L.dfepe_homography_workspace_bytes(B, N, T)), H=buf(f64, B, 9), H_model=buf(f64, B, 9), mask=buf(u8, B, N),
             n_inliers=buf(i32, B), iters_run=buf(i32, B), best_iter=buf(i32, B), hyp_counts=buf(i32, B, T))
    rc = L.dfepe_ransac_homography(m.data_ptr(), nv.data_ptr(), B, N, 3.0, conf, T, seed, flags, *(o[k].data_ptr() for k in o), st)
    return rc, o


calls = []
for N in (15, 64, 65, 257):
    for T in (1, 64, 65, 130):
        for B in (1, 4, 5):
            calls.append((f"ransac_fundamental B={B} N={N} max_iters={T}", ransac_f, (B, N, T)))
calls.append(("ransac_fundamental B=2 N=3169 max_iters=65 (LDS attribute)", ransac_f, (2, 3169, 65)))
calls.append(("ransac_fundamental B=3 N=257 max_iters=130 noise + collinear pairs", ransac_f, (3, 257, 130), dict(special=True, conf=1.0)))
for N in (6, 64, 65, 1685):
    for T in (1, 16, 17, 40):
        for B in (1, 4, 5):
            calls.append((f"ransac_essential B={B} N={N} max_iters={T}", ransac_e, (B, N, T)))
for essential, sizes in ((False, (8, 14, 64, 65, 129)), (True, (6, 64, 65, 129))):
    for N in sizes:
        for B in (1, 5):
            for T in (17, 1000):
                calls.append((f"lmeds_{'essential' if essential else 'fundamental'} B={B} N={N} max_iters={T}", lmeds, (essential, B, N, T)))
for N in (4, 5, 64, 65):
    for T in (1, 65):
        for flags in (0, 1, 2):
            calls.append((f"ransac_homography N={N} max_iters={T} flags={flags} ragged n_valid", homography, (N, T, flags)))
calls.append(("ransac_homography N=200 max_iters=3 flags=0 seed=0 (no sample past the first model)", homography, (200, 3, 0), dict(seed=0)))

bad = 0
for i, (what, fn, args, *kw) in enumerate(calls):
    kw = dict(dict(conf=CONF[i % len(CONF)], seed=SEEDS[i % len(SEEDS)]), **(kw[0] if kw else {}))
    conf = kw["conf"]
    outs = []
    for L in libs:
        rc, o = fn(L, *args, **kw)
        assert rc == 0, (what, rc)
        torch.cuda.synchronize()
        outs.append(o)
    diff = [k for k in outs[0] if not torch.equal(outs[0][k].view(u8), outs[1][k].view(u8))]
    models = int((outs[0]["n_inliers"] > 0).sum())
    print(f"{what} confidence={conf}: {len(outs[0])} buffers, {models} pairs with a model: " + (f"DIFFER {diff}" if diff else "identical"))
    if diff and bad == 0:
        k = diff[0]
        a, b = outs[0][k].view(u8).flatten(), outs[1][k].view(u8).flatten()
        at = int((a != b).nonzero()[0])
        print(f"  first differing buffer: {k}, byte {at} of {a.numel()}: {int(a[at])} against {int(b[at])}")
    bad += bool(diff)
print("ALL IDENTICAL" if bad == 0 else f"{bad} of {len(calls)} CALLS DIFFER")
sys.exit(0 if bad == 0 else 1)
