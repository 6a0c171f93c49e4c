"""Shared inputs of the SuperPoint output-processing tests and their one check().  The shapes are the smallest that reach every
edge: 16x24 (2x3 cells), 24x32, 40x72 (more than 1024 pixels: several trips of the 1024-lane loops, H and W no multiple of d+1),
and one image above sp::kLdsPixels (104x120) for the NMS path that keeps its state in the workspace."""
import numpy as np

SHAPES = [(16, 24), (24, 32), (40, 72)]
BIG_SHAPE = (104, 120)  # 12480 > 12288 pixels
THR = 0.015             # conf_thresh of the reference's configs
NMS_DISTS = [0, 1, 4, 8]
BORDERS = [0, 4]


def nms_families(H, W, r, seed=0):
    """name -> [H,W] float32 heatmap.  Each family is built for one edge of the greedy loop."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    thr = np.float32(THR)
    fam = {}
    fam["random"] = (rng.random((H, W)) * 0.05).astype(np.float32)                       # a third below the threshold
    fam["plateau"] = np.full((H, W), 0.5, np.float32)                                    # ties only: reaches the capacity
    fam["quantised"] = (np.round(rng.random((H, W)) * 4) / 4 * 0.1).astype(np.float32)   # five levels: many ties, one level below
    fam["ramp_x"] = (thr + xx * 1e-3).astype(np.float32)                                 # the longest chains of the fixpoint
    fam["ramp_y"] = (thr + yy * 1e-3).astype(np.float32)
    fam["ramp_diag"] = (thr + (xx + yy) * 1e-3).astype(np.float32)
    fam["ramp_down"] = (thr + (H + W - xx - yy) * 1e-3).astype(np.float32)
    t = np.zeros((H, W), np.float32)
    t[H // 2, W // 2] = thr                                                              # equal to conf_thresh: a candidate
    t[H // 2, W // 2 + 1] = np.nextafter(thr, np.float32(0))                             # the float just below: none
    t[2, W - 3] = np.nextafter(thr, np.float32(1))
    fam["at_thresh"] = t
    b = np.zeros((H, W), np.float32)
    edge = max(r - 1, 0)
    b[H // 2, edge] = 0.9                                                                # in the border (r > 0), outranks ...
    b[H // 2, edge + 1] = 0.8                                                            # ... its interior neighbour
    b[edge, W // 2], b[edge + 1, W // 2] = 0.7, 0.6
    b[H - 1, W - 1], b[0, 0] = 0.5, 0.5                                                  # corners: clipped windows
    fam["border_outranks"] = b
    n = fam["random"].copy()
    n[rng.random((H, W)) < 0.1] = np.nan                                                 # NaN is no candidate
    n[1, 1] = np.inf
    fam["nan"] = n
    fam["empty"] = np.zeros((H, W), np.float32)
    return fam


def nms_batch(H, W, r, seed=0):
    fam = nms_families(H, W, r, seed)
    return list(fam), np.stack([fam[k] for k in fam])[:, None]


def rand_semi(B, Hc, Wc, seed, scale=2.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((B, 65, Hc, Wc)) * scale).astype(np.float32)


def flatten_semi(B, Hc, Wc, seed=3):
    """Random logits with a NaN cell entry, a NaN dustbin, a cell whose dustbin dominates and a cell with one huge logit."""
    s = rand_semi(B, Hc, Wc, seed)
    s[0, 5, 0, 1] = np.nan
    s[0, 64, 1, 0] = np.nan
    s[-1, 64, Hc - 1, Wc - 1] = 60.0     # dustbin dominates: the 64 probabilities are ~e^-60
    s[-1, 7, 0, 0] = 90.0                # exp would overflow fp32 without the maximum
    return s


def heat_for_patches(B, H, W, seed=5):
    """A heatmap with peaked, flat and zero-holed neighbourhoods (float32, as sp_flatten would hand it on)."""
    rng = np.random.default_rng(seed)
    h = (rng.random((B, 1, H, W)) * 0.03).astype(np.float32)
    h[0, 0, 4:13, 4:13] = 0.02                       # flat: the offset is 0 up to the epsilon terms
    h[0, 0, 8, 8] = 0.020000001
    h[-1, 0, H - 12:H - 4, 4:12] = 0.0               # zeros ...
    h[-1, 0, H - 8, 8] = 0.3                         # ... around one peak
    h[-1, 0, H - 8, 10] = 0.1
    h[0, 0, 6, W - 8] = 0.9                          # a peaked patch
    return h


def check(got, want, what, tol=None):
    """|got - want| <= tol elementwise (tol None: exact equality, NaN equal to NaN), with the worst cell in the message."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    if tol is None:
        np.testing.assert_array_equal(got, want, err_msg=what)
        return 0.0
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    bad = err > tol
    worst = float((err / np.maximum(tol, 1e-300)).max()) if err.size else 0.0
    print(f"{what}: max err {float(err.max()) if err.size else 0.0:.3e}, worst err/tol {worst:.3f}")
    assert not bad.any(), f"{what}: {int(bad.sum())} cells beyond the bound, worst err/tol {worst:.3f}, max err {float(err.max()):.3e}"
    return worst
