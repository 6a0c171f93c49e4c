"""Restatement of the SuperPoint output processing (include/dfepe.h, the dfepe_sp_* block) for the tests: the sequential nms_fast
with its padded grid in numpy (a different algorithm from the kernel's fixpoint), the stated formulas in float64 numpy, and the
same formulas in torch for autograd (any dtype: float64 is the reference, float32 measures what single precision costs).

Tolerances.  Every kernel computes a value in fp64 from fp32 data and rounds it once, so against this float64 restatement
    |kernel - ref| <= 2^-24 |ref| + 2^-36 scale,    scale = max |ref| over the tensor:
the first term is the one rounding to fp32 (half an ulp), the second bounds the fp64 work: at most 2^13 operations per value (the
adjoint of a 9 x 9 patch sums 81 entries for each of up to 81 covering points) at 2^-53 each, times 2^4 of head-room for
cancellation among the summed terms.  TOL() returns it.  The NMS is integers and copied floats: exact.
Where the kernel's *input* already differs from the restatement's (the chain: its heatmap is rounded to fp32 before the
soft-argmax reads it) no such bound can be derived; there the tests measure the distance of torch's float32 evaluation of these
formulas from the float64 one on the same inputs and allow 4 times that (the margin of test_refcfg_gpu.py).
"""
import numpy as np
import torch

EPS = 1e-6


def TOL(ref):
    ref = np.asarray(ref, dtype=np.float64)
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    return 2.0 ** -24 * np.abs(ref) + 2.0 ** -36 * scale + 1e-300


def capacity(H, W, d):
    return -(-H // (d + 1)) * -(-W // (d + 1))


# ---- NMS ---------------------------------------------------------------------------------------------------------------
def visit_order(heat, thr):
    """Candidates (h >= thr; NaN is none) as flat indices in visiting order: confidence descending, index ascending."""
    flat = heat.reshape(-1)
    with np.errstate(invalid="ignore"):
        cand = np.flatnonzero(flat >= np.float32(thr))
    return cand[np.lexsort((cand, -flat[cand].astype(np.float64)))]


def nms_fast(heat, thr, d, r):
    """SuperPoint's nms_fast for one [H,W] float32 heatmap: a grid padded by d, candidates marked 1, visited in order; a
    candidate still marked 1 is kept (-1) and clears its (2d+1)^2 window.  The border is removed afterwards.
    -> (map [H,W] float32 of 0/1, pts [n,2] int32 (x, y) in row-major order, conf [n] float32)."""
    H, W = heat.shape
    grid = np.zeros((H + 2 * d, W + 2 * d), dtype=np.int8)
    order = visit_order(heat, thr)
    ys, xs = order // W, order % W
    grid[ys + d, xs + d] = 1
    for y, x in zip(ys, xs):
        if grid[y + d, x + d] == 1:
            grid[y:y + 2 * d + 1, x:x + 2 * d + 1] = 0
            grid[y + d, x + d] = -1
    kept = grid[d:d + H, d:d + W] == -1
    inside = np.zeros((H, W), dtype=bool)
    if H - r > r and W - r > r:
        inside[r:H - r, r:W - r] = True
    kept &= inside
    yy, xx = np.nonzero(kept)
    return kept.astype(np.float32), np.stack((xx, yy), 1).astype(np.int32), heat[yy, xx].astype(np.float32)


def nms_brute(heat, thr, d, r):
    """The definition, without a grid: a candidate is kept iff no candidate kept before it lies within Chebyshev distance d."""
    H, W = heat.shape
    kept = []
    for i in visit_order(heat, thr):
        y, x = divmod(int(i), W)
        if all(max(abs(y - ky), abs(x - kx)) > d for ky, kx in kept):
            kept.append((y, x))
    out = np.zeros((H, W), dtype=np.float32)
    for y, x in kept:
        if x >= r and x < W - r and y >= r and y < H - r:
            out[y, x] = 1.0
    return out


def nms_batch(heat, thr, d, r):
    """heat [B,1,H,W] -> dict like ops.sp_nms, padded to the capacity."""
    B, _, H, W = heat.shape
    cap = capacity(H, W, d)
    out = {"nms_map": np.zeros((B, 1, H, W), np.float32), "pts": np.zeros((B, cap, 2), np.int32), "conf": np.zeros((B, cap), np.float32),
           "count": np.zeros(B, np.int32)}
    for b in range(B):
        m, p, c = nms_fast(heat[b, 0], thr, d, r)
        assert len(p) <= cap
        out["nms_map"][b, 0], out["count"][b] = m, len(p)
        out["pts"][b, :len(p)], out["conf"][b, :len(p)] = p, c
    return out


# ---- flattenDetection ----------------------------------------------------------------------------------------------------
def flatten(semi):
    """semi [B,65,Hc,Wc] (NaN read as 0) -> heatmap [B,1,8Hc,8Wc] float64."""
    s = np.where(np.isnan(semi), 0.0, semi).astype(np.float64)
    e = np.exp(s - s.max(1, keepdims=True))
    p = (e / e.sum(1, keepdims=True))[:, :64]
    B, _, Hc, Wc = p.shape
    return p.reshape(B, 8, 8, Hc, Wc).transpose(0, 3, 1, 4, 2).reshape(B, 1, 8 * Hc, 8 * Wc)


def flatten_torch(semi):
    """The same in torch (dtype of semi); differentiable.  A NaN is replaced by a constant 0."""
    s = torch.where(torch.isnan(semi), torch.zeros_like(semi), semi)
    p = torch.softmax(s, dim=1)[:, :64]
    B, _, Hc, Wc = p.shape
    return p.reshape(B, 8, 8, Hc, Wc).permute(0, 3, 1, 4, 2).reshape(B, 1, 8 * Hc, 8 * Wc)


# ---- pred_soft_argmax ------------------------------------------------------------------------------------------------------
def soft_argmax(heat, pts, count, p):
    """heat [B,1,H,W], pts [B,cap,2] (x, y), count [B] -> pred [B,cap,2] float64, patches [B,cap,p,p] float64: the formulas as
    written (log, exp).  A patch whose sum is <= 0: offset 0."""
    B, cap = pts.shape[:2]
    c = p // 2
    pred, patches = np.zeros((B, cap, 2)), np.zeros((B, cap, p, p))
    grid = np.arange(p, dtype=np.float64)
    for b in range(B):
        for k in range(int(count[b])):
            x, y = int(pts[b, k, 0]), int(pts[b, k, 1])
            h = heat[b, 0, y - c:y + c + 1, x - c:x + c + 1].astype(np.float64)
            assert h.shape == (p, p)
            q = h / (h.sum() + EPS)
            q = np.where(q < 0, EPS, q)
            patches[b, k] = q
            if not h.sum() > 0:
                continue
            with np.errstate(divide="ignore"):
                l = np.log(q)
            e = np.exp(l - l.max())
            den = e.sum() + EPS
            pred[b, k] = ((e * grid[None, :]).sum() / den - c, (e * grid[:, None]).sum() / den - c)
    return pred, patches


def soft_argmax_torch(heat, pts, count, p):
    """The same function in torch (dtype of heat), differentiable w.r.t. heat.  e = exp(log q - max log q) is evaluated as
    q / max q: the same function, whose derivative exists at q = 0 where the chain through log gives 0 * inf.  amax spreads the
    maximum's gradient evenly over ties; a clamped entry (q < 0) is a constant."""
    B, cap = pts.shape[:2]
    c = p // 2
    pts = torch.as_tensor(np.asarray(pts)).long()
    n = torch.as_tensor(np.asarray(count)).long()
    live = torch.arange(cap)[None, :] < n[:, None]
    off = torch.arange(p) - c
    ys = (pts[:, :, 1, None, None] + off[None, None, :, None]).clamp(0, heat.shape[2] - 1).expand(B, cap, p, p)
    xs = (pts[:, :, 0, None, None] + off[None, None, None, :]).clamp(0, heat.shape[3] - 1).expand(B, cap, p, p)
    h = heat[torch.arange(B)[:, None, None, None], 0, ys, xs]
    s = h.sum((2, 3), keepdim=True)
    q = h / (s + EPS)
    q = torch.where(q < 0, torch.full_like(q, EPS), q)
    valid = live[:, :, None, None] & (s > 0)
    qs = torch.where(valid, q, torch.ones_like(q))  # rows without a patch: any harmless value, masked below
    e = qs / qs.amax((2, 3), keepdim=True)
    den = e.sum((2, 3)) + EPS
    grid = torch.arange(p, dtype=heat.dtype)
    ox = (e * grid[None, None, None, :]).sum((2, 3)) / den - c
    oy = (e * grid[None, None, :, None]).sum((2, 3)) / den - c
    pred = torch.stack((ox, oy), 2)
    return torch.where(valid[:, :, :, 0], pred, torch.zeros_like(pred))


# ---- sample_desc_from_points ---------------------------------------------------------------------------------------------------
def sample_desc(desc, pts, pred, count, align_corners=True):
    """desc [B,D,Hc,Wc], positions pts + pred (pixels of the [8Hc,8Wc] image) -> [B,cap,D] float64: bilinear, zero padding,
    divided by the L2 norm (zero norm: zeros); zero rows from count[b] on."""
    B, D, Hc, Wc = desc.shape
    cap = pts.shape[1]
    d64 = np.where(np.isnan(desc), 0.0, desc).astype(np.float64)
    out = np.zeros((B, cap, D))
    for b in range(B):
        for k in range(int(count[b])):
            x = float(pts[b, k, 0]) + (float(pred[b, k, 0]) if pred is not None else 0.0)
            y = float(pts[b, k, 1]) + (float(pred[b, k, 1]) if pred is not None else 0.0)
            gx, gy = x / (4.0 * Wc) - 1.0, y / (4.0 * Hc) - 1.0
            ix = (gx + 1.0) * 0.5 * (Wc - 1) if align_corners else ((gx + 1.0) * Wc - 1.0) * 0.5
            iy = (gy + 1.0) * 0.5 * (Hc - 1) if align_corners else ((gy + 1.0) * Hc - 1.0) * 0.5
            x0, y0 = int(np.floor(ix)), int(np.floor(iy))
            ax, ay = ix - x0, iy - y0
            v = np.zeros(D)
            for yy, xx, w in ((y0, x0, (1 - ax) * (1 - ay)), (y0, x0 + 1, ax * (1 - ay)), (y0 + 1, x0, (1 - ax) * ay), (y0 + 1, x0 + 1, ax * ay)):
                if 0 <= xx < Wc and 0 <= yy < Hc:
                    v += w * d64[b, :, yy, xx]
            nrm = np.sqrt((v * v).sum())
            out[b, k] = v / nrm if nrm > 0 else 0.0
    return out


# ---- the adjoint of the gathered offsets ---------------------------------------------------------------------------------------
def gather_offsets_bwd(g, m1, m2, choice, N1, N2):
    """g [B,n_out,4] float32, m1, m2 [B,N1], choice [B,n_out] -> g_off1 [B,N1,2], g_off2 [B,N2,2] in float64 index arithmetic."""
    B, n_out = choice.shape
    g1, g2 = np.zeros((B, N1, 2)), np.zeros((B, N2, 2))
    for b in range(B):
        for t in range(n_out):
            c = choice[b, t]
            g1[b, m1[b, c]] += g[b, t, :2].astype(np.float64)
            g2[b, m2[b, c]] += g[b, t, 2:].astype(np.float64)
    return g1, g2
