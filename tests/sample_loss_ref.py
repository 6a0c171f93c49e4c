"""The sample-loss branch (include/dfepe.h: dfepe_sample_multisets and what follows it) restated from the
specification and the reference's lines, not from csrc/sample_loss_math.h:
  the draw     Python integers over the streams, the quantisation and the prefix sums of tests/sampler_ref.py: equality, no tolerance
  top-K        the stated rule through Python's sort on (value class, value, index): equality
  gather, accu numpy float64
  fits         oracle.deepf_oracle.fit_forward in float64 on the gathered rows
  loss         tests/epipolar_ref.py (the per-point float64 restatement with its derived bounds), the sets in the place of the layers
  end to end   torch float64 with autograd: DeepFNetSampleLoss.Fit.forward:364-436 and train_good_utils.py:387-426 for GIVEN sets."""
import importlib
import math

import numpy as np
import torch

import epipolar_ref as er
import sampler_ref as sr

MIN_DRAWS, MAX_DRAWS = 8, 32
CLAMP = 0.02  # the literal of train_good_utils.py:406


# ---- the draw ------------------------------------------------------------------------------------------------------------------------
def pick(t, P, n):
    lo, hi = 0, n  # the largest i < n with P[i] <= t
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if P[mid] <= t:
            lo = mid
        else:
            hi = mid
    return lo


def multiset(r, q, P, n, K):
    """r: the r64 of draws 0 .. K-1.  P None (no drawable weight, or no weights): uniform with replacement."""
    if P is None:
        return [(r[j] * n) >> 64 for j in range(K)]
    return [pick((r[j] * P[n]) >> 64, P, n) for j in range(K)]


def sample_multisets(B, N, H, K, seed, offset=0, counter=None, weights=None, n_valid=None, pairs=None, sets=None):
    """-> (idx [B,H,K] int32, fallback [B] int32, q per pair).  ``pairs`` / ``sets``: only these are computed (the others stay -1)."""
    off = sr.offset_of(offset, counter)
    ns = sr.valid_counts(B, N, K, n_valid)
    idx = np.full((B, H, K), -1, np.int32)
    fallback = np.zeros(B, np.int32)
    qs = [None] * B
    for b in (range(B) if pairs is None else pairs):
        n = ns[b]
        q = P = None
        if weights is not None:
            q = sr.quantise(np.asarray(weights, np.float32)[b, :n])
            qs[b] = q
            if not any(q):
                fallback[b] = 1
            else:
                P = sr.prefix(q)
        for h in (range(H) if sets is None else sets):
            idx[b, h] = multiset(sr.r64_draws(seed, off, b, h, K), q, P, n, K)
    return idx, fallback, qs


# ---- top-K ---------------------------------------------------------------------------------------------------------------------------
def topk(x, K, n_valid=None):
    """The K largest of x[b, :n] in descending order: NaN greatest, equal values (-0 = +0) lowest index first."""
    x = np.asarray(x, np.float32)
    B, N = x.shape
    ns = sr.valid_counts(B, N, K, n_valid)
    out = np.zeros((B, K), np.int32)
    for b in range(B):
        rows = [(0 if math.isnan(v) else 1, 0.0 if math.isnan(v) else -float(v), i) for i, v in enumerate(x[b, :ns[b]])]
        out[b] = [i for _, _, i in sorted(rows)[:K]]  # -(-0.0) == 0.0 == -(0.0) under Python's comparison: ties by index
    return out


# ---- gather and accu -----------------------------------------------------------------------------------------------------------------
def gather(pts1, pts2, weights, idx):
    B, H, K = idx.shape
    b = np.arange(B)[:, None, None]
    return (pts1[b, idx].reshape(B * H, K, 3), pts2[b, idx].reshape(B * H, K, 3), weights[b, idx].reshape(B * H, K))


def accu(weights, idx):
    """prod(1000 w) / (sum over the pair's sets + 1e-10) in float64 (DeepFNetSampleLoss.py:418-419).
    Bound of the device's float32 value: the device forms each product with K - 1 float64 roundings and the sum with at most H more,
    the quotient with one, and rounds to float32 once: |err| <= (2^-24 + (K + H + 2) 2^-53) accu, plus half a float32 denormal."""
    B, H, K = idx.shape
    w = np.asarray(weights, np.float64)[np.arange(B)[:, None, None], idx]
    p = np.prod(1000.0 * w, axis=2)
    a = p / (p.sum(1, keepdims=True) + 1e-10)
    return a, (2.0 ** -24 + (K + H + 2) * 2.0 ** -53) * np.abs(a) + 2.0 ** -150


# ---- fits ----------------------------------------------------------------------------------------------------------------------------
def fits(p1_sel, p2_sel, w_sel):
    """float64 fit of the gathered rows [B H,K,*] as the device wrote them -> F [B H,3,3] (LAPACK's sign)."""
    oracle = importlib.import_module("oracle.deepf_oracle")
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    return oracle.fit_forward(t(p1_sel), t(p2_sel), t(w_sel).unsqueeze(1))[0].numpy()


def fit_error(F_dev, F_ref):
    """Per problem: |F_dev / |F_dev| -+ F_ref / |F_ref||_F with the aligning sign (the gauge every fit test of this suite uses)."""
    a = F_dev.reshape(len(F_dev), 9).astype(np.float64)
    b = F_ref.reshape(len(F_ref), 9)
    a = a / np.linalg.norm(a, axis=1, keepdims=True)
    b = b / np.linalg.norm(b, axis=1, keepdims=True)
    s = np.sign((a * b).sum(1, keepdims=True))
    return np.linalg.norm(a * s - b, axis=1)


# ---- loss ----------------------------------------------------------------------------------------------------------------------------
def floss(F_sel, T1, T2, virt1, virt2, clamp_at=CLAMP):
    """F_sel float32 [B,H,3,3] -> the epipolar_ref.Ref with the sets in the place of the layers ([H,B,...])."""
    return er.floss_ref(np.ascontiguousarray(np.asarray(F_sel, np.float32).transpose(1, 0, 2, 3)), T1, T2, None, virt1, virt2, clamp_at)


# ---- scatter -------------------------------------------------------------------------------------------------------------------------
def scatter(g_w_sel, g_accu, weights, accu32, idx, N):
    """-> (g_w [B,N] float64, the sum of magnitudes per correspondence, occurrences [B,N])."""
    B, H, K = idx.shape
    g = np.zeros((B, N))
    mag = np.zeros((B, N))
    occ = np.zeros((B, N), np.int64)
    for b in range(B):
        G = 0.0 if g_accu is None else float((np.asarray(g_accu[b], np.float64) * np.asarray(accu32[b], np.float64)).sum())
        for h in range(H):
            for k in range(K):
                n = int(idx[b, h, k])
                v = 0.0 if g_w_sel is None else float(g_w_sel[b, h, k])
                if g_accu is not None and weights[b, n] != 0:
                    v += float(accu32[b, h]) * (float(g_accu[b, h]) - G) / float(weights[b, n])
                g[b, n] += v
                mag[b, n] += abs(v)
                occ[b, n] += 1
    return g, mag, occ


# ---- end to end, for given sets ------------------------------------------------------------------------------------------------------
def compute_epi_residual(pts1, pts2, F, clamp_at):
    l1 = pts2 @ F
    l2 = pts1 @ F.transpose(1, 2)
    dd = (pts1 * l1).sum(2)
    d = dd.abs() * (1 / (l1[:, :, :2].norm(dim=2) + 1e-6) + 1 / (l2[:, :, :2].norm(dim=2) + 1e-6))
    return torch.clamp(d, max=clamp_at)


def fit_selected(pts1, pts2, weights, idx, dtype=torch.float64):
    """out_sample_selected_batch [B,H,3,3] and weights_sample_selected_accu_batch [B,H,1] (DeepFNetSampleLoss.py:399-429) for GIVEN
    sets idx [B,H,K], in ``dtype``, differentiable in weights [B,N]."""
    oracle = importlib.import_module("oracle.deepf_oracle")
    B, H, K = idx.shape
    ix = torch.as_tensor(np.asarray(idx), dtype=torch.long)
    b = torch.arange(B)[:, None, None]
    p1, p2, w = pts1.to(dtype)[b, ix].reshape(B * H, K, 3), pts2.to(dtype)[b, ix].reshape(B * H, K, 3), weights[b, ix]
    F = oracle.fit_forward(p1, p2, w.reshape(B * H, 1, K))[0].reshape(B, H, 3, 3)
    p = torch.prod(w * 1000.0, dim=2, keepdim=True)
    return F, p / (p.sum(1, keepdim=True) + 1e-10)


def loss_selected(F_sel_layers, T1, T2, virt1, virt2):
    """loss_selected_F of train_good_utils.py:387-426: per layer and pair the mean over [H,M], then over pairs, then over layers."""
    dtype = F_sel_layers[0].dtype
    e1 = (T1.to(dtype) @ virt1.to(dtype).permute(0, 2, 1)).permute(0, 2, 1)
    e2 = (T2.to(dtype) @ virt2.to(dtype).permute(0, 2, 1)).permute(0, 2, 1)
    layers = []
    for F_sel in F_sel_layers:
        per_pair = [compute_epi_residual(e1[b:b + 1], e2[b:b + 1], F_sel[b], CLAMP).mean() for b in range(F_sel.shape[0])]
        layers.append(sum(per_pair) / len(per_pair))
    return sum(layers) / len(layers), layers
