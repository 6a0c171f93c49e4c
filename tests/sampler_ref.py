"""The device-side DSAC sampler (dfepe_sample_sets, include/dfepe.h) restated in Python integers and numpy, from the
specification and not from csrc/sampler_math.h: Philox4x32-10, the streams, Floyd's subset algorithm, the quantisation through
math.frexp / math.ldexp, the prefix sums and the weighted pick.  Everything is exact integer arithmetic, so the kernel and the host
build of the header are held to EQUALITY with what is here."""
import math

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32, MASK64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
QUANT_BITS = 30
MIN_SAMPLE, MAX_SAMPLE = 8, 16
MAX_WEIGHTED_N = 1 << 20

# Known-answer vectors of the Random123 distribution (kat_vectors, philox4x32 10): counter, key -> output
KAT = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((MASK32,) * 4, (MASK32,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))


def philox4x32_10(counter, key):
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c0, c1, c2, c3


def r64_draws(seed, off, b, h, S):
    """r64 of the draws 0 .. S-1 of hypothesis h of pair b: word[2j+1] << 32 | word[2j], block k = the words 4k .. 4k+3."""
    key = (seed & MASK32, (seed >> 32) & MASK32)
    words = []
    for k in range((2 * S + 3) // 4):
        words.extend(philox4x32_10((k, h, b, off & MASK32), key))
    return [(words[2 * j + 1] << 32) | words[2 * j] for j in range(S)]


def floyd(r, n, S):
    out = []
    for i in range(S):
        j = n - S + i
        t = (r[i] * (j + 1)) >> 64
        out.append(j if t in out else t)
    return out


def quantise(w):
    """w: the float32 weights of the correspondences that can be drawn (the first n) -> q as Python integers."""
    w = [float(x) for x in np.asarray(w, np.float32)]
    ok = [not (math.isnan(x) or math.isinf(x) or x <= 0.0) for x in w]
    if not any(ok):
        return [0] * len(w)
    m = max(x for x, k in zip(w, ok) if k)
    _, e = math.frexp(m)
    return [int(math.floor(math.ldexp(x, QUANT_BITS - e))) if k else 0 for x, k in zip(w, ok)]


def prefix(q):
    P = [0]
    for x in q:
        P.append(P[-1] + x)
    return P


def weighted(r, q, P, S):
    n = len(q)
    chosen, out = [], []
    for k in range(S):
        total = P[n] - sum(q[c] for c in chosen)
        t = (r[k] * total) >> 64
        rem = 0
        for c in sorted(chosen):
            if t + rem >= P[c]:
                rem += q[c]
            else:
                break
        u = t + rem
        lo, hi = 0, n  # the largest i < n with P[i] <= u
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if P[mid] <= u:
                lo = mid
            else:
                hi = mid
        chosen.append(lo)
        out.append(lo)
    return out


def offset_of(offset, counter):
    return (offset + (0 if counter is None else counter)) & MASK32


def valid_counts(B, N, S, n_valid):
    return [N] * B if n_valid is None else [min(max(int(v), S), N) for v in n_valid]


def sample_sets(B, N, H, S, seed, offset=0, counter=None, weights=None, n_valid=None, pairs=None, hyps=None):
    """-> (idx [B,H,S] int32, fallback [B] int32, q: per pair the list of q or None).  ``pairs`` / ``hyps``: only these are computed
    (the others stay -1): a set depends on its own (b, h) alone."""
    off = offset_of(offset, counter)
    ns = valid_counts(B, N, S, n_valid)
    idx = np.full((B, H, S), -1, np.int32)
    fallback = np.zeros(B, np.int32)
    qs = [None] * B
    for b in (range(B) if pairs is None else pairs):
        n = ns[b]
        q = P = None
        if weights is not None:
            q = quantise(np.asarray(weights, np.float32)[b, :n])
            qs[b] = q
            if sum(1 for x in q if x > 0) < S:
                fallback[b] = 1
            else:
                P = prefix(q)
        for h in (range(H) if hyps is None else hyps):
            r = r64_draws(seed, off, b, h, S)
            idx[b, h] = floyd(r, n, S) if P is None else weighted(r, q, P, S)
    return idx, fallback, qs
