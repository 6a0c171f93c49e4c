"""The shared cases of the device-side DSAC sampler and the one check(): what the kernel (tests/test_sampler_gpu.py) and the host build
of csrc/sampler_math.h (tests/test_sampler_ref_cpu.py) are both held to.  The arithmetic is integer arithmetic, so the check is
EQUALITY with the restatement tests/sampler_ref.py; on top of it every set is distinct, lies in [0, n), and in weighted mode
holds only indices with q > 0.  The restatement of a case is computed once per process and shared."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_ref as sr  # noqa: E402

F32 = np.float32
UNIFORM_SHAPES = ((1, 1, 8, 8), (1, 1, 9, 8), (2, 65, 10, 10), (3, 257, 100, 16), (1, 64, 2 ** 31 - 1, 16))  # (B, H, N, S)
SEEDS = (0, 1, 0xfedcba9876543210)
OFFSETS = ((0, None), (0xffffffff, 2))  # (offset, *counter): the second wraps to 1
N_VALID = (10, 7, 40, 45, 23)


def _case(name, B, H, N, S, seed=1, offset=0, counter=None, weights=None, n_valid=None, **extra):
    c = dict(name=name, B=B, H=H, N=N, S=S, seed=seed, offset=offset, counter=counter, n_valid=None if n_valid is None else
             np.asarray(n_valid, np.int32), weights=None if weights is None else np.ascontiguousarray(weights, F32))
    assert c["weights"] is None or c["weights"].shape == (B, N)
    c.update(extra)
    return c


def uniform_cases():
    out = [_case(f"uniform B{B} H{H} N{N} S{S} seed{seed:x} off{off:x}", B, H, N, S, seed, off, ctr)
           for (B, H, N, S) in UNIFORM_SHAPES for seed in SEEDS for (off, ctr) in OFFSETS]
    out.append(_case("n_valid", 5, 33, 40, 10, seed=5, n_valid=N_VALID))
    return out


def _positive(rng, *shape):
    return (rng.random(shape) ** 4 + 1e-3).astype(F32)


def weighted_cases(chunk):
    rng = np.random.default_rng(2024)
    S = 10
    out = [_case("weighted N=S", 2, 65, S, S, weights=_positive(rng, 2, S))]
    w = np.zeros((2, 40), F32)
    keep = [np.sort(rng.choice(40, S, replace=False)) for _ in range(2)]
    for b in range(2):
        w[b, keep[b]] = _positive(rng, S)
    out.append(_case("weighted exactly S positive", 2, 65, 40, S, weights=w, expect_sets=keep))
    w1 = w.copy()
    w1[1, keep[1][3]] = 0.0  # pair 1: S - 1 positive
    out.append(_case("weighted S-1 positive", 2, 65, 40, S, weights=w1, expect_fallback=[0, 1]))
    w = _positive(rng, 2, 40)
    w[:, 3], w[:, 9], w[:, 17], w[:, 21], w[:, 30] = 0.0, -1.0, np.nan, np.inf, F32(1e-42)
    w[1, 4] = -np.inf
    out.append(_case("weighted 0 -1 nan inf denormal", 2, 65, 40, S, weights=w, expect_q={3: 0, 9: 0, 17: 0, 21: 0, 30: 0}))
    for m in (F32(1.0), F32(0.99999994)):  # the frexp boundary: 1.0 = 0.5 2^1, 0.99999994 = (1 - 2^-24) 2^0
        w = (_positive(rng, 2, 40) * F32(0.5)).astype(F32)
        w[:, 11] = m
        q11 = int(m * 2 ** 29) if m == 1.0 else (1 << 30) - 64
        out.append(_case(f"weighted max {float(m)!r}", 2, 65, 40, S, weights=w, expect_q={11: q11}))
    w = _positive(rng, 2, 40)
    m = F32(w.max() * 2)
    w[:, 0], w[:, 7], w[:, 8] = m, m * F32(2.0 ** -29), m * F32(2.0 ** -30)
    e = int(np.frexp(m)[1])
    out.append(_case("weighted q=1 and q=0", 2, 65, 40, S, weights=w,
                     expect_q={7: int(np.floor(np.ldexp(float(w[0, 7]), 30 - e))), 8: int(np.floor(np.ldexp(float(w[0, 8]), 30 - e)))}))
    assert out[-1]["expect_q"] in ({7: 1, 8: 0},)  # m is a power of two times f >= 0.5: f 2 -> 1, f -> 0 for f < 1
    for N in (chunk - 1, chunk, chunk + 1, 2 * chunk + 1):
        w = _positive(rng, 2, N)
        w[:, ::7] = 0.0
        out.append(_case(f"weighted N={N} (chunk {chunk})", 2, 65, N, 16, seed=3, weights=w))
    out.append(_case("weighted N=2^20", 1, 64, 1 << 20, 16, seed=4, weights=_positive(rng, 1, 1 << 20)))
    w = _positive(rng, 5, 40)
    w[1, 2] = 0.0  # pair 1: n = clamp(7) = 10, nine positive among them, thirty beyond: falls back
    out.append(_case("weighted with n_valid", 5, 33, 40, S, seed=6, weights=w, n_valid=N_VALID, expect_fallback=[0, 1, 0, 0, 0]))
    return out


def all_cases(chunk):
    return uniform_cases() + weighted_cases(chunk)


_REF = {}


def reference(case):
    key = case["name"]
    if key not in _REF:
        idx, fb, qs = sr.sample_sets(case["B"], case["N"], case["H"], case["S"], case["seed"], case["offset"], case["counter"],
                                     case["weights"], case["n_valid"])
        idx.setflags(write=False)
        fb.setflags(write=False)
        _REF[key] = (idx, fb, qs)
    return _REF[key]


def check(got_idx, got_fallback, case):
    B, H, N, S = case["B"], case["H"], case["N"], case["S"]
    idx, fb, qs = reference(case)
    got_idx, got_fallback = np.asarray(got_idx), np.asarray(got_fallback)
    assert got_idx.shape == (B, H, S) and got_idx.dtype == np.int32 and got_fallback.shape == (B,), case["name"]
    assert np.array_equal(got_fallback, fb), (case["name"], got_fallback, fb)
    assert np.array_equal(got_idx, idx), (case["name"], np.argwhere(got_idx != idx)[:4])
    ns = sr.valid_counts(B, N, S, case["n_valid"])
    for b in range(B):
        s = np.sort(got_idx[b].astype(np.int64), axis=1)
        assert s.min() >= 0 and s.max() < ns[b], case["name"]
        assert (np.diff(s, axis=1) > 0).all(), case["name"]
        if case["weights"] is not None and not fb[b]:
            assert (np.asarray(qs[b], np.int64)[got_idx[b]] > 0).all(), case["name"]
            assert 2 ** 29 <= max(qs[b]) < 2 ** 30, case["name"]
    # what the case says about itself, so that a restatement that is wrong the same way as the code is still caught
    if case["weights"] is None:
        assert not fb.any(), case["name"]
    if "expect_fallback" in case:
        assert fb.tolist() == case["expect_fallback"], case["name"]
    for b, keep in enumerate(case.get("expect_sets", ())):
        assert (np.sort(got_idx[b], axis=1) == keep[None]).all(), case["name"]
    for i, q in case.get("expect_q", {}).items():
        assert all(qb[i] == q for qb in qs), (case["name"], i, q, [qb[i] for qb in qs])
