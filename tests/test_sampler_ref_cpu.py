"""The device-side DSAC sampler without a GPU: the Philox known-answer vectors through the restatement (tests/sampler_ref.py) and
through the host build of csrc/sampler_math.h (tests/emu/emu_sampler.cpp), every shared case of tests/sampler_cases.py through the
same check() as the GPU, and two chi-square checks of the restatement's laws with fixed seeds (deterministic)."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_cases as sc  # noqa: E402
import sampler_ref as sr  # noqa: E402

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EMU_DIR = os.path.join(REPO, "tests", "emu")
CSRC = os.path.join(REPO, "pytorch-deepfepe_amd", "csrc")


@pytest.fixture(scope="module")
def emu():
    out = os.path.join(EMU_DIR, "_build")
    os.makedirs(out, exist_ok=True)
    lib, srcs = os.path.join(out, "libemu_sampler.so"), [os.path.join(EMU_DIR, "emu_sampler.cpp"), os.path.join(CSRC, "sampler_math.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", f"-I{CSRC}", srcs[0], "-o", lib], check=True)
    L = ctypes.CDLL(lib)
    i, p, u, u64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_uint, ctypes.c_ulonglong
    L.emu_philox4x32_10.argtypes, L.emu_philox4x32_10.restype = [p, p, p], None
    L.emu_sampler_scan.argtypes, L.emu_sampler_scan.restype = [p, p, i, i, i, p], None
    L.emu_sampler_draw.argtypes, L.emu_sampler_draw.restype = [i, i, i, i, u64, u, p, p, p, p, p], None
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def run_emu(L, case):
    B, H, N, S = case["B"], case["H"], case["N"], case["S"]
    idx, fb = np.full((B, H, S), -1, np.int32), np.full(B, -1, np.int32)
    ws = None
    if case["weights"] is not None:
        ws = np.full((B, N + 2), 2 ** 64 - 1, np.uint64)
        L.emu_sampler_scan(_p(case["weights"]), _p(case["n_valid"]), B, N, S, _p(ws))
    ctr = None if case["counter"] is None else np.array([case["counter"]], np.uint32)
    L.emu_sampler_draw(B, N, H, S, case["seed"], case["offset"], _p(ctr), _p(ws), _p(case["n_valid"]), _p(idx), _p(fb))
    return idx, fb


def test_philox_known_answers(emu):
    for counter, key, want in sr.KAT:
        assert sr.philox4x32_10(counter, key) == want
        c, k, out = np.array(counter, np.uint32), np.array(key, np.uint32), np.zeros(4, np.uint32)
        emu.emu_philox4x32_10(_p(c), _p(k), _p(out))
        assert tuple(int(x) for x in out) == want


def test_streams_are_the_specified_words():
    """Draw j of (b, h) is word[2j+1] << 32 | word[2j] of the blocks (k, h, b, off) under the key (seed lo, seed hi)."""
    seed, off, b, h = 0xfedcba9876543210, 7, 3, 5
    r = sr.r64_draws(seed, off, b, h, 10)
    blk = [sr.philox4x32_10((k, h, b, off), (0x76543210, 0xfedcba98)) for k in range(5)]
    assert r[0] == blk[0][1] << 32 | blk[0][0] and r[1] == blk[0][3] << 32 | blk[0][2] and r[9] == blk[4][3] << 32 | blk[4][2]
    assert sr.offset_of(0xffffffff, 2) == 1 and sr.offset_of(5, None) == 5


def test_host_build_passes_the_check(emu):
    chunk = emu.emu_sampler_scan_chunk()
    assert chunk >= 64
    for case in sc.all_cases(chunk):
        sc.check(*run_emu(emu, case), case)


def test_host_quantisation_is_frexp_ldexp(emu):
    """The header shifts significands; the restatement calls math.frexp / math.ldexp.  Pairs whose largest weight is a denormal, the
    smallest and the largest normal float, and powers of two on either side of the exponent boundary."""
    rows = [[1e-45, 3e-45, 1e-42, 0.0] + [2e-45] * 8, [1.17549435e-38, 1e-40, 1e-44, 5.9e-39] + [1e-38] * 8,
            [3.4028235e38, 1e30, 3.4e38, 1.0] + [2e38] * 8, [0.5, 0.25, 0.49999997, 2.0 ** -31] + [0.3] * 8,
            [2.0 ** -126, 2.0 ** -127, 2.0 ** -149, 2.0 ** -140] + [2.0 ** -130] * 8]
    w = np.array(rows, np.float32)
    B, N = w.shape
    ws = np.zeros((B, N + 2), np.uint64)
    emu.emu_sampler_scan(_p(w), None, B, N, 8, _p(ws))
    for b in range(B):
        q = sr.quantise(w[b])
        assert 2 ** 29 <= max(q) < 2 ** 30
        assert [int(x) for x in ws[b, :N + 1]] == sr.prefix(q) and int(ws[b, N + 1]) == sum(1 for x in q if x > 0), b


CHI2_999 = {49: 85.35, 35: 66.62}  # the 99.9 % quantiles of chi-square


def test_uniform_inclusion_counts():
    """N = 50, S = 10, seed 1234, offset 0, b = 0, h = 0 .. 19999: every index is included with probability S / N; the counts of a
    without-replacement sample have variance e (N - S) / N, hence the correction.  58.56 at 49 degrees of freedom."""
    N, S, hyps = 50, 10, 20000
    c = np.zeros(N)
    for h in range(hyps):
        for i in sr.floyd(sr.r64_draws(1234, 0, 0, h, S), N, S):
            c[i] += 1
    e = hyps * S / N
    stat = ((c - e) ** 2 / e).sum() * N / (N - S)
    print(f"uniform inclusion counts: chi2 = {stat:.2f} at {N - 1} dof (bound {CHI2_999[N - 1]})")
    assert stat < CHI2_999[N - 1]


def test_weighted_first_draw_marginal():
    """The first draw of a weighted hypothesis against q / sum q.  29.15 at 35 degrees of freedom (36 drawable weights)."""
    rng = random.Random(3)
    w = [rng.random() ** 4 for _ in range(40)]
    w[5:9] = [0.0, float("nan"), -1.0, 1e-12]
    q = sr.quantise(w)
    P = sr.prefix(q)
    assert [q[i] for i in range(5, 9)] == [0, 0, 0, 0]
    c = np.zeros(40)
    hyps = 20000
    for h in range(hyps):
        c[sr.weighted(sr.r64_draws(9, 1, 0, h, 8), q, P, 8)[0]] += 1
    qa = np.array(q, float)
    pos = qa > 0
    e = hyps * qa[pos] / qa.sum()
    stat = ((c[pos] - e) ** 2 / e).sum()
    dof = int(pos.sum()) - 1
    print(f"weighted first draw: chi2 = {stat:.2f} at {dof} dof (bound {CHI2_999[dof]})")
    assert c[~pos].sum() == 0 and stat < CHI2_999[dof]
