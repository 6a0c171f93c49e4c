"""The Hartley record of the forward fit (csrc/w8pt16_body.h: HM; dfepe_w8pt_fwd_shared), without a GPU.

Layer 1 of a step that fits the same matches at every layer writes the six fp64 values of Fit.normalize -- two centroids, two
scales -- and layers 2..L read them instead of computing them.  The kernel body is compiled for the host against the row-group
emulation of tests/emu/ (tests/emu/emu_w8pt16_hartley.cpp) and run plain, writing and reading: every output byte must be the same
in the three modes, the written values must be Fit.normalize's, and a record nobody wrote must poison the fit.  The C entry points
are checked for their host-side validation and for the rule that says which shapes take the record (csrc/fit_plan.h)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EMU_DIR = os.path.join(REPO, "tests", "emu")
IMAGE_SIZE = [376, 1241, 3]
RAW, LOGITS, SQRT2, NO_HARTLEY = 1, 2, 4, 32
NONE, WRITE, READ = 0, 1, 2
SAVE_FLOATS, HARTLEY_DOUBLES = 128, 8
ROW, ROW_LEAN, PAIR2, COOP = 0, 1, 2, 3
P, I, U, F32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_float


@pytest.fixture(scope="module")
def emu():
    """Built like tests/test_emu_cpu.py builds its library, from the source that includes that library's own."""
    out = os.path.join(EMU_DIR, "_build")
    os.makedirs(out, exist_ok=True)
    lib = os.path.join(out, "libemu_w8pt16_hartley.so")
    srcs = [os.path.join(EMU_DIR, f) for f in ("emu_w8pt16_hartley.cpp", "emu_w8pt16.cpp", "rowgroup.h")] + [
        os.path.join(REPO, "pytorch-deepfepe_amd", "csrc", f)
        for f in ("w8pt16_body.h", "w8pt16_bwd_body.h", "loss_tail_body.h", "pose_math.h", "dfepe_math.h", "fit_plan.h")] + [
        os.path.join(REPO, "include", "dfepe.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", f"-I{EMU_DIR}", f"-I{REPO}/pytorch-deepfepe_amd/csrc",
                        f"-I{REPO}/include", srcs[0], "-o", lib], check=True)
    L = ctypes.CDLL(lib)
    L.emu_w8pt16_fwd_shared.restype = I
    L.emu_w8pt16_fwd_shared.argtypes = [P, P, P, I, I, I, U, F32, F32, F32, P, P, P, P, P, P, I, I]
    L.emu_fit_shares_hartley.restype = I
    L.emu_fit_shares_hartley.argtypes = [I, U]
    L.emu_fit_plan.restype = None
    L.emu_fit_plan.argtypes = [I] * 11 + [ctypes.POINTER(I)]
    return L


def _p(t):
    return None if t is None else t.data_ptr()


def _bits(t):
    return t.contiguous().view(torch.int32)  # byte equality, NaN payloads included


def _inputs(B, N, raw, logits, seed, nan_pair=None):
    """B pairs of N correspondences: pixel matches [B,N,4] or homogeneous points [B,N,3] x 2 (third coordinate not always 1, as the
    body uses it), logits or positive weights.  ``nan_pair``: that pair gets one correspondence with a NaN coordinate."""
    g = torch.Generator().manual_seed(seed)
    H, W = float(IMAGE_SIZE[0]), float(IMAGE_SIZE[1])
    if raw:
        pts1 = torch.rand(B, N, 4, generator=g) * torch.tensor([W, H, W, H])
        pts2 = None
    else:
        pts1 = torch.cat((torch.rand(B, N, 2, generator=g) * 2 - 1, 1.0 + 0.05 * torch.randn(B, N, 1, generator=g)), 2).contiguous()
        pts2 = torch.cat((torch.rand(B, N, 2, generator=g) * 2 - 1, 1.0 + 0.05 * torch.randn(B, N, 1, generator=g)), 2).contiguous()
    if nan_pair is not None:
        pts1[nan_pair, N // 2, 1] = float("nan")
    w = torch.randn(B, N, generator=g) if logits else torch.rand(B, N, generator=g) + 0.05
    return pts1, pts2, w


def _run(L, pts1, pts2, w, flags, mode, record, lean=False, want_save=True, n_sets=1):
    """One emulated launch of dfepe_w8pt_fwd_shared: (F, residual, epi, weights_out | None, save | None)."""
    N = w.shape[-1]
    B = pts1.shape[0]
    F = torch.full((n_sets * B, 9), 7.0)
    res = torch.full((n_sets * B, N), 7.0)
    epi = torch.full((n_sets * B, N), 7.0)
    wout = torch.full((n_sets * B, N), 7.0) if flags & LOGITS else None
    save = torch.full((n_sets * B, SAVE_FLOATS), 7.0) if want_save else None
    rc = L.emu_w8pt16_fwd_shared(_p(pts1), _p(pts2), _p(w), B, N, n_sets, flags, float(IMAGE_SIZE[1]), float(IMAGE_SIZE[0]), 0.5,
                                 _p(F), _p(res), _p(epi), _p(save), _p(wout), _p(record), mode, int(lean))
    assert rc == 0
    return F, res, epi, wout, save


def _assert_same_bytes(a, b, what):
    for name, x, y in zip(("F", "residual", "epi", "weights_out", "save"), a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert torch.equal(_bits(x), _bits(y)), f"{what}: {name} differs in {int((_bits(x) != _bits(y)).sum())} words"


def _restated(pts1, pts2, raw, scale):
    """Fit.normalize in fp64 torch on the coordinates as the body holds them (fp32, a dropped correspondence zeroed): centroid =
    mean, s = scale / mean distance to the centroid.  Returns [B, 6]: c1x, c1y, s1, c2x, c2y, s2."""
    H, W = float(IMAGE_SIZE[0]), float(IMAGE_SIZE[1])
    if raw:
        sx, sy = np.float32(2.0) / np.float32(W), np.float32(2.0) / np.float32(H)
        s4 = torch.tensor([sx, sy, sx, sy], dtype=torch.float64)
        xy = (pts1.double() * s4 - 1.0).float()  # fmaf(v, 2 / W, -1) in fp32: the product is exact in fp64, one rounding
        keep = torch.isfinite(xy).all(dim=2) & (xy.abs().sum(dim=2) < 1e18)
        a, b = xy[..., 0:2], xy[..., 2:4]
    else:
        both = torch.cat((pts1, pts2), 2)
        keep = torch.isfinite(both).all(dim=2) & (both.abs().sum(dim=2) < 1e18)
        a, b = pts1[..., 0:2], pts2[..., 0:2]
    out = []
    for q in (a, b):
        q = torch.where(keep[..., None], q, torch.zeros_like(q)).double()
        c = q.mean(dim=1)
        d = (q - c[:, None, :]).norm(dim=2).mean(dim=1)
        out += [c[:, 0], c[:, 1], scale / d]
    return torch.stack(out, dim=1)


N_EDGES = [8, 9, 16, 17, 33, 100, 112, 113, 128]
CASES = [(N, raw, logits, lean) for N in N_EDGES for raw in (1, 0) for logits in (1, 0) for lean in ((False, True) if N > 64 else (False,))]


@pytest.mark.parametrize("N,raw,logits,lean", CASES)
def test_write_and_read_runs_equal_the_plain_run_byte_for_byte(emu, N, raw, logits, lean):
    """Every rung of the N ladder and both sides of each edge, the resident and the lean body (the library has a lean build for 7 and 8
    correspondences per lane), pixel matches and homogeneous points, logits and plain weights; pair 1 has a NaN correspondence."""
    B = 3
    flags = (RAW if raw else 0) | (LOGITS if logits else 0)
    pts1, pts2, w = _inputs(B, N, raw, logits, seed=1000 + N, nan_pair=1)
    plain = _run(emu, pts1, pts2, w, flags, NONE, None, lean)
    assert torch.isfinite(plain[0]).all() and torch.isfinite(plain[1]).all()  # the NaN correspondence was dropped, not spread
    record = torch.full((B, HARTLEY_DOUBLES), 3.0, dtype=torch.float64)
    wrote = _run(emu, pts1, pts2, w, flags, WRITE, record, lean)
    _assert_same_bytes(wrote, plain, "write")
    # the six values are Fit.normalize's (literal 1.4142), slot 6 is zero, slot 7 the tag
    want = _restated(pts1, pts2, raw, 1.4142)
    got = record[:, [0, 1, 2, 3, 4, 5]]
    rel = ((got - want).abs() / want.abs()).max().item()
    print(f"N={N} raw={raw}: written values vs fp64 restatement: max relative difference {rel:.2e}")
    assert rel <= 1e-12
    assert (record[:, 6] == 0.0).all() and (record[:, 7] == record[0, 7]).all() and record[0, 7] != 0.0
    # a reader with OTHER weights (the next layer's) equals the plain run on those weights
    w2 = torch.roll(w, 1, dims=1) * 0.5 if logits else torch.roll(w, 1, dims=1)
    plain2 = _run(emu, pts1, pts2, w2, flags, NONE, None, lean)
    kept = record.clone()
    read2 = _run(emu, pts1, pts2, w2, flags, READ, record, lean)
    _assert_same_bytes(read2, plain2, "read")
    assert torch.equal(record, kept)  # a reader leaves the record alone
    _assert_same_bytes(_run(emu, pts1, pts2, w, flags, READ, record, lean), plain, "read, the writer's weights")


def test_centroid_values_to_1e12_relative(emu):
    """The same bound on data whose centroids are far from zero (pixel matches in one image corner)."""
    B, N = 4, 100
    g = torch.Generator().manual_seed(5)
    pts1 = (torch.rand(B, N, 4, generator=g) * 0.3 + 0.6) * torch.tensor([1241.0, 376.0, 1241.0, 376.0])
    w = torch.randn(B, N, generator=g)
    record = torch.zeros(B, HARTLEY_DOUBLES, dtype=torch.float64)
    _run(emu, pts1, None, w, RAW | LOGITS, WRITE, record)
    want = _restated(pts1, None, True, 1.4142)
    rel = ((record[:, :6] - want).abs() / want.abs()).max().item()
    print(f"written values vs fp64 restatement, max relative difference {rel:.2e}")
    assert rel <= 1e-12


@pytest.mark.parametrize("raw", [1, 0])
def test_sqrt2_scale_is_handed_on_as_it_is(emu, raw):
    """DFEPE_W8PT_SQRT2 (forward only: no save record): the writer's sqrt(2) scale reaches the reader unchanged."""
    B, N = 2, 100
    flags = (RAW if raw else 0) | SQRT2
    pts1, pts2, w = _inputs(B, N, raw, 0, seed=77)
    plain = _run(emu, pts1, pts2, w, flags, NONE, None, want_save=False)
    record = torch.zeros(B, HARTLEY_DOUBLES, dtype=torch.float64)
    _assert_same_bytes(_run(emu, pts1, pts2, w, flags, WRITE, record, want_save=False), plain, "write")
    want = _restated(pts1, pts2, raw, float(np.sqrt(2.0)))
    assert ((record[:, [2, 5]] - want[:, [2, 5]]).abs() / want[:, [2, 5]]).max().item() <= 1e-12
    lit = _restated(pts1, pts2, raw, 1.4142)
    assert ((record[:, [2, 5]] - lit[:, [2, 5]]).abs() / lit[:, [2, 5]]).min().item() > 1e-6  # and it is not the literal
    _assert_same_bytes(_run(emu, pts1, pts2, w, flags, READ, record, want_save=False), plain, "read")


def test_several_weight_sets_read_one_record(emu):
    """n_weight_sets = 3: the record is indexed by pair % B like the correspondences; the writer of a one-set launch serves them all."""
    B, N, S = 3, 33, 3
    pts1, _, w1 = _inputs(B, N, 1, 1, seed=9)
    w = torch.randn(S, B, N, generator=torch.Generator().manual_seed(10))
    record = torch.zeros(B, HARTLEY_DOUBLES, dtype=torch.float64)
    _run(emu, pts1, None, w1, RAW | LOGITS, WRITE, record)
    plain = _run(emu, pts1, None, w, RAW | LOGITS, NONE, None, n_sets=S)
    _assert_same_bytes(_run(emu, pts1, None, w, RAW | LOGITS, READ, record, n_sets=S), plain, "read, three weight sets")
    # a writer with three sets leaves the same record
    again = torch.zeros(B, HARTLEY_DOUBLES, dtype=torch.float64)
    _assert_same_bytes(_run(emu, pts1, None, w, RAW | LOGITS, WRITE, again, n_sets=S), plain, "write, three weight sets")
    assert torch.equal(again, record)


@pytest.mark.parametrize("lean", [False, True])
def test_a_record_nobody_wrote_poisons_the_fit(emu, lean):
    """Zero-filled record (tag 0): s1 becomes NaN, and with it F and the residual of every pair -- the convention of the save record.
    (The epipolar residual is min(|x2 F x1| (...), clamp): fminf drops the NaN, so it comes out as the clamp, not as a number that
    looks like a residual.)"""
    B, N = 2, 100
    pts1, _, w = _inputs(B, N, 1, 1, seed=3)
    F, res, epi, _, _ = _run(emu, pts1, None, w, RAW | LOGITS, READ, torch.zeros(B, HARTLEY_DOUBLES, dtype=torch.float64), lean)
    assert torch.isnan(F).all() and torch.isnan(res).all()
    assert (torch.isnan(epi) | (epi == 0.5)).all()
    # a record of the right values with another tag: the same
    record = torch.zeros(B, HARTLEY_DOUBLES, dtype=torch.float64)
    _run(emu, pts1, None, w, RAW | LOGITS, WRITE, record, lean)
    record[:, 7] += 1.0
    F, res, _, _, _ = _run(emu, pts1, None, w, RAW | LOGITS, READ, record, lean)
    assert torch.isnan(F).all() and torch.isnan(res).all()


def test_no_hartley_ignores_both_modes(emu):
    """DFEPE_W8PT_NO_HARTLEY: nothing is written, nothing is read, the launch is the plain one."""
    B, N = 2, 33
    pts1, pts2, w = _inputs(B, N, 0, 0, seed=4)
    plain = _run(emu, pts1, pts2, w, NO_HARTLEY, NONE, None, want_save=False)
    record = torch.full((B, HARTLEY_DOUBLES), 5.0, dtype=torch.float64)
    _assert_same_bytes(_run(emu, pts1, pts2, w, NO_HARTLEY, WRITE, record, want_save=False), plain, "write")
    assert (record == 5.0).all()
    _assert_same_bytes(_run(emu, pts1, pts2, w, NO_HARTLEY, READ, torch.zeros(B, HARTLEY_DOUBLES, dtype=torch.float64), want_save=False),
                       plain, "read")


def _plan(L, N, pairs, raw, row_per_pair, force_lean=-1, force_pair2=-1):
    out = (I * 5)()
    L.emu_fit_plan(0, N, pairs, raw, row_per_pair, 0, 1, 0, force_lean, force_pair2, 0, out)
    return out[0], out[1]


def test_the_rule_is_one_for_every_pair_count_and_names_kernels_that_take_the_record(emu, dfepe):
    """fit_shares_hartley knows N and the flags only: the same answer at every pair count and under every forced switch, so a writer
    and its readers agree -- and wherever it says yes, the forward plan is a registers-resident row kernel (the only kernels that
    take the record); the library's dfepe_w8pt_shares_hartley states the same rule."""
    lib = dfepe._lib.lib()
    for N in (1, 8, 9, 16, 17, 32, 33, 64, 65, 100, 112, 113, 128, 129, 256, 1000, 2048, 2049):
        want = 1 if N <= 128 else 0
        assert emu.emu_fit_shares_hartley(N, 0) == want and lib.dfepe_w8pt_shares_hartley(N, 0) == want
        for flags in (RAW, LOGITS, SQRT2, RAW | LOGITS | 64):
            assert emu.emu_fit_shares_hartley(N, flags) == want and lib.dfepe_w8pt_shares_hartley(N, flags) == want
        assert emu.emu_fit_shares_hartley(N, NO_HARTLEY) == 0 and lib.dfepe_w8pt_shares_hartley(N, NO_HARTLEY | RAW) == 0
        for pairs in (1, 16, 17, 1280, 1281, 3072, 3073, 4096, 8191, 8192, 12287, 12288, 32768):
            for raw in (0, 1):
                for rpp in (0, 1):
                    for fl, fp in ((-1, -1), (0, 0), (1, 1)):
                        kind, it = _plan(emu, N, pairs, raw, rpp, fl, fp)
                        assert (kind in (ROW, ROW_LEAN) and it > 0) == bool(want), (N, pairs, raw, rpp, fl, fp, kind, it)


def test_shares_hartley_entry_point(dfepe):
    lib = dfepe._lib.lib()
    assert lib.dfepe_w8pt_shares_hartley(100, 0) == 1
    assert lib.dfepe_w8pt_shares_hartley(129, 0) == 0
    assert lib.dfepe_w8pt_shares_hartley(100, NO_HARTLEY) == 0
    assert lib.dfepe_w8pt_shares_hartley(128, RAW | LOGITS) == 1 and lib.dfepe_w8pt_shares_hartley(0, 0) == 0
    assert dfepe._lib.HARTLEY_DOUBLES == 8 and (dfepe._lib.HARTLEY_NONE, dfepe._lib.HARTLEY_WRITE, dfepe._lib.HARTLEY_READ) == (0, 1, 2)
    assert lib.dfepe_version() == 154


def test_shared_entry_point_validates_on_the_host(dfepe):
    """Before any HIP call (there is no GPU here): a mode outside 0..2, a non-zero mode with a NULL or misaligned record: -1; B = 0: 0."""
    lib = dfepe._lib.lib()
    buf = np.zeros(64, dtype=np.float64)
    base = buf.ctypes.data
    aligned = (base + 63) & ~63
    m = np.zeros((1, 8, 4), dtype=np.float32)
    mp = (m.ctypes.data + 15) & ~15

    def call(B, hartley, mode, N=8, flags=RAW | LOGITS):
        return lib.dfepe_w8pt_fwd_shared(mp, None, mp, B, N, 1, flags, 1241.0, 376.0, 0.5, mp, mp, None, None, None, hartley, mode, None)

    for mode in (-1, 3, 17):
        assert call(0, aligned, mode) == -1 and call(0, None, mode) == -1
    for mode in (WRITE, READ):
        assert call(0, None, mode) == -1
        for off in (8, 16, 32, 56):
            assert call(0, aligned + off, mode) == -1
        assert call(0, aligned, mode) == 0       # B = 0: nothing to do
        assert call(0, aligned, mode, N=1000) == 0
        assert call(-1, aligned, mode) == -1     # ... and the checks of dfepe_w8pt_fwd still hold
    assert call(0, None, NONE) == 0 and call(0, aligned + 8, NONE) == 0  # mode 0: the record is ignored
    assert call(-1, None, NONE) == -1
    # dfepe_w8pt_fwd itself is what it was
    assert lib.dfepe_w8pt_fwd(mp, None, mp, 0, 8, 1, RAW, 1241.0, 376.0, 0.5, mp, mp, None, None, None, None) == 0
    assert lib.dfepe_w8pt_fwd(mp, None, mp, -1, 8, 1, RAW, 1241.0, 376.0, 0.5, mp, mp, None, None, None, None) == -1
