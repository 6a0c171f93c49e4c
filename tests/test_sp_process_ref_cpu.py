"""The restatement of the SuperPoint output processing (tests/sp_process_ref.py) against brute-force definitions, and the host
build of csrc/sp_process_math.h (tests/emu/emu_sp_process.cpp, a stand-alone program; also built with the address and
undefined-behaviour sanitizers) against the restatement: the round rule of the NMS fixpoint, the patch arithmetic and its
adjoint, the bilinear taps, the softmax and its adjoint.  No GPU."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sp_process_cases as sc  # noqa: E402
import sp_process_ref as sr  # noqa: E402

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(REPO, "pytorch-deepfepe_amd", "csrc")
EMU_DIR = os.path.join(REPO, "tests", "emu")


def _build(name, extra):
    out = os.path.join(EMU_DIR, "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, name)
    srcs = [os.path.join(EMU_DIR, "emu_sp_process.cpp"), os.path.join(CSRC, "sp_process_math.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", *extra, f"-I{CSRC}", srcs[0], "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def emu():
    return _build("emu_sp_process", [])


def run_emu(exe, payload, tmp_path, tag="io"):
    fin, fout = tmp_path / f"{tag}.in", tmp_path / f"{tag}.out"
    fin.write_bytes(payload)
    subprocess.run([exe, str(fin), str(fout)], check=True)
    return fout.read_bytes()


def _nms_record(heat, d, r):
    H, W = heat.shape
    return struct.pack("<5if", 1, H, W, d, r, sc.THR) + heat.astype("<f4").tobytes()


def _read_nms(buf, off, H, W):
    rounds, count = struct.unpack_from("<2i", buf, off)
    off += 8
    m = np.frombuffer(buf, np.uint8, H * W, off).reshape(H, W)
    off += H * W
    pts = np.frombuffer(buf, "<i4", 2 * count, off).reshape(count, 2)
    off += 8 * count
    conf = np.frombuffer(buf, "<f4", count, off)
    return rounds, m, pts, conf, off + 4 * count


# ---- the restatement against definitions ---------------------------------------------------------------------------------
@pytest.mark.parametrize("d", sc.NMS_DISTS)
@pytest.mark.parametrize("r", sc.BORDERS)
def test_nms_fast_is_the_greedy_definition(d, r):
    H, W = sc.SHAPES[0]
    for name, heat in sc.nms_families(H, W, r).items():
        m, pts, conf = sr.nms_fast(heat, sc.THR, d, r)
        np.testing.assert_array_equal(m, sr.nms_brute(heat, sc.THR, d, r), err_msg=name)
        assert len(pts) <= sr.capacity(H, W, d)
        flat = pts[:, 1] * W + pts[:, 0]
        assert (np.diff(flat) > 0).all() and (m[pts[:, 1], pts[:, 0]] == 1).all() and len(pts) == int(m.sum())
        np.testing.assert_array_equal(conf, heat[pts[:, 1], pts[:, 0]])


def test_families_do_what_they_were_built_for():
    H, W = sc.SHAPES[0]
    f0, f4 = sc.nms_families(H, W, 0), sc.nms_families(H, W, 4)
    assert sr.nms_fast(f0["empty"], sc.THR, 4, 0)[0].sum() == 0
    m = sr.nms_fast(f0["at_thresh"], sc.THR, 0, 0)[0]
    assert m[H // 2, W // 2] == 1 and m[H // 2, W // 2 + 1] == 0 and m.sum() == 2
    # the border point outranks its interior neighbour: with d >= 1 both are gone, with d = 0 the neighbour stays
    assert sr.nms_fast(f4["border_outranks"], sc.THR, 1, 4)[0][H // 2, 4] == 0
    assert sr.nms_fast(f4["border_outranks"], sc.THR, 0, 4)[0][H // 2, 4] == 1
    assert np.isnan(f0["nan"]).sum() > 10 and not np.isnan(sr.nms_fast(f0["nan"], sc.THR, 1, 0)[2]).any()
    assert len(np.unique(f0["quantised"])) == 5


@pytest.mark.parametrize("shape", sc.SHAPES)
@pytest.mark.parametrize("d", sc.NMS_DISTS)
def test_a_plateau_reaches_the_capacity_and_nothing_exceeds_it(shape, d):
    H, W = shape
    fam = sc.nms_families(H, W, 0)
    assert len(sr.nms_fast(fam["plateau"], sc.THR, d, 0)[1]) == sr.capacity(H, W, d)
    for name, heat in fam.items():
        assert len(sr.nms_fast(heat, sc.THR, d, 0)[1]) <= sr.capacity(H, W, d), name


def test_flatten_is_softmax_and_pixel_shuffle():
    s = sc.flatten_semi(2, 2, 3)
    t = torch.from_numpy(np.nan_to_num(s, nan=0.0)).double()
    want = torch.nn.functional.pixel_shuffle(torch.softmax(t, 1)[:, :64], 8).numpy()
    np.testing.assert_allclose(sr.flatten(s), want, rtol=1e-13, atol=1e-300)
    np.testing.assert_allclose(sr.flatten_torch(torch.from_numpy(s).double()).numpy(), want, rtol=1e-13, atol=1e-300)
    assert want[-1, 0, -8:, -8:].max() < 1e-15 and abs(want[-1, 0, 0, 7] - 1.0) < 1e-12   # the dustbin cell, the huge logit


@pytest.mark.parametrize("p", [3, 5, 9])
def test_soft_argmax_twins_agree_and_the_flat_patch_has_no_offset(p):
    H, W = sc.SHAPES[1]
    heat = sc.heat_for_patches(2, H, W)
    out = sr.nms_batch(heat, sc.THR, 1, 4)
    pred, patches = sr.soft_argmax(heat, out["pts"], out["count"], p)
    tw = sr.soft_argmax_torch(torch.from_numpy(heat).double(), out["pts"], out["count"], p).numpy()
    np.testing.assert_allclose(tw, pred, rtol=0, atol=1e-12)
    assert np.abs(pred).max() <= p // 2 and np.abs(pred).max() > 0.1
    flat = np.full((1, 1, 16, 24), 0.25, np.float32)
    pts = np.array([[[8, 8]]], np.int32)
    off, _ = sr.soft_argmax(flat, pts, np.array([1]), p)
    # flat: sum x e / (p^2 + 1e-6) - p//2 = -(p//2) 1e-6 / (p^2 + 1e-6)
    np.testing.assert_allclose(off[0, 0], -(p // 2) * 1e-6 / (p * p + 1e-6), rtol=1e-6)


def test_sample_desc_is_grid_sample():
    rng = np.random.default_rng(2)
    B, D, Hc, Wc = 2, 8, 3, 4
    desc = rng.standard_normal((B, D, Hc, Wc)).astype(np.float32)
    pts = rng.integers(0, [8 * Wc, 8 * Hc], (B, 6, 2)).astype(np.int32)
    pred = (rng.random((B, 6, 2)) * 8 - 4).astype(np.float32)
    cnt = np.array([6, 4])
    for align in (True, False):
        ours = sr.sample_desc(desc, pts, pred, cnt, align)
        pos = torch.from_numpy(pts.astype(np.float64) + pred.astype(np.float64))
        grid = torch.stack((pos[..., 0] / (4.0 * Wc) - 1, pos[..., 1] / (4.0 * Hc) - 1), -1)[:, None]
        smp = torch.nn.functional.grid_sample(torch.from_numpy(desc).double(), grid, mode="bilinear", padding_mode="zeros", align_corners=align)
        want = torch.nn.functional.normalize(smp[:, :, 0].transpose(1, 2), dim=2).numpy()
        np.testing.assert_allclose(ours[0], want[0], atol=1e-12)
        np.testing.assert_allclose(ours[1, :4], want[1, :4], atol=1e-12)
        assert (ours[1, 4:] == 0).all()


# ---- the host build of the math header ---------------------------------------------------------------------------------------
def _payload_and_checks():
    """Records for the emulation and, for each, a function that checks its slice of the output."""
    payload, readers = b"", []
    H, W = sc.SHAPES[0]
    for d in sc.NMS_DISTS:
        for r in sc.BORDERS:
            for name, heat in sc.nms_families(H, W, r).items():
                payload += _nms_record(heat, d, r)
                readers.append(("nms", name, heat, d, r))
    H2, W2 = sc.SHAPES[1]
    heat = sc.heat_for_patches(2, H2, W2)
    rng = np.random.default_rng(9)
    for p, d in ((3, 4), (5, 1), (9, 4), (5, 4)):
        out = sr.nms_batch(heat, sc.THR, d, 4)
        for b in range(2):
            n = int(out["count"][b])
            g = rng.standard_normal((n, 2)).astype(np.float32)
            payload += struct.pack("<5i", 2, H2, W2, p, n) + heat[b, 0].astype("<f4").tobytes() + out["pts"][b, :n].astype("<i4").tobytes() + g.tobytes()
            readers.append(("soft", heat[b:b + 1], out["pts"][b:b + 1, :n], n, p, g))
    Hc, Wc, D = 3, 4, 8
    desc = rng.standard_normal((1, D, Hc, Wc)).astype(np.float32)
    desc[0, :, 0, 0] = 0.0
    xy = np.concatenate((rng.random((12, 2)) * [8 * Wc, 8 * Hc], [[4.0, 4.0], [8.0 * Wc - 1, 8.0 * Hc - 1], [-30.0, 5.0], [5.0, 8.0 * Hc + 20], [0.0, 0.0]]))
    for align in (1, 0):
        payload += struct.pack("<6i", 3, Hc, Wc, D, align, len(xy)) + desc.tobytes() + xy.astype("<f8").tobytes()
        readers.append(("desc", desc, xy, align))
    semi = sc.flatten_semi(1, 2, 3)
    gh = rng.standard_normal((1, 1, 16, 24)).astype(np.float32)
    payload += struct.pack("<3i", 4, 2, 3) + semi.tobytes() + gh.tobytes()
    readers.append(("flat", semi, gh))
    return payload, readers


def _soft_grad(heat, pts, n, p, g):
    h = torch.from_numpy(heat).double().requires_grad_(True)
    pred = sr.soft_argmax_torch(h, pts, np.array([n]), p)
    (pred[0] * torch.from_numpy(g).double()).sum().backward()
    return pred.detach().numpy()[0], h.grad.numpy()[0, 0]


def _check_output(buf, readers):
    off, rounds_seen = 0, {}
    for rec in readers:
        if rec[0] == "nms":
            _, name, heat, d, r = rec
            H, W = heat.shape
            rounds, m, pts, conf, off = _read_nms(buf, off, H, W)
            wm, wp, wc = sr.nms_fast(heat, sc.THR, d, r)
            sc.check(m.astype(np.float32), wm, f"emu nms {name} d={d} r={r} map")
            sc.check(pts, wp, f"emu nms {name} d={d} r={r} pts")
            sc.check(conf, wc, f"emu nms {name} d={d} r={r} conf")
            rounds_seen[(name, d)] = rounds
        elif rec[0] == "soft":
            _, heat, pts, n, p, g = rec
            H, W = heat.shape[2:]
            pred = np.frombuffer(buf, "<f4", 2 * n, off).reshape(n, 2)
            off += 8 * n
            gh = np.frombuffer(buf, "<f4", H * W, off).reshape(H, W)
            off += 4 * H * W
            wpred, wg = _soft_grad(heat, pts, n, p, g)
            sc.check(pred, wpred, f"emu soft-argmax p={p}", sr.TOL(wpred))
            sc.check(gh, wg, f"emu soft-argmax adjoint p={p}", sr.TOL(wg))
        elif rec[0] == "desc":
            _, desc, xy, align = rec
            n, D = len(xy), desc.shape[1]
            got = np.frombuffer(buf, "<f4", n * D, off).reshape(n, D)
            off += 4 * n * D
            whole = np.floor(xy)
            want = sr.sample_desc(desc, whole[None].astype(np.int32), (xy - whole)[None], np.array([n]), bool(align))[0]
            sc.check(got, want, f"emu sample_desc align={align}", sr.TOL(want))
            assert (got[-3] == 0).all() and (got[-2] == 0).all()          # pushed outside: zero padding, zero norm
        else:
            _, semi, gh = rec
            heat = np.frombuffer(buf, "<f4", 16 * 24, off).reshape(1, 1, 16, 24)
            off += 4 * 16 * 24
            gs = np.frombuffer(buf, "<f4", 65 * 6, off).reshape(1, 65, 2, 3)
            off += 4 * 65 * 6
            t = torch.from_numpy(semi).double().requires_grad_(True)
            w = sr.flatten_torch(t)
            (w * torch.from_numpy(gh).double()).sum().backward()
            sc.check(heat, w.detach().numpy(), "emu flatten", sr.TOL(w.detach().numpy()))
            sc.check(gs, t.grad.numpy(), "emu flatten adjoint", sr.TOL(t.grad.numpy()))
            assert (gs[np.isnan(semi)] == 0).all()
    assert off == len(buf)
    return rounds_seen


def test_host_build_agrees_with_the_restatement(emu, tmp_path):
    payload, readers = _payload_and_checks()
    rounds = _check_output(run_emu(emu, payload, tmp_path), readers)
    # the fixpoint has no fixed depth: on ramps and plateaus at 16x24 with d = 1 a synchronous schedule needs 38 rounds
    assert max(v for (name, d), v in rounds.items() if d == 1) == 38
    assert rounds[("empty", 4)] == 0 and rounds[("random", 0)] == 1


def test_host_build_is_clean_under_the_sanitizers(emu, tmp_path):
    san = _build("emu_sp_process_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    payload, _ = _payload_and_checks()
    assert run_emu(san, payload, tmp_path, "san") == run_emu(emu, payload, tmp_path, "plain")
