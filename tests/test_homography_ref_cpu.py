"""The homography estimator without a GPU: the fp64 restatement (tests/homography_ref.py) against a known H, against its 50-digit
twin and against the host build of csrc/homography_math.h (tests/emu/emu_homography.cpp, a stand-alone program; also built with
-fsanitize=address,undefined and run on its own, never inside Python)."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import homography_cases as hc  # noqa: E402
import homography_ref as hr  # noqa: E402
import rule_tables  # noqa: E402

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EMU_DIR = os.path.join(REPO, "tests", "emu")
CSRC = os.path.join(REPO, "pytorch-deepfepe_amd", "csrc")


def _build(name, extra):
    out = os.path.join(EMU_DIR, "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, name)
    srcs = [os.path.join(EMU_DIR, "emu_homography.cpp"), os.path.join(CSRC, "homography_math.h"), os.path.join(CSRC, "ransac_math.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", *extra, f"-I{CSRC}", srcs[0], "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def emu():
    return _build("emu_homography", [])


def rec_pair(m, n, threshold, confidence, max_iters, seed, flags):
    m = np.ascontiguousarray(m[:n], np.float32)
    return struct.pack("<iiddiQI", 5, n, threshold, confidence, max_iters, seed, flags) + m.tobytes()


def parse_pair(buf, off, n, max_iters):
    def take(fmt, count=1):
        nonlocal off
        a = np.frombuffer(buf, fmt, count, off)
        off += a.nbytes
        return a

    g = {"table": take("<i4", max_iters).astype(np.int64)}
    g["best"], g["best_k"], g["iters"] = (int(v) for v in take("<i4", 3))
    g["H_model"] = take("<f8", 9).copy()
    g["mask"] = take("u1", n).copy()
    g["refit_ok"] = int(take("<i4")[0])
    g["H_refit"] = take("<f8", 9).copy()
    g["H_out"] = take("<f8", 9).copy()
    g["lm_iters"] = int(take("<i4")[0])
    g["R"] = take("<f8", 10).copy()
    g["S0"], g["S1"] = (float(v) for v in take("<f8", 2))
    if g["lm_iters"] == 0:
        g["S0"] = g["S1"] = None
    return g, off


def run_emu(exe, payload, tmp_path, tag="io"):
    fin, fout = tmp_path / f"{tag}.in", tmp_path / f"{tag}.out"
    fin.write_bytes(payload)
    subprocess.run([exe, str(fin), str(fout)], check=True)
    return fout.read_bytes()


def test_restatement_recovers_a_noise_free_homography():
    m, H = hc.synth(5, 60, 0.0, 0.0)
    r = hr.estimate(m, None, 3.0, 0.995, 32, 0)
    assert r["best"] == 60 and r["mask"].all()
    # float32 rounding of the coordinates is the only noise: ~320 * 2^-24 = 2e-5 px, which a four-point fit magnifies at the far
    # corners and the fit over all 60 averages down
    for key, tol in (("H_model", 5e-3), ("H_refit", 1e-4), ("H_out", 1e-4)):
        assert hr.max_transfer_diff(r[key], H / H[2, 2], m) < tol, key
    assert r["lm"]["S1"] <= r["lm"]["S0"]


def test_restatement_agrees_with_its_mpmath_twin():
    """The yardsticks of tests/homography_cases.py are not exceeded on a sample of what they were measured on."""
    for name in ("synth_30_5_4", "projective", "noise"):
        m = hc.pair(name)
        for idx, H, kap in hc.hyps(name, hc.N_DEFAULT, None, 0, 24)[:6]:
            if H is None:
                continue
            sure, _, _ = hr.classify(H, m, 3.0, kap)
            sure[idx] = True
            d = hr.max_transfer_diff(H, hr.mp_solve4(m[idx]), m[sure], corners=False)
            assert d <= hc.Y_SOLVE_PER_KAPPA_EPS * kap * hc.EPS, (name, idx, d)
        r = hc.ref(name, max_iters=24)
        pin = m[r["mask"] > 0]
        assert hr.max_transfer_diff(r["H_refit"], hr.mp_refit(pin), pin) <= hc.Y_REFIT_PER_KAPPA_EPS * r["kappa_refit"] * hc.EPS
        h = r["H_refit"].reshape(-1)[:8]
        rr_, J = hr.lm_eval(h, pin)
        A, v, S = hr.mp_lm_eval(h, pin)
        Jf = J.reshape(-1, 8)
        np.testing.assert_allclose(Jf.T @ Jf, A, rtol=1e-12, atol=1e-12 * np.abs(A).max())
        np.testing.assert_allclose((rr_ * rr_).sum(), S, rtol=1e-10, atol=len(pin) * (4 * hc.EPS * hc.WIDTH) ** 2)
        # every residual carries a rounding error of about 4 eps * 320 px, which J^T multiplies
        assert (np.abs(Jf.T @ rr_.reshape(-1) - v) <= 4 * hc.EPS * hc.WIDTH * np.abs(Jf).sum(0) + 1e-300).all()


def test_lm_never_increases_the_cost():
    for name in hc.FAMILIES:
        r = hc.ref(name)
        if r["lm"] is not None:
            S = r["lm"]["S"] + [r["lm"]["S1"]]
            assert all(b <= a for a, b in zip(S, S[1:])), name
            assert r["lm"]["S1"] <= r["lm"]["S0"]


def test_select_rule_on_a_hand_made_table():
    n = 100
    # 3 is not a model (count must exceed 3); 10 at k=1 wins; 10 again does not replace it; 50 at k=4 does and leaves niters at
    # 7 (84 wanted); 99 at k=5 wants two iterations, so the loop stops at k = 6 and the second 99 is never read
    tab = [3, 10, 10, hr.NO_MODEL, 50, 99, 99]
    assert hr.update_num_iters4(0.995, 0.5, 7) == 7 and hr.update_num_iters4(0.995, 0.01, 7) == 2
    assert hr.select(tab, n, 0.995, len(tab)) == (99, 5, 6)
    assert hr.select([3, 10, hr.NO_SAMPLE, 99], n, 0.995, 4) == (10, 1, 2)          # the loop ends at the first missing sample
    assert hr.select([hr.NO_SAMPLE, 99], n, 0.995, 2) == (0, -1, 0)                 # ... and there is no model when that is k = 0
    assert hr.select([100, 4, 4], n, 0.995, 3) == (100, 0, 1)                       # all inliers: niters = 0, the loop stops
    assert hr.select([hr.NO_MODEL] * 5, n, 0.995, 5) == (0, -1, 5)
    assert hr.select([60, 70], n, 0.0, 2) == (60, 0, 1)                              # confidence 0: one model is enough
    assert hr.update_num_iters4(1.0, 0.5, 2000) == 2000 and hr.update_num_iters4(0.995, 0.7, 2000) == 651  # log(0.005) / log(1 - 0.3^4) = 651.5 - 0.03


def test_qr_and_svd_routes_stay_inside_the_ambiguity_cap():
    """The cap of the comparison: at most 10 % of the compared pairs may be ambiguous, decided by the restatement alone -- its
    two null-space routes must agree on every pair it calls unambiguous, and it may call at most 10 % ambiguous."""
    total, amb = 0, []
    for name in hc.FAMILIES:
        for (t, p, it, seed, flags) in hc.SETTINGS:
            a = hc.ref(name, threshold=t, confidence=p, max_iters=it, seed=seed, flags=flags)
            b = hc.ref(name, threshold=t, confidence=p, max_iters=it, seed=seed, flags=flags, route="svd")
            total += 1
            if a["ambiguous"] is not None or b["ambiguous"] is not None:
                amb.append((name, t, flags, a["ambiguous"] or b["ambiguous"]))
                continue
            g = {k: a[k] for k in ("table", "best", "best_k", "iters", "H_model", "mask", "H_refit", "H_out")}
            assert hc.check(g, b, hc.pair(name), t, p, what=f"{name} t={t} qr against svd") == "exact"
    print(f"{len(amb)} of {total} pairs ambiguous:", *amb, sep="\n  ")
    assert len(amb) <= 0.10 * total


def test_special_pairs_do_what_they_were_built_for():
    r = hr.estimate(hc.pair("collinear", 50), None, 3.0, 0.995, 3, 0)
    assert r["best"] == 0 and (r["table"] == hr.NO_SAMPLE).all() and r["iters"] == 0 and not r["H_out"].any()
    r = hr.estimate(hc.pair("sampler_stop", 200), None, 3.0, 0.995, 3, 0)
    assert r["table"][0] == 4 and r["table"][1] == hr.NO_SAMPLE and (r["best"], r["best_k"], r["iters"]) == (4, 0, 1)
    m = hc.pair("w_zero")
    H = np.array([[1.0, 0.02, 3.0], [-0.01, 1.0, -2.0], [-1.0 / 128.0, 0.0, 1.0]])
    assert hr.transfer(H, m[:1])[2][0] == 0.0 and not np.isfinite(hr.errors(H, m[:1])[0])
    r = hc.ref("w_zero")
    assert r["mask"][0] == 0 and r["best"] >= 90


@pytest.mark.parametrize("n", hc.N_VALID)
def test_pair_sizes_in_the_restatement(n):
    r = hc.ref("synth_30_5_4", n=n, max_iters=16)
    if n is not None and n < 4:
        assert r["best"] == 0 and not r["mask"].any() and not r["H_out"].any()
    elif n == 4:
        assert r["best"] == 4 and r["mask"][:4].all() and not r["mask"][4:].any() and r["lm"] is None and (r["H_out"] == r["H_model"]).all()


def test_host_build_agrees_with_the_restatement(emu, tmp_path):
    """Every family at every setting, every pair size, the slow-sampler pairs: the host build of homography_math.h, launch by
    launch as csrc/homography.hip runs it, through the same check() as the GPU."""
    jobs = hc.jobs()
    payload = b""
    for (name, N, n, t, p, it, seed, flags) in jobs:
        payload += rec_pair(hc.pair(name, N), N if n is None else n, t, p, it, seed, flags)
    buf = run_emu(emu, payload, tmp_path)
    off, kinds = 0, []
    for (name, N, n, t, p, it, seed, flags) in jobs:
        nn = N if n is None else n
        g, off = parse_pair(buf, off, nn, it)
        g["mask"] = np.r_[g["mask"], np.zeros(N - nn, np.uint8)]
        r = hc.ref(name, N, n, t, p, it, seed, flags)
        if flags & hr.NO_REFINE:
            g["H_out"] = g["H_refit"]
        kinds.append(hc.check(g, r, hc.pair(name, N), t, p, what=f"{name} n={n} t={t} p={p} flags={flags}"))
    assert off == len(buf)
    assert kinds.count("ambiguous") <= 0.10 * len(kinds)


def test_host_build_small_records(emu, tmp_path):
    m = hc.pair("synth_30_5_4")
    payload = b""
    for k in range(8):
        payload += struct.pack("<iQii", 1, 3, k, len(m)) + m.tobytes()
    payload += struct.pack("<iQii", 1, (1 << 64) - 1, 0, 50) + hc.pair("collinear", 50).tobytes()
    quad = m[hr.draw_sample(0, 0, m)]
    payload += struct.pack("<i", 2) + quad.tobytes()
    payload += struct.pack("<i", 2) + np.tile(quad[:1], (4, 1)).tobytes()  # four equal points: sums below FLT_EPSILON, no model
    tab = [3, 10, 10, hr.NO_MODEL, 50, 99, 99]
    payload += struct.pack("<iidi", 3, 100, 0.995, len(tab)) + np.array(tab, "<i4").tobytes()
    grid = [(p, ep, ni) for p in (0.0, 0.5, 0.995, 1.0) for ep in (0.0, 0.1, 0.5, 0.96, 1.0) for ni in (1, 64, 2000)]
    for (p, ep, ni) in grid:
        payload += struct.pack("<iddi", 4, p, ep, ni)
    buf = run_emu(emu, payload, tmp_path, "small")
    off = 0
    for k in range(8):
        ok, *idx = struct.unpack_from("<5i", buf, off)
        off += 20
        assert ok == 1 and idx == hr.draw_sample(3, k, m)
    ok, *idx = struct.unpack_from("<5i", buf, off)
    off += 20
    assert ok == 0
    ok, = struct.unpack_from("<i", buf, off)
    H = np.frombuffer(buf, "<f8", 9, off + 4).reshape(3, 3)
    off += 76
    Hr, kap = hr.solve4(quad)
    assert ok == 1 and hr.max_transfer_diff(H, Hr, quad, corners=False) <= hc.tol_solve(kap)
    ok, = struct.unpack_from("<i", buf, off)
    off += 76
    assert ok == 0
    assert struct.unpack_from("<3i", buf, off) == hr.select(tab, 100, 0.995, len(tab))
    off += 12
    for (p, ep, ni) in grid:
        assert struct.unpack_from("<i", buf, off)[0] == hr.update_num_iters4(p, ep, ni), (p, ep, ni)
        off += 4
    assert off == len(buf)


def test_shared_rule_as_1_slot_of_4_points_on_the_edge_tables(emu, tmp_path):
    """rs::select_best<1, 4> on tests/rule_tables.py: no sample at k = 0 and past the first model, ties, confidence 0 and 1 --
    the three outputs it has with one slot against this estimator's own restatement."""
    cases = [(tab[:, 0].copy(), N, conf) for tab, N, conf in rule_tables.tables(1, hr.NO_SAMPLE)]
    payload = b"".join(struct.pack("<iidi", 3, N, conf, len(tab)) + tab.astype("<i4").tobytes() for tab, N, conf in cases)
    buf = run_emu(emu, payload, tmp_path, "rule")
    assert len(buf) == 12 * len(cases)
    for i, (tab, N, conf) in enumerate(cases):
        assert struct.unpack_from("<3i", buf, 12 * i) == hr.select(tab, N, conf, len(tab)), (tab.tolist(), N, conf)


def test_host_build_is_clean_under_the_sanitizers(emu, tmp_path):
    """The same program built with -fsanitize=address,undefined, run on its own: same bytes out, nothing reported."""
    san = _build("emu_homography_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    payload = b""
    for name, N, n, flags in (("synth_30_5_4", 100, None, 0), ("noise", 100, None, 0), ("synth_30_5_4", 100, 4, 0), ("synth_30_5_4", 100, 0, 0),
                              ("w_zero", 100, None, hr.ALL_POINTS), ("collinear", 50, None, 0), ("sampler_stop", 200, None, 0)):
        payload += rec_pair(hc.pair(name, N), N if n is None else n, 3.0, 0.995, 3 if N != 100 else 16, 0, flags)
    assert run_emu(san, payload, tmp_path, "san") == run_emu(emu, payload, tmp_path, "plain")
