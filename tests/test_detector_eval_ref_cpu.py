"""The detector evaluation without a GPU: the fp64 restatement (tests/detector_eval_ref.py) against the reference's own outputs
(tests/golden/repeatability.npz: compute_repeatability and scikit-learn's average_precision_score), against its 50-digit twin,
and against the host build of csrc/detector_eval_math.h (tests/emu/emu_detector_eval.cpp, a stand-alone program; also built with
-fsanitize=address,undefined and run on its own, never inside Python)."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detector_eval_cases as dc  # noqa: E402
import detector_eval_ref as dr  # noqa: E402

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EMU_DIR = os.path.join(REPO, "tests", "emu")
CSRC = os.path.join(REPO, "pytorch-deepfepe_amd", "csrc")


def _build(name, extra):
    out = os.path.join(EMU_DIR, "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, name)
    srcs = [os.path.join(EMU_DIR, "emu_detector_eval.cpp"), os.path.join(CSRC, "detector_eval_math.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", *extra, f"-I{CSRC}", srcs[0], "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def emu():
    return _build("emu_detector_eval", [])


def run_emu(exe, payload, tmp_path, tag="io"):
    fin, fout = tmp_path / f"{tag}.in", tmp_path / f"{tag}.out"
    fin.write_bytes(payload)
    subprocess.run([exe, str(fin), str(fout)], check=True)
    return fout.read_bytes()


def rec_pair(kp1, kp2, H, height, width, keep_k, thresh):
    C = kp1.shape[1]
    f8 = lambda a: np.ascontiguousarray(a, "<f8").tobytes()  # noqa: E731
    return struct.pack("<8i", 1, len(kp1), len(kp2), C, height, width, keep_k, len(thresh)) + f8(H) + f8(thresh) + f8(kp1) + f8(kp2)


def parse_pair(buf, off, T):
    kept1, kept2, unw = struct.unpack_from("<3i", buf, off)
    off += 12
    g = {"kept1": kept1, "kept2": kept2, "n_unwarped": unw}
    for key, fmt in (("count1", "<i4"), ("count2", "<i4"), ("repeatability", "<f8"), ("loc_err", "<f8")):
        g[key] = np.frombuffer(buf, fmt, T, off).copy()
        off += g[key].nbytes
    return g, off


def rec_ap(lab, sc):
    return struct.pack("<2i", 2, len(lab)) + np.ascontiguousarray(lab, "u1").tobytes() + np.ascontiguousarray(sc, "<f8").tobytes()


def parse_ap(buf, off, m):
    ap, = struct.unpack_from("<d", buf, off)
    P, = struct.unpack_from("<i", buf, off + 8)
    tp = np.frombuffer(buf, "<i4", m, off + 12).copy()
    cnt = np.frombuffer(buf, "<i4", m, off + 12 + 4 * m).copy()
    return {"ap": ap, "n_pos": P, "tp_at": tp, "cnt_at": cnt}, off + 12 + 8 * m


def golden_cases(golden):
    g = golden("repeatability")
    for i in range(int(g["n_cases"][0])):
        h, w, k, th = g[f"c{i}_par"]
        yield i, g[f"c{i}_kp1"], g[f"c{i}_kp2"], g[f"c{i}_H"], int(h), int(w), int(k), float(th), g[f"c{i}_out"]


def test_golden_file_holds_what_the_cases_module_makes(golden):
    """The maker took its inputs from detector_eval_cases.golden_inputs(): the file and the module have not drifted apart."""
    cases = dc.golden_inputs()
    assert int(golden("repeatability")["n_cases"][0]) == len(cases) >= 12
    for (i, kp1, kp2, H, h, w, k, th, _), c in zip(golden_cases(golden), cases):
        assert np.array_equal(kp1, c[0]) and np.array_equal(kp2, c[1]) and np.array_equal(H, c[2]) and (h, w, k, th) == tuple(c[3:]), i
        if kp1.shape[1] == 3:  # distinct probabilities: the reference's unstable argsort has no choice to make
            assert len(np.unique(kp1[:, 2])) == len(kp1) and len(np.unique(kp2[:, 2])) == len(kp2), i


def test_restatement_reproduces_the_reference(golden):
    """compute_repeatability's own outputs: repeatability exactly, the localization error within the restatement's bound (the
    reference inverts H with LAPACK where the restatement takes the adjugate, and sums in numpy's order)."""
    counted = 0
    for i, kp1, kp2, H, h, w, k, th, out in golden_cases(golden):
        r = dr.repeatability_pair(kp1, kp2, H, h, w, k, [th])
        assert r["undecided"] == 0, i
        assert r["repeatability"][0] == out[0], (i, r["repeatability"][0], out[0])
        if r["count1"][0] + r["count2"][0] == 0:
            assert out[0] == 0 and out[1] == -1 and r["loc_err"][0] == -1, i
        else:
            counted += 1
            assert abs(r["loc_err"][0] - out[1]) <= dr.TOL * r["loc_err_bound"][0], (i, r["loc_err"][0], out[1], r["loc_err_bound"][0])
    assert counted >= 6


def test_restatement_reproduces_scikit_learn(golden):
    g = golden("repeatability")
    vecs = dc.golden_ap_inputs()
    assert int(g["n_ap"][0]) == len(vecs)
    for i, (lab, sc) in enumerate(vecs):
        assert np.array_equal(g[f"a{i}_labels"], lab) and np.array_equal(g[f"a{i}_scores"], sc)
        r = dr.average_precision(lab, sc)
        assert abs(r["ap"] - g[f"a{i}_ap"][0]) <= dr.TOL * r["ap_bound"], (i, r["ap"], g[f"a{i}_ap"][0])


def test_average_precision_does_not_depend_on_the_order_of_equal_scores():
    lab, sc = dc.ap_vector(9, 80, "tied")
    a = dr.average_precision(lab, sc)
    perm = np.random.default_rng(0).permutation(80)
    b = dr.average_precision(lab[perm], sc[perm])
    assert abs(a["ap"] - b["ap"]) <= dr.TOL * a["ap_bound"] and a["n_pos"] == b["n_pos"]
    assert np.array_equal(a["tp_at"][perm], b["tp_at"]) and np.array_equal(a["cnt_at"][perm], b["cnt_at"])
    # by hand: scores (1, 1, 0) with labels (1, 0, 1): the tied group gives precision 1/2 at recall 1/2, the whole list 2/3
    r = dr.average_precision([1, 0, 1], [1.0, 1.0, 0.0])
    assert r["tp_at"].tolist() == [1, 1, 2] and r["cnt_at"].tolist() == [2, 2, 3] and abs(r["ap"] - (0.5 * 0.5 + 0.5 * 2 / 3)) < 1e-15


def test_restatement_agrees_with_its_mpmath_twin():
    """The warp (by H and through the adjugate) and every distance of the seeded families at 50 digits: the derived bounds hold."""
    import mpmath as mp

    for name, b in (("projective", 0), ("projective", 2), ("ties", 1), ("lattice", 1)):
        r = dc.ref(name)[b]
        kp1, kp2, H = dc.pair_inputs(dc.jobs()[name], b)
        t1, t2 = dr.mp_warp(H, kp1[:, :2], False), dr.mp_warp(H, kp2[:, :2], True)
        for w, e, t in ((r["w1"], r["e1"], t1), (r["w2"], r["e2"], t2)):
            for i, p in enumerate(t):
                assert p is not None
                assert abs(mp.mpf(float(w[i, 0])) - p[0]) <= e[i, 0] and abs(mp.mpf(float(w[i, 1])) - p[1]) <= e[i, 1], (name, b, i)
        exact2 = [(mp.mpf(float(x)), mp.mpf(float(y))) for x, y in kp2[:, :2]]
        for a, i in enumerate(r["sel1"][:12]):
            for c, j in enumerate(r["sel2"]):
                assert abs(mp.mpf(float(r["D"][a, c])) - dr.mp_dist(t1[i], exact2[j])) <= r["eD"][a, c], (name, b, i, j)


def test_lattice_pairs_do_what_they_were_built_for():
    """Minima of exactly 3 and 5 are counted at thresholds 3 and 5; w - 0.5 is inside the half-open rule and outside the closed one."""
    job = dc.jobs()["lattice"]
    for b, r in enumerate(dc.ref("lattice")):
        assert (r["min1"] == 3.0).any() and (r["min1"] == 5.0).any() and (r["min2"] == 3.0).any() and (r["min2"] == 5.0).any()
        for t, th in enumerate(job["thresh"]):
            assert r["count1"][t] == (r["min1"] <= th).sum() and r["count2"][t] == (r["min2"] <= th).sum()
            if th in (3.0, 5.0):  # a strict comparison would count fewer
                assert r["count1"][t] > (r["min1"] < th).sum() and r["count2"][t] > (r["min2"] < th).sum()
        half = r["w2"][:, 0] == dc.WIDTH - 0.5
        assert half.any() and r["kept2"] > r["n_unwarped"]
        assert not r["eD"][r["D"] == np.rint(r["D"])].any()  # integer distances carry no error


def test_selection_rule_among_equal_probabilities():
    """Stable ascending argsort, then [-k:]: the higher index wins; [-0:] is everything; NaN above +inf; -0 equals +0."""
    assert dr.select_k_best([0.5, 0.5, 0.5, 0.5], 2).tolist() == [2, 3]
    assert sorted(dr.select_k_best([0.5, 0.9, 0.5, 0.1], 2).tolist()) == [1, 2]
    assert len(dr.select_k_best([0.3, 0.2, 0.1], 0)) == 3 and len(dr.select_k_best([0.3, 0.2], 5)) == 2
    assert sorted(dr.select_k_best([np.nan, np.inf, 1.0, np.nan], 3).tolist()) == [0, 1, 3]
    assert sorted(dr.select_k_best([0.0, -0.0, -1.0], 1).tolist()) == [1]


def _all_pairs():
    for name, job in dc.jobs().items():
        for b in range(len(job["H"])):
            yield name, job, b


def test_host_build_agrees_with_the_restatement(emu, tmp_path):
    """Every family, pair by pair, through the same check() as the GPU; then the average precision and the matching score."""
    payload = b""
    for name, job, b in _all_pairs():
        kp1, kp2, H = dc.pair_inputs(job, b)
        payload += rec_pair(kp1, kp2, H, job["height"], job["width"], job["keep_k"], job["thresh"])
    for name, (lab, sc, nv) in dc.ap_jobs().items():
        for b in range(len(lab)):
            n = lab.shape[1] if nv is None else nv[b]
            payload += rec_ap(lab[b, :n], sc[b, :n])
    scores = [(0, 0, 0), (5, 10, 10), (7, 0, 3), (3, 1000, 999), (2 ** 30, 2 ** 30, 2 ** 30)]
    for s in scores:
        payload += struct.pack("<4i", 3, *s)
    buf = run_emu(emu, payload, tmp_path)
    off = 0
    for name, job, b in _all_pairs():
        g, off = parse_pair(buf, off, len(job["thresh"]))
        dc.check(g, name, b, what="host build")
    for name, (lab, sc, nv) in dc.ap_jobs().items():
        for b in range(len(lab)):
            n = lab.shape[1] if nv is None else nv[b]
            g, off = parse_ap(buf, off, n)
            dc.check_ap(g, name, b, what="host build")
    for s in scores:
        got, = struct.unpack_from("<d", buf, off)
        off += 8
        want = dr.matching_score(*s)
        assert got == want or (np.isnan(got) and np.isnan(want)), (s, got, want)
    assert off == len(buf)


def test_host_build_is_clean_under_the_sanitizers(emu, tmp_path):
    """The same program built with -fsanitize=address,undefined, run on its own: same bytes out, nothing reported."""
    san = _build("emu_detector_eval_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    payload = b""
    for name in ("lattice", "projective_k", "ties_signed_zero_nan_inf", "two_columns", "empty_both", "empty_1", "outside", "ragged", "edge_257"):
        job = dc.jobs()[name]
        for b in range(len(job["H"])):
            kp1, kp2, H = dc.pair_inputs(job, b)
            payload += rec_pair(kp1, kp2, H, job["height"], job["width"], job["keep_k"], job["thresh"])
    for name in ("kinds", "no_pos_all_pos", "one_entry", "no_entry", "edge_65"):
        lab, sc, nv = dc.ap_jobs()[name]
        for b in range(len(lab)):
            payload += rec_ap(lab[b], sc[b])
    payload += struct.pack("<4i", 3, 5, 10, 10) + struct.pack("<4i", 3, 0, 0, 0)
    assert run_emu(san, payload, tmp_path, "san") == run_emu(emu, payload, tmp_path, "plain")
