"""The correspondence evaluation without a GPU: the fp64 restatement (tests/corr_eval_ref.py) against the reference's own outputs
(tests/golden/corr_eval.npz: epi_distance_np and Result_processor), against its 50-digit twin, and the host build of
csrc/corr_eval_math.h (tests/emu/emu_corr_eval.cpp, compiled with g++) through the same check() as the GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import corr_eval_cases as cc  # noqa: E402
import corr_eval_ref as cr  # noqa: E402

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EMU_DIR = os.path.join(REPO, "tests", "emu")
CSRC = os.path.join(REPO, "pytorch-deepfepe_amd", "csrc")
ALL_CASES = [s[0] for s in cc.SHAPES] + ["nomask", "edge", "dist", "golden"]


def case_of(name):
    special = {"nomask": cc.no_mask_case, "edge": cc.edge_case, "dist": cc.dist_case, "golden": cc.golden_padded}
    return special[name]() if name in special else cc.shape_case(name)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(REPO, "tests", "golden", "corr_eval.npz"))


@pytest.fixture(scope="module")
def emu():
    out = os.path.join(EMU_DIR, "_build")
    os.makedirs(out, exist_ok=True)
    lib = os.path.join(out, "libemu_corr_eval.so")
    srcs = [os.path.join(EMU_DIR, "emu_corr_eval.cpp"), os.path.join(CSRC, "corr_eval_math.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", f"-I{CSRC}", srcs[0], "-o", lib], check=True)
    return ctypes.CDLL(lib)


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def run_emu(L, case):
    m, d = case.get("matches"), case.get("dist")
    B, N = (m.shape[:2] if m is not None else d.shape)
    F = None if m is None else np.ascontiguousarray(case["F"], np.float64).reshape(B, 9)
    sc = case["scores"]
    it = np.asarray(case["ithds"], np.float64)
    mt = None if sc is None else np.asarray(case["mthds"], np.float64)
    Ti, Tm = len(it), (1 if mt is None else len(mt))
    got = {"cnt": np.full((B, Tm, Ti), -7, np.int32), "num": np.full((B, Tm), -7, np.int32), "ratio": np.full((B, Tm, Ti), -7.0),
           "dist_out": np.full((B, N), -7.0, np.float32)}
    keep = [np.ascontiguousarray(a) if a is not None else None for a in (m, d, sc, case["n_valid"])]
    rc = L.emu_inlier_table(_p(keep[0]), _p(F), _p(keep[1]), _p(keep[2]), _p(keep[3]), B, N, _p(it), Ti, _p(mt), Tm, _p(got["cnt"]),
                            _p(got["num"]), _p(got["ratio"]), _p(got["dist_out"]))
    assert rc == 0
    got["mean"], got["num_T"] = np.full((Tm, Ti), -7.0), np.full((Tm, B), -7, np.int32)
    assert L.emu_inlier_table_mean(_p(got["ratio"]), _p(got["num"]), B, Tm, Ti, _p(got["mean"]), _p(got["num_T"])) == 0
    return got


def test_fixture_holds_the_golden_inputs(golden):
    pairs = cc.golden_inputs()
    assert len(pairs) == 12 and sorted(len(p[0]) for p in pairs) == sorted(cc.GOLDEN_SIZES)
    for k, (m, F, sc) in enumerate(pairs):
        assert np.array_equal(golden[f"matches_{k}"], m) and golden[f"matches_{k}"].dtype == np.float32
        assert np.array_equal(golden[f"F_{k}"], F) and np.array_equal(golden[f"scores_{k}"], sc)
    assert list(golden["ithds"]) == cc.GOLDEN_ITHDS and list(golden["mthds"]) == cc.GOLDEN_MTHDS
    assert np.isnan(golden["mask_mean"]).all() and (golden["mask_num"][:, list(cc.GOLDEN_NONE_KEPT)] == 0).all()


def test_restatement_reproduces_the_reference(golden):
    case = cc.golden_padded()
    ref, und, triples = cc.expected(case)
    assert not triples  # every decision of the fixture is outside the bound, so numpy's BLAS order cannot move a count
    B = len(cc.GOLDEN_SIZES)
    for k in range(B):
        n = cc.GOLDEN_SIZES[k]
        d, e = ref["dist64"][k, :n], golden[f"dist3_{k}"]
        assert (np.abs(d - e) <= cr.TOL * cr.dist3_bound(case["F"][k], case["matches"][k, :n])).all()
    # counts and num_corrs exactly; ratios bit for bit (equal integers divided in fp64 give the same quotient)
    assert np.array_equal(ref["num"].T, golden["mask_num"])
    assert cc._same(ref["ratio"].transpose(1, 0, 2), golden["from_est_mask"])
    with np.errstate(all="ignore"):
        counts = np.rint(golden["from_est_mask"] * golden["mask_num"][:, :, None])
    kept = golden["mask_num"] > 0
    assert np.array_equal(ref["cnt"].transpose(1, 0, 2)[kept], counts[kept].astype(np.int64))
    assert (ref["cnt"].transpose(1, 0, 2)[~kept] == 0).all()
    assert np.isnan(ref["mean"]).all() and np.isnan(golden["mask_mean"]).all()  # a pair with nothing kept is in the mean
    # without the mask, and the mean table within (B - 1) 2^-53 sum|x| of the reference's stored value
    nm = cr.inlier_table(matches=case["matches"], F=case["F"], n_valid=case["n_valid"], inlier_thds=case["ithds"])
    assert np.array_equal(nm["num"][:, 0], golden["nomask_num"]) and np.array_equal(nm["num"][:, 0], np.asarray(cc.GOLDEN_SIZES))
    assert cc._same(nm["ratio"][:, 0], golden["from_est"])
    tol = (B - 1) * 2.0 ** -53 * np.abs(nm["ratio"][:, 0]).sum(0)
    assert (np.abs(nm["mean"][0] - golden["nomask_mean"]) <= tol).all()
    assert (np.abs(nm["mean"][0] - golden["nested"]) <= tol).all()
    # the masked mean over the pairs that keep something
    kp = golden["kept_pairs"]
    sub = cr.inlier_table(matches=case["matches"][kp], F=case["F"][kp], scores=case["scores"][kp], n_valid=case["n_valid"][kp],
                          inlier_thds=case["ithds"], mask_thds=case["mthds"])
    assert np.array_equal(sub["num_T"], golden["kept_num"])
    tol = (len(kp) - 1) * 2.0 ** -53 * np.abs(sub["ratio"]).sum(0)
    assert np.isfinite(golden["kept_mean"]).all() and (np.abs(sub["mean"] - golden["kept_mean"]) <= tol).all()


@pytest.mark.parametrize("name", ["n63", "n257", "edge"])
def test_distance_within_its_bound_of_the_50_digit_twin(name):
    import mpmath as mp

    case = case_of(name)
    worst = 0.0
    for b in range(case["matches"].shape[0]):
        d, bound = cr.dist3(case["F"][b], case["matches"][b]), cr.dist3_bound(case["F"][b], case["matches"][b])
        exact = cr.dist3_mp(case["F"][b], case["matches"][b])
        with mp.workdps(50):
            for i, e in enumerate(exact):
                if mp.isnan(e) or mp.isinf(e):
                    assert (np.isnan(d[i]) if mp.isnan(e) else d[i] == np.inf) and bound[i] == 0.0
                    continue
                err = abs(mp.mpf(float(d[i])) - e)
                assert err <= mp.mpf(float(bound[i])), (name, b, i)
                worst = max(worst, float(err) / float(bound[i]))
    print(f"{name}: largest |fp64 - exact| / bound = {worst:.3f}")


@pytest.mark.parametrize("name", ALL_CASES)
def test_undecided_set_is_the_listed_one(name):
    case = case_of(name)
    _, und, triples = cc.expected(case)
    assert triples == case["listed"]
    if name != "edge":
        assert not triples and not und.any()  # the random cases are decided everywhere


def test_edge_case_is_what_it_says():
    case = cc.edge_case()
    ref, _, _ = cc.expected(case)
    assert np.isnan(ref["dist64"][1, :2]).all() and np.isfinite(ref["dist64"][1, 2:]).all()
    assert np.isinf(ref["dist64"][2]).all()
    assert ref["num"].tolist()[1:] == [[70, 70], [70, 70], [0, 0]]
    assert ref["cnt"][1, 0, 2] == 68 and (ref["cnt"][2] == 0).all()  # the NaN distances stay in the denominator: 68 / 70
    assert ref["ratio"][1, 0, 2] == 68 / 70 and np.isnan(ref["ratio"][3]).all() and np.isnan(ref["mean"]).all()
    sc = case["scores"][0]
    kept05 = int((sc[5:].astype(np.float64) < 0.5).sum()) + 1  # of the planted five only the one a step below 0.5 is kept
    assert ref["num"][0, 0] == kept05 and ref["num"][0, 1] == int((sc[5:].astype(np.float64) < 1.0).sum()) + 2
    assert ref["cnt"][0, 1, 1] == int((ref["dist64"][0][sc < 1.0] < case["ithds"][1]).sum())  # match 5 itself is no inlier of its own distance


def test_dist_input_agrees_with_matches_input():
    """The fp32-rounded distance decides as the fp64 one wherever no threshold lies between the two."""
    case = cc.shape_case("n65")
    ref, _, _ = cc.expected(case)
    d32 = ref["dist_out"]
    for th in case["ithds"]:
        lo, hi = np.minimum(d32.astype(np.float64), ref["dist64"]), np.maximum(d32.astype(np.float64), ref["dist64"])
        assert not ((lo < th) & (th <= hi)).any()
    again = cr.inlier_table(dist=d32, scores=case["scores"], n_valid=case["n_valid"], inlier_thds=case["ithds"], mask_thds=case["mthds"])
    assert np.array_equal(again["cnt"], ref["cnt"]) and np.array_equal(again["num"], ref["num"])


@pytest.mark.parametrize("name", ALL_CASES)
def test_host_build_passes_the_check(emu, name):
    case = case_of(name)
    cc.check(case, run_emu(emu, case))


def test_host_build_refusals(emu):
    a = np.zeros(64, np.float64)
    f = lambda **k: emu.emu_inlier_table(*[k.get(n, _p(a)) if n not in ("B", "N", "Ti", "Tm") else k.get(n, 2) for n in  # noqa: E731
                                           ("m", "F", "d", "sc", "nv", "B", "N", "it", "Ti", "mt", "Tm", "cnt", "num", "ratio", "do")])
    assert f(d=None) == 0 and f(m=None, F=None) == 0
    assert f() == -1 and f(d=None, Ti=0) == -1 and f(d=None, Tm=17) == -1 and f(d=None, B=-1) == -1
    assert f(d=None, sc=None, Tm=2) == -1 and f(d=None, sc=None, mt=None, Tm=1) == 0
    assert f(m=None, d=None) == -1 and f(m=None, d=None, N=0) == 0 and f(d=None, F=None) == -1
    assert f(d=None, cnt=None, num=None, ratio=None, do=None) == -1 and f(d=None, B=0, it=None) == 0
