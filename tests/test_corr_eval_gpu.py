"""The correspondence evaluation on the GPU: every case of tests/corr_eval_cases.py through ops.inlier_table / ops.inlier_table_mean
and the same check() as the host build -- outside the listed undecided set every count exact, the ratios bit-exact, dist_out the
fp32 rounding of the fp64 distance, bit-identical on a second call -- then the compat surface: Result_processor against the
reference's own outputs (tests/golden/corr_eval.npz), and correspondence_eval_batch against the same pairs pushed one at a time
through PointTracker -> epi_dist_from_matches -> Result_processor, eagerly and from a captured graph."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import corr_eval_cases as cc  # noqa: E402
import corr_eval_ref as cr  # noqa: E402
import match_ref as mr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ALL_CASES = [s[0] for s in cc.SHAPES] + ["nomask", "edge", "dist", "golden"]


def case_of(name):
    special = {"nomask": cc.no_mask_case, "edge": cc.edge_case, "dist": cc.dist_case, "golden": cc.golden_padded}
    return special[name]() if name in special else cc.shape_case(name)


def _dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=DEV, dtype=dtype)


def _run(dfepe, case):
    it = _dev(np.asarray(case["ithds"], np.float64))
    mt = None if case["scores"] is None else _dev(np.asarray(case["mthds"], np.float64))
    out = dfepe.ops.inlier_table(matches=_dev(case.get("matches")), F=_dev(case.get("F")), dist=_dev(case.get("dist")),
                                 scores=_dev(case["scores"]), n_valid=_dev(case["n_valid"]), inlier_thds=it, mask_thds=mt,
                                 want=("cnt", "num", "ratio", "dist_out"))
    out["mean"], out["num_T"] = dfepe.ops.inlier_table_mean(out["ratio"], out["num"])
    return out


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else (t.view(torch.int32) if t.dtype == torch.float32 else t)


@pytest.mark.parametrize("name", ALL_CASES)
def test_cases_pass_the_check_and_repeat_bit_for_bit(dfepe, name):
    case = case_of(name)
    out, again = _run(dfepe, case), _run(dfepe, case)
    for key, v in out.items():
        assert torch.equal(_bits(v), _bits(again[key])), key
    cc.check(case, {k: v.cpu().numpy() for k, v in out.items()})


def test_dist_input_gives_the_counts_of_the_matches_input(dfepe):
    case = cc.shape_case("n65")  # held on the CPU: no threshold lies between a distance and its fp32 rounding
    a = _run(dfepe, case)
    b = dfepe.ops.inlier_table(dist=a["dist_out"], scores=_dev(case["scores"]), n_valid=_dev(case["n_valid"]), inlier_thds=case["ithds"],
                               mask_thds=case["mthds"], want=("cnt", "num", "ratio", "dist_out"))
    for key in ("cnt", "num", "ratio", "dist_out"):
        assert torch.equal(_bits(a[key]), _bits(b[key])), key


def test_outputs_are_optional_and_inputs_untouched(dfepe):
    case = cc.shape_case("n257")
    m, sc = _dev(case["matches"]), _dev(case["scores"])
    m0, sc0 = m.clone(), sc.clone()
    full = _run(dfepe, case)
    for want in (("cnt",), ("num",), ("ratio",), ("dist_out",)):
        r = dfepe.ops.inlier_table(matches=m, F=_dev(case["F"]), scores=sc, n_valid=_dev(case["n_valid"]), inlier_thds=case["ithds"],
                                   mask_thds=case["mthds"], want=want)
        assert tuple(r) == want and torch.equal(_bits(r[want[0]]), _bits(full[want[0]]))
    assert torch.equal(m, m0) and torch.equal(sc, sc0)


def test_empty_batch(dfepe):
    r = dfepe.ops.inlier_table(dist=torch.zeros(0, 5, device=DEV), inlier_thds=[1.0, 2.0])
    assert r["cnt"].shape == (0, 1, 2) and r["ratio"].shape == (0, 1, 2)
    mean, num_T = dfepe.ops.inlier_table_mean(r["ratio"], r["num"])
    assert mean.shape == (1, 2) and bool(torch.isnan(mean).all()) and num_T.shape == (1, 0)


def test_result_processor_reproduces_the_reference(dfepe):
    g = np.load(os.path.join(REPO, "tests", "golden", "corr_eval.npz"))
    B = len(cc.GOLDEN_SIZES)
    # the fixture's own float64 distances, rounded to float32 on the way in: decided for these thresholds (no threshold between a
    # distance and its rounding), so the counts are the reference's
    dists, scores = [g[f"dist3_{k}"] for k in range(B)], [g[f"scores_{k}"] for k in range(B)]
    ithds, mthds = list(g["ithds"]), list(g["mthds"])
    for d in dists:
        lo, hi = np.minimum(d, d.astype(np.float32)), np.maximum(d, d.astype(np.float32))
        assert not any(((lo < t) & (t <= hi)).any() for t in ithds)
    rp = dfepe.compat.eval_tools.Result_processor(["epi_dist_mean_gt", "mscores"])
    for d, s in zip(dists, scores):
        rp.load_result({"epi_dist_mean_gt": d, "mscores": s})
    r = rp.inlier_ratio(dists, ithds)
    tol = (B - 1) * 2.0 ** -53 * np.abs(g["from_est"]).sum(0)
    assert np.array_equal(r["num_corrs"], g["nomask_num"]) and (np.abs(r["inlier_ratio"] - g["nomask_mean"]) <= tol).all()
    assert (np.abs(rp.inlier_ratio_nested(dists, ithds) - g["nested"]) <= tol).all()
    assert (np.abs(rp.inlier_ratio("epi_dist_mean_gt", ithds)["inlier_ratio"] - g["nomask_mean"]) <= tol).all()
    for k in (0, 4, 10):
        got = rp.inlier_ratio_from_est(dists[k], ithds)
        assert isinstance(got, list) and np.array_equal(np.asarray(got), g["from_est"][k])
    for j, mt in enumerate(mthds):
        r = rp.inlier_ratio(dists, ithds, mask_list=scores, mask_thd=mt)
        assert np.array_equal(r["num_corrs"], g["mask_num"][j]) and np.isnan(r["inlier_ratio"]).all()
    kp = list(g["kept_pairs"])
    sub = dfepe.compat.eval_tools.Result_processor(["epi_dist_mean_gt", "mscores"])
    for k in kp:
        sub.load_result({"epi_dist_mean_gt": dists[k], "mscores": scores[k]})
    ap = sub.ap_inlier_thd("epi_dist_mean_gt", ithds, mthds)
    tol = (len(kp) - 1) * 2.0 ** -53 * np.abs(g["from_est_mask"][:, kp]).sum(1)
    assert ap["inlier_thd"].shape == (2, 5) and (np.abs(ap["inlier_thd"] - g["kept_mean"]) <= tol).all()
    assert np.array_equal(ap["num_corrs"], g["kept_num"])
    for j, mt in enumerate(mthds):
        r = sub.inlier_ratio([dists[k] for k in kp], ithds, mask_list=[scores[k] for k in kp], mask_thd=mt)
        assert np.array_equal(r["inlier_ratio"], ap["inlier_thd"][j]) and np.array_equal(r["num_corrs"], ap["num_corrs"][j])


def test_epi_dist_from_matches(dfepe):
    case = cc.shape_case("n257")
    ref, _, _ = cc.expected(case)
    sample = {"F": torch.as_tensor(case["F"][1:])}
    r = dfepe.compat.evaluation_epiDist.epi_dist_from_matches(case["matches"][1:2], sample, DEV)
    d = r["epi_dist_mean_gt"]
    assert isinstance(d, np.ndarray) and d.dtype == np.float32 and np.array_equal(d, cr.dist3(case["F"][1], case["matches"][1]).astype(np.float32))
    assert np.array_equal(d[:1], ref["dist_out"][1, :1])


# ---- the pipeline: descriptors -> matches -> distances -> table ---------------------------------------------------------------------
B_PIPE, N_PIPE, D_PIPE = 3, 150, 64


def _pipeline_inputs():
    """Seeded pairs: image 2 holds a permuted, perturbed copy of most of image 1's descriptors (distances 0.05 .. 0.9, on both sides
    of the threshold) and some of its own; the keypoints come from a corr_eval_cases scene through the same permutation, so the
    matches have distances on both sides of the inlier thresholds."""
    g = np.random.RandomState(77)
    m, F, _ = cc.scene(78, B_PIPE, N_PIPE)
    d1 = g.randn(B_PIPE, N_PIPE, D_PIPE)
    d1 /= np.linalg.norm(d1, axis=2, keepdims=True)
    d2, p2 = np.zeros_like(d1), np.zeros((B_PIPE, N_PIPE, 2), np.float32)
    for b in range(B_PIPE):
        perm = g.permutation(N_PIPE)
        noise = g.randn(N_PIPE, D_PIPE)
        noise /= np.linalg.norm(noise, axis=1, keepdims=True)
        moved = d1[b] + noise * g.uniform(0.05, 0.9, (N_PIPE, 1))
        fresh = g.rand(N_PIPE) < 0.2
        moved[fresh] = g.randn(int(fresh.sum()), D_PIPE)
        d2[b, perm] = moved / np.linalg.norm(moved, axis=1, keepdims=True)
        p2[b, perm] = m[b, :, 2:]
    return m[:, :, :2].copy(), p2, d1.astype(np.float32), d2.astype(np.float32), F


@pytest.fixture(scope="module")
def pipe():
    p1, p2, d1, d2, F = _pipeline_inputs()
    refs = [mr.PairRef(d1[b], d2[b]) for b in range(B_PIPE)]
    thr = mr.pick_threshold(refs, 0.7)
    for r in refs:  # the match sets are decided by match_ref's rule: every row, every column it names, and the threshold
        assert (r.status(thr) != 0).all()
    return {"p1": p1, "p2": p2, "d1": d1, "d2": d2, "F": F, "thr": thr, "refs": refs, "ithds": [0.5, 1.0, 2.0, 8.0], "mthds": [0.4, 0.6, 1.0]}


def _batch(dfepe, pipe, ithds, mthds):
    return dfepe.compat.correspondence_eval_batch((_dev(pipe["p1"]), _dev(pipe["p2"])), (_dev(pipe["d1"]), _dev(pipe["d2"])), _dev(pipe["F"]),
                                                  pipe["thr"], ithds, mthds)


def test_batch_equals_the_pairs_pushed_one_at_a_time(dfepe, pipe):
    out = {k: v.cpu().numpy() for k, v in _batch(dfepe, pipe, pipe["ithds"], pipe["mthds"]).items()}
    tracker = dfepe.compat.model_wrap.PointTracker(max_length=2, nn_thresh=pipe["thr"])
    rp = dfepe.compat.eval_tools.Result_processor(["epi_dist_mean_gt", "mscores", "num_matches"])
    for b in range(B_PIPE):
        ones = np.ones((1, N_PIPE))
        tracker.update(np.concatenate([pipe["p1"][b].T.astype(np.float64), ones]), pipe["d1"][b].T)
        tracker.update(np.concatenate([pipe["p2"][b].T.astype(np.float64), ones]), pipe["d2"][b].T)
        matches, mscores = tracker.get_matches(), tracker.get_mscores()
        tracker.clear_desc()
        i1, i2, score = pipe["refs"][b].matches(pipe["thr"])
        n = len(i1)
        assert 20 < n < N_PIPE and matches.shape == (4, n) and mscores.shape == (n,) and out["num_matches"][b] == n
        assert np.array_equal(matches.T, np.concatenate([pipe["p1"][b][i1], pipe["p2"][b][i2]], 1).astype(np.float64))
        assert np.array_equal(matches.T.astype(np.float32), out["matches"][b, :n]) and not out["matches"][b, n:].any()
        assert np.array_equal(mscores.astype(np.float32), out["mscores"][b, :n]) and not out["mscores"][b, n:].any()
        sample = {"F": torch.as_tensor(pipe["F"][b:b + 1])}
        d = dfepe.compat.evaluation_epiDist.epi_dist_from_matches(matches.transpose()[np.newaxis, ...], sample, DEV)["epi_dist_mean_gt"]
        assert np.array_equal(d, out["epi_dist_mean_gt"][b, :n]) and not out["epi_dist_mean_gt"][b, n:].any()
        rp.load_result({"epi_dist_mean_gt": d, "mscores": mscores, "num_matches": n})
    for j, mt in enumerate(pipe["mthds"]):
        r = rp.inlier_ratio(rp.get_entry_from_result("epi_dist_mean_gt"), pipe["ithds"], mask_list=rp.get_entry_from_result("mscores"), mask_thd=mt)
        assert np.array_equal(r["num_corrs"], out["num_corrs"][j]) and r["num_corrs"].min() > 0
        assert np.array_equal(r["inlier_ratio"], out["inlier_ratio"][j])
    ap = rp.ap_inlier_thd("epi_dist_mean_gt", pipe["ithds"], pipe["mthds"])
    assert np.array_equal(ap["inlier_thd"], out["inlier_ratio"]) and np.array_equal(ap["num_corrs"], out["num_corrs"])
    # and the table is the restatement's on the batch's own matches
    case = {"name": "pipe", "matches": out["matches"], "F": pipe["F"], "scores": out["mscores"], "n_valid": out["num_matches"],
            "ithds": pipe["ithds"], "mthds": pipe["mthds"], "listed": set()}
    cc.check(case, {"cnt": out["cnt"], "num": out["num"], "ratio": out["ratio"], "dist_out": out["epi_dist_mean_gt"],
                    "mean": out["inlier_ratio"], "num_T": out["num_corrs"]})


def test_batch_honours_counts_and_noise(dfepe, pipe):
    p1, p2, d1, d2, F = (_dev(pipe[k]) for k in ("p1", "p2", "d1", "d2", "F"))
    c1 = torch.tensor([N_PIPE, 100, 0], dtype=torch.int32, device=DEV)
    c2 = torch.tensor([N_PIPE, N_PIPE, 40], dtype=torch.int32, device=DEV)
    noise = torch.full((B_PIPE, N_PIPE, 2), 0.25, device=DEV)
    out = dfepe.compat.correspondence_eval_batch((p1, p2), (d1, d2), F, pipe["thr"], pipe["ithds"], pipe["mthds"], counts=(c1, c2), noise=noise)
    full = _batch(dfepe, pipe, pipe["ithds"], pipe["mthds"])
    n = out["num_matches"].cpu().numpy()
    assert n[0] == full["num_matches"][0].item() and 0 < n[1] <= 100 and n[2] == 0
    assert torch.equal(out["matches"][0, :n[0], 2:], full["matches"][0, :n[0], 2:] + 0.25)
    assert torch.equal(out["matches"][0, :, :2], full["matches"][0, :, :2])
    assert bool(torch.isnan(out["ratio"][2]).all()) and bool(torch.isnan(out["inlier_ratio"]).all()) and not out["num"][2].any()


def test_batch_runs_from_a_captured_graph(dfepe, pipe):
    it, mt = _dev(np.asarray(pipe["ithds"], np.float64)), _dev(np.asarray(pipe["mthds"], np.float64))
    eager = _batch(dfepe, pipe, it, mt)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        _batch(dfepe, pipe, it, mt)  # warm-up on the side stream: the allocator's pools
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    args = ((_dev(pipe["p1"]), _dev(pipe["p2"])), (_dev(pipe["d1"]), _dev(pipe["d2"])), _dev(pipe["F"]))
    with torch.cuda.graph(graph):
        held = dfepe.compat.correspondence_eval_batch(*args, pipe["thr"], it, mt)
    for _ in range(2):
        for v in held.values():
            v.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for key, v in eager.items():
            assert torch.equal(_bits(v), _bits(held[key])), key
