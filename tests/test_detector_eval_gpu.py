"""The detector evaluation on the GPU: every family of tests/detector_eval_cases.py through ops and the same check() as the host
build -- counts, kept sizes, n_unwarped and the AP's integer counts exactly, the continuous outputs within the restatement's
bounds, bit-identical on a second call -- then the compat mirrors against the reference's own outputs (tests/golden/
repeatability.npz) and the batched front-end table against the per-pair calls."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detector_eval_cases as dc  # noqa: E402
import detector_eval_ref as dr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=DEV, dtype=dtype)


def _run(dfepe, job, dtype=torch.float64):
    return dfepe.ops.keypoint_repeatability(_dev(job["kp1"], dtype), _dev(job["kp2"], dtype), _dev(job["H"]), job["height"], job["width"],
                                            job["keep_k"], _dev(np.asarray(job["thresh"], np.float64)), _dev(job["n1"]), _dev(job["n2"]))


@pytest.mark.parametrize("name", list(dc.jobs()))
def test_repeatability_families(dfepe, name):
    job = dc.jobs()[name]
    out = _run(dfepe, job)
    again = _run(dfepe, job)
    for key, v in out.items():
        assert torch.equal(v, again[key]) or (v.dtype.is_floating_point and torch.equal(v.view(torch.int64), again[key].view(torch.int64))), key
    host = {k: v.cpu().numpy() for k, v in out.items()}
    for b in range(len(job["H"])):
        dc.check({k: v[b] for k, v in host.items()}, name, b, what="gpu")


def test_float32_keypoints_are_upcast_exactly(dfepe):
    """The lattice is exact in float32 too: the same counts, bit for bit the same values."""
    job = dc.jobs()["lattice"]
    a, b = _run(dfepe, job), _run(dfepe, job, torch.float32)
    for key in a:
        assert torch.equal(a[key], b[key]), key


def test_inputs_are_not_written_to(dfepe):
    job = dc.jobs()["projective_k"]
    kp1, kp2, H = _dev(job["kp1"]), _dev(job["kp2"]), _dev(job["H"])
    keep = kp1.clone(), kp2.clone(), H.clone()
    dfepe.ops.keypoint_repeatability(kp1, kp2, H, job["height"], job["width"], job["keep_k"], _dev(np.asarray(job["thresh"])))
    assert torch.equal(kp1, keep[0]) and torch.equal(kp2, keep[1]) and torch.equal(H, keep[2])


@pytest.mark.parametrize("name", list(dc.ap_jobs()))
def test_average_precision_families(dfepe, name):
    lab, sc, nv = dc.ap_jobs()[name]
    run = lambda: dfepe.ops.average_precision(_dev(lab), _dev(sc), _dev(nv), want_counts=True)  # noqa: E731
    out, again = run(), run()
    assert torch.equal(out["ap"].view(torch.int64), again["ap"].view(torch.int64))
    host = {k: v.cpu().numpy() for k, v in out.items()}
    for b in range(len(lab)):
        dc.check_ap({k: v[b] for k, v in host.items()}, name, b, what="gpu")
    plain = dfepe.ops.average_precision(_dev(lab), _dev(sc), _dev(nv))  # without the optional outputs: the same ap
    assert plain["tp_at"] is None and torch.equal(plain["ap"].view(torch.int64), out["ap"].view(torch.int64))


def test_matching_score(dfepe):
    rows = [(5, 10, 10), (7, 0, 3), (3, 1000, 999), (0, 5, 5), (2 ** 30, 2 ** 30, 2 ** 30), (0, 0, 0), (4, 0, 0)]
    cols = [_dev(np.array(c, np.int32)) for c in zip(*rows)]
    got = dfepe.ops.matching_score(*cols).cpu().numpy()
    for g, r in zip(got, rows):
        want = dr.matching_score(*r)
        assert g == want or (np.isnan(g) and np.isnan(want)), (r, g, want)


def _golden_data(g, i):
    h, w, k, th = g[f"c{i}_par"]
    data = {"prob": g[f"c{i}_kp1"].copy(), "warped_prob": g[f"c{i}_kp2"].copy(), "homography": g[f"c{i}_H"].copy(), "image": np.zeros((int(h), int(w)))}
    return data, int(k), float(th), g[f"c{i}_out"]


def test_compat_compute_repeatability_reproduces_the_reference(dfepe, golden):
    """The reference's own outputs: repeatability exactly, the localization error within the restatement's bound; (0, -1) for the
    empty and the all-outside pairs; and the caller's data is left as it was, which the reference does not do."""
    g = golden("repeatability")
    for i in range(int(g["n_cases"][0])):
        data, k, th, want = _golden_data(g, i)
        before = {key: v.copy() for key, v in data.items()}
        rep, loc = dfepe.compat.detector_evaluation.compute_repeatability(data, keep_k_points=k, distance_thresh=th)
        for key, v in before.items():
            assert np.array_equal(data[key], v), (i, key)
        assert rep == want[0], (i, rep, want[0])
        if want[1] == -1:
            assert (rep, loc) == (0, -1), i
        else:
            r = dr.repeatability_pair(data["prob"], data["warped_prob"], data["homography"], *data["image"].shape, k, [th])
            assert abs(loc - want[1]) <= dr.TOL * r["loc_err_bound"][0], (i, loc, want[1])


def test_compat_average_precision_reproduces_scikit_learn(dfepe, golden):
    g = golden("repeatability")
    for i in range(int(g["n_ap"][0])):
        lab, sc, want = g[f"a{i}_labels"], g[f"a{i}_scores"], g[f"a{i}_ap"][0]
        got = dfepe.ops.average_precision(_dev(lab[None]), _dev(sc[None]))["ap"][0].item()
        assert abs(got - want) <= dr.TOL * dr.average_precision(lab, sc)["ap_bound"], (i, got, want)
    dist = np.array([0.2, 0.9, 0.5, 0.9, 0.1], np.float32)
    lab = np.array([1, 0, 1, 1, 0])
    r = dr.average_precision(lab, (dist.max() - dist).astype(np.float64))
    assert abs(dfepe.compat.evaluate_frontend.nn_average_precision(dist, lab) - r["ap"]) <= dr.TOL * r["ap_bound"]


def _frontend_pairs(B=3, N=64, D=32):
    rng = np.random.default_rng(5)
    out = []
    for b in range(B):
        kp1, kp2, H = dc.seeded_pair(500 + b, N, N, spill=0.05)
        d1 = rng.normal(size=(N, D))
        d1 /= np.linalg.norm(d1, axis=1, keepdims=True)
        # image-2 descriptors: a noisy copy of a random image-1 descriptor each, so that two-way matches exist and some are wrong
        src = rng.permutation(N)
        d2 = d1[src] + 0.25 * rng.normal(size=(N, D)) / np.sqrt(D)
        d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
        hom = np.concatenate([kp1[src, :2], np.ones((N, 1))], 1) @ H.T
        kp2[:, :2] = hom[:, :2] / hom[:, 2:] + rng.uniform(-2.5, 2.5, (N, 2))
        out.append({"prob": kp1, "warped_prob": kp2, "desc": d1.astype(np.float32), "warped_desc": d2.astype(np.float32), "homography": H,
                    "image": np.zeros((dc.HEIGHT, dc.WIDTH))})
    return out


@pytest.mark.parametrize("method", ["gt", "cv"])
def test_frontend_metrics_batch_agrees_with_the_per_pair_calls(dfepe, method):
    ef, de_, ds = dfepe.compat.evaluate_frontend, dfepe.compat.detector_evaluation, dfepe.compat.descriptor_evaluation
    pairs = _frontend_pairs()
    st = lambda key, dt: _dev(np.stack([p[key] for p in pairs]), dt)  # noqa: E731
    out = ef.frontend_metrics_batch(st("prob", torch.float64), st("warped_prob", torch.float64), st("desc", torch.float32),
                                    st("warped_desc", torch.float32), st("homography", torch.float64), (dc.HEIGHT, dc.WIDTH),
                                    inliers_method=method)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    tracker = dfepe.compat.model_wrap.PointTracker(max_length=2, nn_thresh=ef.NN_THRESH)
    for b, d in enumerate(pairs):
        rep, loc = de_.compute_repeatability(d, keep_k_points=300, distance_thresh=3)
        assert (rep, loc) == (out["repeatability"][b], out["localization_err"][b]), b
        res = ds.compute_homography(d, correctness_thresh=[1, 3, 5], shape=(dc.HEIGHT, dc.WIDTH))
        assert np.array_equal(np.asarray(res["correctness"]).astype(np.uint8), out["correctness"][b]), b
        ms = ef.matching_score(res["inliers"], d["prob"], d["warped_prob"], d["homography"], d["image"].shape)
        assert ms == out["mscore"][b] and 0 < ms <= 1, (b, ms)
        m = tracker.nn_match_two_way(d["desc"].T, d["warped_desc"].T, ef.NN_THRESH)
        assert m.shape[1] == out["nn_count"][b] > 8
        xy = np.concatenate([d["prob"][m[0].astype(int), :2], d["warped_prob"][m[1].astype(int), :2]], 1)
        labels = ds.get_inliers(xy, d["homography"], 3) if method == "gt" else ds.get_inliers_cv(xy.astype(np.float32))
        ap = ef.nn_average_precision(m[2].astype(np.float32), labels)
        assert ap == out["mAP"][b] and 0 < ap <= 1, (b, ap, out["mAP"][b])
    means = ef.evaluate(pairs, rep_thd=3, inliers_method=method)
    assert means["repeatability"] == np.mean(out["repeatability"]) and means["mAP"] == np.mean(out["mAP"])
    assert means["mscore"] == np.mean(out["mscore"]) and np.array_equal(means["correctness"], out["correctness"].astype(np.float64).mean(0))
    assert means["localization_err"] == np.mean(out["localization_err"][out["localization_err"] > 0])
