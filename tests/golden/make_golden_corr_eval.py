#!/usr/bin/env python3
"""Golden vectors for the correspondence evaluation, from the reference itself: epi_distance_np of
deepFEPE/dsac_tools/utils_F.py (:363-385) and Result_processor.inlier_ratio (with and without the mask), inlier_ratio_nested,
inlier_ratio_from_est and get_mask of deepFEPE/utils/eval_tools.py (:27-174).  The reference is imported at generation time only:
eval_tools.py through importlib as make_golden_odometry.py does (it needs no stubs), utils_F.py with the stub modules of
make_golden.py (cv2 and the superpoint package, which the functions used here never call).  Only data is written.

    python tests/golden/make_golden_corr_eval.py <path to the reference checkout>     # rewrites tests/golden/corr_eval.npz

tests/golden/corr_eval.npz (described here, not in MANIFEST.txt).  The inputs are corr_eval_cases.golden_inputs(): B = 12 seeded
pairs of n = 1 .. 200 matches; pairs 3 and 11 have every score >= 1, so nothing of them is kept under either mask threshold.
    matches_k [n,4] float32, F_k [3,3] float64, scores_k [n] float32     the inputs of pair k, as golden_inputs() returns them
    ithds [5], mthds [2] float64                                         the inlier and the mask thresholds
    dist3_k, dist1_k, dist2_k [n] float64     epi_distance_np(F_k, x1, x2) with the coordinates widened to float64
    from_est [B,5] float64                    inlier_ratio_from_est(dist3_k, ithds) per pair
    from_est_mask [2,B,5] float64             inlier_ratio_from_est(dist3_k[get_mask(scores_k, mthd)], ithds) (NaN: nothing kept)
    nested [5] float64                        inlier_ratio_nested(all dist3, ithds)
    nomask_mean [5] float64, nomask_num [B]   inlier_ratio(all dist3, ithds): "inlier_ratio" and "num_corrs"
    mask_mean [2,5] float64, mask_num [2,B]   inlier_ratio(all dist3, ithds, mask_list=all scores, mask_thd=mthd) per mask threshold
                                              (NaN: a pair with nothing kept is in the mean)
    kept_pairs [10] int64, kept_mean [2,5] float64, kept_num [2,10]   the same over the pairs that keep something: a finite mean
"""
import contextlib
import importlib.util
import io
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]


def load_reference(root):
    import make_golden as mg

    mg.REF = root
    mg.install_stubs()
    with contextlib.redirect_stdout(io.StringIO()):
        import deepFEPE.dsac_tools.utils_F as utils_F
    spec = importlib.util.spec_from_file_location("ref_eval_tools", os.path.join(root, "deepFEPE", "utils", "eval_tools.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return utils_F.epi_distance_np, mod.Result_processor


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    import corr_eval_cases as cc

    epi_distance_np, Result_processor = load_reference(sys.argv[1])
    pairs = cc.golden_inputs()
    ithds, mthds = list(cc.GOLDEN_ITHDS), list(cc.GOLDEN_MTHDS)
    rp = Result_processor(["epi_dist_mean_gt", "mscores"])
    out = {"ithds": np.asarray(ithds, np.float64), "mthds": np.asarray(mthds, np.float64)}
    dists, scores = [], []
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for k, (m, F, sc) in enumerate(pairs):
            d3, d1, d2 = epi_distance_np(F, m[:, :2].astype(np.float64), m[:, 2:].astype(np.float64))
            assert d3.dtype == np.float64 and d3.shape == (len(m),)
            out.update({f"matches_{k}": m, f"F_{k}": F, f"scores_{k}": sc, f"dist3_{k}": d3, f"dist1_{k}": d1, f"dist2_{k}": d2})
            dists.append(d3)
            scores.append(sc)
        out["from_est"] = np.array([rp.inlier_ratio_from_est(d, ithds) for d in dists])
        out["from_est_mask"] = np.array([[rp.inlier_ratio_from_est(d[rp.get_mask(s, mt)], ithds) for d, s in zip(dists, scores)] for mt in mthds])
        out["nested"] = np.asarray(rp.inlier_ratio_nested(dists, ithds))
        r = rp.inlier_ratio(dists, ithds)
        out["nomask_mean"], out["nomask_num"] = r["inlier_ratio"], r["num_corrs"]
        rs = [rp.inlier_ratio(dists, ithds, mask_list=scores, mask_thd=mt) for mt in mthds]
        out["mask_mean"], out["mask_num"] = np.array([r["inlier_ratio"] for r in rs]), np.array([r["num_corrs"] for r in rs])
        kept = [k for k in range(len(pairs)) if k not in cc.GOLDEN_NONE_KEPT]
        rs = [rp.inlier_ratio([dists[k] for k in kept], ithds, mask_list=[scores[k] for k in kept], mask_thd=mt) for mt in mthds]
        out["kept_pairs"] = np.asarray(kept, np.int64)
        out["kept_mean"], out["kept_num"] = np.array([r["inlier_ratio"] for r in rs]), np.array([r["num_corrs"] for r in rs])
    path = os.path.join(HERE, "corr_eval.npz")
    np.savez_compressed(path, **out)
    print(f"corr_eval.npz: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
