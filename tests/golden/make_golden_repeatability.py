#!/usr/bin/env python3
"""Golden vectors for the front-end detector evaluation (dfepe_keypoint_repeatability, dfepe_average_precision): the reference's
own compute_repeatability on a dozen small pairs, and scikit-learn's average_precision_score on tied and untied vectors.

    python tests/golden/make_golden_repeatability.py <path to the reference checkout>     # rewrites tests/golden/repeatability.npz

The reference is imported here, at generation time, and nowhere else; `settings` (which only names an experiment folder) is
stubbed.  compute_repeatability overwrites its input, so every call gets a copy; its prints are swallowed.  Only data is stored
(tests/golden/repeatability.npz, 83 arrays, 29807 bytes, written with numpy 2.2.6 and scikit-learn 1.7.2; described here, not in
MANIFEST.txt, which like every existing file under tests/ is left as it is):

    n_cases, then per case i:  c<i>_kp1 [n1,C], c<i>_kp2 [n2,C] float64 rows (x, y[, prob]);  c<i>_H [3,3];  c<i>_par = (height, width,
        keep_k, thresh) float64;  c<i>_out = (repeatability, localization_err) float64 as returned
    n_ap, then per vector i:   a<i>_labels [m] uint8, a<i>_scores [m] float64, a<i>_ap [1] float64

The probabilities of every case are distinct: numpy's default argsort, which the reference calls, is not stable, so with equal
probabilities at the k-th place the reference itself is undefined.  The cases come from tests/detector_eval_cases.golden_inputs(),
so that the tests can check they hold what the file holds.
"""
import contextlib
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import detector_eval_cases as dc  # noqa: E402


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    root = sys.argv[1]
    sys.modules["settings"] = types.SimpleNamespace(EXPER_PATH="")
    sys.path.insert(0, root)
    from evaluations.detector_evaluation import compute_repeatability
    from sklearn.metrics import average_precision_score

    out = {}
    cases = dc.golden_inputs()
    out["n_cases"] = np.array([len(cases)])
    for i, (kp1, kp2, H, h, w, k, th) in enumerate(cases):
        data = {"prob": kp1.copy(), "warped_prob": kp2.copy(), "homography": H.copy(), "image": np.zeros((h, w))}
        with contextlib.redirect_stdout(io.StringIO()):
            rep, loc = compute_repeatability(data, keep_k_points=k, distance_thresh=th)
        out[f"c{i}_kp1"], out[f"c{i}_kp2"], out[f"c{i}_H"] = kp1, kp2, H
        out[f"c{i}_par"] = np.array([h, w, k, th], np.float64)
        out[f"c{i}_out"] = np.array([rep, loc], np.float64)
        print(f"case {i}: n1 {len(kp1)} n2 {len(kp2)} k {k} thresh {th} -> {rep} {loc}")
    vecs = dc.golden_ap_inputs()
    out["n_ap"] = np.array([len(vecs)])
    for i, (lab, sc) in enumerate(vecs):
        out[f"a{i}_labels"], out[f"a{i}_scores"] = lab, sc
        out[f"a{i}_ap"] = np.array([average_precision_score(lab, sc)], np.float64)
        print(f"ap {i}: m {len(lab)} -> {out[f'a{i}_ap'][0]!r}")
    path = os.path.join(HERE, "repeatability.npz")
    np.savez_compressed(path, **out)
    print(f"repeatability.npz: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
