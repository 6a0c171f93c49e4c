#!/usr/bin/env python3
"""Golden vectors for the KITTI odometry table (dfepe_trajectory_align, dfepe_kitti_odometry_errors), from the data the reference
ships for that stage.  Nothing of the reference is executed or restated here: the script only reads text files of numbers.

    python tests/golden/make_golden_kitti_odom.py <path to the reference checkout>     # rewrites tests/golden/kitti_odom.npz

What it reads:
    results/{deepFEPE_kitti,deepF_kitti}/{09,10}/{09,10}.txt       estimated trajectories, one 3x4 pose (12 numbers) per line
    deepFEPE/datasets/kitti_gt_poses/{09,10}.txt                   ground-truth trajectories, the same layout
    results/<run>/<seq>/errors/<seq>.txt                           one row `first_frame r_err t_err len speed` per scored segment
    results/<run>/<seq>/result.txt                                 the five published numbers of the sequence

tests/golden/kitti_odom.npz (described here, not in MANIFEST.txt).  Runs are deepFEPE and deepF, sequences 09 (1591 frames) and 10
(1201 frames); keys carry <run>_<seq>:
    est_<run>_<seq>     [n,3,4] float32   the estimated absolute poses.  The text holds float32 values printed with 18 digits; the
                                          script asserts that the float32 array reproduces the parsed float64 values exactly
    gt_<seq>            [n,3,4] float64   the ground truth as parsed: six-digit text, not float32-exact
    errors_<run>_<seq>  [k,5]   float64   the shipped segment rows (k = 958 for 09 and 464 for 10, in both runs)
    result_<run>_<seq>  [5]     float64   Trans. err. (%), Rot. err. (deg/100m), ATE (m), RPE (m), RPE (deg) as printed (three decimals)
"""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
RUNS = {"deepFEPE": "deepFEPE_kitti", "deepF": "deepF_kitti"}
SEQS = ("09", "10")
RESULT_LINES = ("Trans. err. (%)", "Rot. err. (deg/100m)", "ATE (m)", "RPE (m)", "RPE (deg)")


def read_result(path):
    text = open(path).read()
    out = []
    for label in RESULT_LINES:
        m = re.search(re.escape(label) + r":\s*([-+0-9.eE]+)", text)
        assert m, (path, label)
        out.append(float(m.group(1)))
    return np.array(out, np.float64)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    root = sys.argv[1]
    out = {}
    for seq in SEQS:
        gt = np.loadtxt(os.path.join(root, "deepFEPE", "datasets", "kitti_gt_poses", seq + ".txt"), dtype=np.float64)
        out[f"gt_{seq}"] = gt.reshape(-1, 3, 4)
        for run, folder in RUNS.items():
            d = os.path.join(root, "results", folder, seq)
            est = np.loadtxt(os.path.join(d, seq + ".txt"), dtype=np.float64)
            est32 = est.astype(np.float32)
            assert np.array_equal(est32.astype(np.float64), est), "the estimate is not float32-exact"
            assert len(est) == len(gt)
            out[f"est_{run}_{seq}"] = est32.reshape(-1, 3, 4)
            out[f"errors_{run}_{seq}"] = np.loadtxt(os.path.join(d, "errors", seq + ".txt"), dtype=np.float64).reshape(-1, 5)
            out[f"result_{run}_{seq}"] = read_result(os.path.join(d, "result.txt"))
    path = os.path.join(HERE, "kitti_odom.npz")
    np.savez_compressed(path, **out)
    print(f"kitti_odom.npz: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
