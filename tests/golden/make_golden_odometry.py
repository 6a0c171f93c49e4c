#!/usr/bin/env python3
"""Golden vectors for the odometry evaluation, from the reference itself: Exp_table_processor.get_abs_poses, compensate_poses,
compute_pose_error and pose_seq_ate of deepFEPE/utils/eval_tools.py (:252-375), loaded unmodified through importlib (the module
imports only logging, numpy and torch at module level, so no stubs are needed).

    python tests/golden/make_golden_odometry.py <path to the reference checkout>     # rewrites tests/golden/odometry.npz

The one thing restated here instead of run: relative_pose_cam_to_body is a function nested inside a method
(Train_model_pipeline.py:1098-1108) and cannot be imported; its body is the single expression
numpy.linalg.inv(Rt_cam2_gt) @ relative_scene_pose @ Rt_cam2_gt, which `cam_to_body` below repeats with numpy.

tests/golden/odometry.npz (described here, not in MANIFEST.txt).  Two sequences, s = 0 with n = 300 and s = 1 with n = 37
relative poses; keys carry the sequence index as a suffix:
    rel_cam_s     [n,3,4] float32  seeded synthetic camera motions: rotation vector ~ N(0, 0.03^2) per axis, translation ~
                                   N(0, diag(0.05, 0.02, 1)^2) + (0, 0, 1) (a vehicle that keeps moving), rounded to float32 as
                                   the network's output is
    cam2body_s    [3,4]   float32  the sequence's Rt_cam2_gt (a fixed rotation of ~0.1 rad and an offset), float32 as the loader's
    rel_body_s    [n,3,4] float64  cam_to_body of the above (4x4, widened to float64), rows 0..2
    abs_s         [n+1,3,4] float64  get_abs_poses(rel_body as 4x4 matrices)
    gt_s          [n+1,3,4] float32  ground truth: get_abs_poses of a perturbed, rescaled motion (the camera motion's rotation
                                   vector + N(0, 0.002^2), rel_body's translation x 1.7 + N(0, 0.01^2)), rounded to float32 as
                                   read_gt_poses returns it.  It is WIDENED to float64 before it is scored: numpy.stack keeps a
                                   float32 array float32, so the reference would compensate a float32 ground truth in float32
                                   arithmetic; the kernels are fp64 throughout and are pinned to the reference's fp64 behaviour
    errors5_s [n+1-5,2] float32, scale5_s [n+1-5] float64, aligned5_s [n+1-5,3,4] float64   pose_seq_ate(abs, gt, 5)
    errors3_s, scale3_s                                                                     pose_seq_ate(abs, gt, 3)
    comp_est_s, comp_gt_s [5,3,4] float64   compensate_poses of abs[10:15] and of gt[10:15]
    cpe_s [3] float64                        compute_pose_error(comp_est, comp_gt): ATE, RE, scale_factor
"""
import contextlib
import importlib.util
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def load_reference(root):
    path = os.path.join(root, "deepFEPE", "utils", "eval_tools.py")
    spec = importlib.util.spec_from_file_location("ref_eval_tools", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Exp_table_processor


def rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def pose44(R, t):
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, t
    return M


def cam_to_body(relative_scene_pose, Rt_cam2_gt):
    return np.linalg.inv(Rt_cam2_gt) @ relative_scene_pose @ Rt_cam2_gt


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    P = load_reference(sys.argv[1])
    out = {}
    for s, (n, seed) in enumerate(((300, 2024), (37, 2025))):
        g = np.random.RandomState(seed)
        w = 0.03 * g.randn(n, 3)
        t = g.randn(n, 3) * np.array([0.05, 0.02, 1.0]) + np.array([0.0, 0.0, 1.0])
        rel_cam = np.stack([pose44(rodrigues(w[i]), t[i])[:3] for i in range(n)]).astype(np.float32)
        c2b = pose44(rodrigues(np.array([0.08, -0.05, 0.03])), np.array([0.3, -0.1, 1.2]))[:3].astype(np.float32)
        C = pose44(c2b[:, :3].astype(np.float64), c2b[:, 3].astype(np.float64))
        rel_body = [cam_to_body(pose44(rel_cam[i, :, :3].astype(np.float64), rel_cam[i, :, 3].astype(np.float64)), C)
                    for i in range(n)]
        gt_rel = [pose44(rodrigues(w[i] + 0.002 * g.randn(3)), 1.7 * rel_body[i][:3, 3] + 0.01 * g.randn(3)) for i in range(n)]
        with contextlib.redirect_stdout(io.StringIO()):
            abs_poses = P.get_abs_poses(rel_body)
            gt = P.get_abs_poses(gt_rel).astype(np.float32)
            gt64 = gt.astype(np.float64)
            r5 = P.pose_seq_ate(abs_poses, gt64, 5)
            r3 = P.pose_seq_ate(abs_poses, gt64, 3)
            ce, cg = P.compensate_poses(abs_poses[10:15]), P.compensate_poses(gt64[10:15])
            cpe = P.compute_pose_error(ce, cg)
        assert r5["errors"].dtype == np.float32 and abs_poses.dtype == np.float64 and abs_poses.shape == (n + 1, 3, 4)
        out.update({
            f"rel_cam_{s}": rel_cam, f"cam2body_{s}": c2b, f"rel_body_{s}": np.stack(rel_body)[:, :3], f"abs_{s}": abs_poses,
            f"gt_{s}": gt, f"errors5_{s}": r5["errors"], f"scale5_{s}": np.array(r5["scale_factors"], np.float64),
            f"aligned5_{s}": np.stack(r5["aligned_poses"]), f"errors3_{s}": r3["errors"],
            f"scale3_{s}": np.array(r3["scale_factors"], np.float64), f"comp_est_{s}": ce, f"comp_gt_{s}": cg,
            f"cpe_{s}": np.array([cpe["ATE"], cpe["RE"], cpe["scale_factor"]], np.float64),
        })
    path = os.path.join(HERE, "odometry.npz")
    np.savez_compressed(path, **out)
    print(f"odometry.npz: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
