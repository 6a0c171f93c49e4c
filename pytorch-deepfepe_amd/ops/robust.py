"""The robust estimators (csrc/ransac.hip, ransac5.hip, lmeds.hip, homography.hip): RANSAC and LMedS fits of F, E and H, and the
poses of the F and E fits.  The estimators share one output dictionary; the pose functions share one tail."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from ._base import Tensor, _h9, _n_valid_arg, _on, _on_gpu, _prep, _ptr, _shape, _stream, _workspace
from .geometry import cheirality, congruence, project_essential


def _estimate_out(model: str, dtype, best: str, B: int, N: int, dev, extras=(), want_masked: Optional[bool] = None) -> dict:
    """The outputs every estimator fills, in the documented order: the model, mask, n_inliers, iters_run, ``best`` (best_hyp [B,2]
    or best_iter [B]), the estimator's ``extras`` and masked (want_masked None: the estimator has none).  An entry is (key, shape,
    dtype); a shape of None is an output nobody asked for."""
    rows = [(model, (B, 3, 3), dtype), ("mask", (B, N), torch.uint8), ("n_inliers", (B,), torch.int32), ("iters_run", (B,), torch.int32),
            (best, (B, 2) if best == "best_hyp" else (B,), torch.int32), *extras]
    if want_masked is not None:
        rows.append(("masked", (B, N, 4) if want_masked else None, torch.float32))
    return {key: None if shape is None else torch.empty(shape, device=dev, dtype=dt) for key, shape, dt in rows}


def _recover_pose_camera(K: Tensor) -> Tensor:
    """K [B,3,3] -> the camera the reference hands cv2.recoverPose: focal K00, principal point (K02, K12) (utils_opencv.py:177)."""
    Kp = torch.zeros_like(K)
    Kp[:, 0, 0] = Kp[:, 1, 1] = K[:, 0, 0]
    Kp[:, 0, 2], Kp[:, 1, 2], Kp[:, 2, 2] = K[:, 0, 2], K[:, 1, 2], 1.0
    return Kp


def _pose_tail(out: dict, E: Tensor, Kp: Tensor, depth_thres: float) -> dict:
    """cv2.recoverPose(E, x1, x2, camera Kp, mask=inliers) added to an estimator's dict: the cheirality kernel on its masked
    matches, and the correspondences the winner sees in front of both cameras."""
    Rt, win, cnt = cheirality(E, Kp, out["masked"], depth_thres)
    out.update({"Rt_cam": Rt, "winner": win, "counts": cnt, "in_front": ransac_in_front(E, Kp, out["masked"], win, depth_thres)})
    return out


def _fundamental_pose(estimate, matches: Tensor, K: Tensor, K_pose: Optional[Tensor], depth_thres: float, *args) -> dict:
    """The common body of ransac_pose and lmeds_pose: ``estimate`` is ransac_fundamental or lmeds_fundamental, args its own."""
    K = _prep(K, "K")
    out = estimate(matches, *args, want_masked=True)
    B = out["F"].shape[0]
    _shape(K, "K (one intrinsic matrix per pair)", B, 3, 3)
    Kp = K if K_pose is None else _prep(K_pose, "K_pose")
    out["E"] = project_essential(congruence(out["F"], K))
    return _pose_tail(out, out["E"], Kp, depth_thres)


def _essential_pose(estimate, matches: Tensor, K: Tensor, depth_thres: float, *args) -> dict:
    """The common body of ransac_essential_pose and lmeds_essential_pose: ``estimate`` is ransac_essential or lmeds_essential."""
    Kp = _recover_pose_camera(_prep(K, "K"))
    out = estimate(matches, Kp, *args, want_masked=True)
    return _pose_tail(out, out["E"], Kp, depth_thres)


def ransac_fundamental(matches: Tensor, threshold: float = 0.1, confidence: float = 0.99, max_iters: int = 1000, seed: int = 0,
                       want_hyp_counts: bool = False, want_masked: bool = False):
    """matches [B,N,4] pixels -> robust F of every pair by OpenCV 3.4's findFundamentalMat(FM_RANSAC) algorithm (the validation
    baseline, utils_opencv.py:157; include/dfepe.h spells out the sampler, the 7-point solve, the error and the stopping rule).
    Returns dict(F [B,3,3] (F22 = 1; zeros without a model), mask [B,N] uint8, n_inliers [B], iters_run [B], best_hyp [B,2]
    (iteration, root; -1 without a model), hyp_counts [B,max_iters,3] | None (-1: no root, -2: no sample), masked [B,N,4] | None
    (non-inlier rows NaN)).  No host synchronisation.  15 <= N <= 4096: below 15 OpenCV runs LMedS, which is lmeds_fundamental."""
    m = _prep(matches, "matches")
    _shape(m, "matches (pixel x1,y1,x2,y2)", None, None, 4)
    B, N = m.shape[0], m.shape[1]
    if N < _lib.RANSAC_MIN_N:
        raise _lib.DfepeError(f"ransac_fundamental: {N} correspondences per pair; the RANSAC estimator needs at least "
                              f"{_lib.RANSAC_MIN_N} (OpenCV switches to LMedS below that, which is not built into this entry: see lmeds_fundamental)")
    L = _lib.lib()
    dev = m.device
    ws = _workspace(L.dfepe_ransac_workspace_bytes(B, N, int(max_iters)), dev)
    out = _estimate_out("F", torch.float32, "best_hyp", B, N, dev,
                        [("hyp_counts", (B, int(max_iters), 3) if want_hyp_counts else None, torch.int32)], bool(want_masked))
    with _on(dev):
        rc = L.dfepe_ransac_fundamental(_ptr(m), B, N, float(threshold), float(confidence), int(max_iters), int(seed) & ((1 << 64) - 1),
                                        _ptr(ws), _ptr(out["F"]), _ptr(out["mask"]), _ptr(out["n_inliers"]), _ptr(out["iters_run"]),
                                        _ptr(out["best_hyp"]), _ptr(out["hyp_counts"]), _ptr(out["masked"]), _stream())
    _lib.check(rc, "dfepe_ransac_fundamental")
    return out


def ransac_in_front(E: Tensor, K: Tensor, matches: Tensor, winner: Tensor, depth_thres: float = 50.0) -> Tensor:
    """[B,N] uint8: the correspondences the winning candidate of cheirality(E, K, matches, depth_thres) sees in front of both
    cameras (cv2.recoverPose's mask output); a row sums to that call's counts[winner]."""
    E, K, m = _prep(E, "E"), _prep(K, "K"), _prep(matches, "matches")
    _shape(m, "matches (pixel x1,y1,x2,y2)", None, None, 4)
    B, N = m.shape[0], m.shape[1]
    _shape(E, "E", B, 3, 3)
    _shape(K, "K (one intrinsic matrix per pair)", B, 3, 3)
    if winner.shape != (B,) or winner.dtype != torch.int32 or not winner.is_contiguous():
        raise ValueError("winner must be the contiguous [B] int32 output of cheirality")
    mask = torch.empty(B, N, device=m.device, dtype=torch.uint8)
    with _on(m.device):
        rc = _lib.lib().dfepe_ransac_in_front(_ptr(E), _ptr(K), _ptr(m), B, N, float(depth_thres), _ptr(winner), _ptr(mask), _stream())
    _lib.check(rc, "dfepe_ransac_in_front")
    return mask


def ransac_pose(matches: Tensor, K: Tensor, threshold: float = 0.1, confidence: float = 0.99, max_iters: int = 1000, seed: int = 0,
                depth_thres: float = 50.0, K_pose: Optional[Tensor] = None):
    """The 8-point baseline of utils_opencv.recover_camera_opencv (utils_opencv.py:157-177) for every pair: ransac_fundamental,
    E = K^T F K projected onto singular values (1, 1, 0), then cv2.recoverPose(E, x1, x2, camera K_pose, mask=inliers): the
    unchanged cheirality kernel on the matches with the non-inlier rows set to NaN (a NaN row passes no depth test).
    K_pose: the camera recoverPose is given (default K; the reference passes focal K[0,0] and principal point (K[0,2], K[1,2])).
    Returns the ransac_fundamental dict with E [B,3,3], Rt_cam [B,3,4], winner [B], counts [B,4] and in_front [B,N] uint8 added."""
    return _fundamental_pose(ransac_fundamental, matches, K, K_pose, depth_thres, threshold, confidence, max_iters, seed)


def ransac_essential(matches: Tensor, K: Tensor, threshold: float = 1.0, confidence: float = 0.999, max_iters: int = 1000, seed: int = 0,
                     want_hyp_counts: bool = False, want_hyp_E: bool = False, want_masked: bool = False):
    """matches [B,N,4] pixels, K [B,3,3] -> robust E of every pair by OpenCV 3.4's findEssentialMat(RANSAC) algorithm, the
    five-point baseline (utils_opencv.py:147-151; include/dfepe.h spells out the normalisation, the sampler, the five-point solve,
    the Sampson score and the stopping rule).  The defaults are cv2's own for findEssentialMat.
    Returns dict(E [B,3,3] (unit Frobenius norm, largest entry positive; zeros without a model), mask [B,N] uint8, n_inliers [B],
    iters_run [B], best_hyp [B,2] (iteration, root; -1 without a model), hyp_counts [B,max_iters,10] | None (-1: no root), hyp_E
    [B,max_iters,10,3,3] float64 | None (the hypotheses; unused slots zero), masked [B,N,4] | None (non-inlier rows NaN)).
    No host synchronisation.  6 <= N <= 4096."""
    m, K = _prep(matches, "matches"), _prep(K, "K")
    _shape(m, "matches (pixel x1,y1,x2,y2)", None, None, 4)
    B, N = m.shape[0], m.shape[1]
    _shape(K, "K (one intrinsic matrix per pair)", B, 3, 3)
    if N < _lib.RANSAC5_MIN_N:
        raise _lib.DfepeError(f"ransac_essential: {N} correspondences per pair; the five-point RANSAC estimator needs at least "
                              f"{_lib.RANSAC5_MIN_N}")
    L = _lib.lib()
    dev = m.device
    T = int(max_iters)
    ws = _workspace(L.dfepe_ransac5_workspace_bytes(B, N, T), dev)
    out = _estimate_out("E", torch.float32, "best_hyp", B, N, dev,
                        [("hyp_counts", (B, T, 10) if want_hyp_counts else None, torch.int32),
                         ("hyp_E", (B, T, 10, 3, 3) if want_hyp_E else None, torch.float64)], bool(want_masked))
    with _on(dev):
        rc = L.dfepe_ransac_essential(_ptr(m), _ptr(K), B, N, float(threshold), float(confidence), T, int(seed) & ((1 << 64) - 1),
                                      _ptr(ws), _ptr(out["E"]), _ptr(out["mask"]), _ptr(out["n_inliers"]), _ptr(out["iters_run"]),
                                      _ptr(out["best_hyp"]), _ptr(out["hyp_counts"]), _ptr(out["hyp_E"]), _ptr(out["masked"]), _stream())
    _lib.check(rc, "dfepe_ransac_essential")
    return out


def ransac_essential_pose(matches: Tensor, K: Tensor, threshold: float = 1.0, confidence: float = 0.999, max_iters: int = 1000,
                          seed: int = 0, depth_thres: float = 50.0):
    """The five-point baseline of utils_opencv.recover_camera_opencv(five_point=True) (utils_opencv.py:147-151,177) for every
    pair: ransac_essential with the camera recover_pose_camera(K) -- the reference gives findEssentialMat and recoverPose the same
    focal length and principal point -- then cv2.recoverPose(E, x1, x2, that camera, mask=inliers): E goes to the unchanged
    cheirality kernel as it is (no K^T F K, no projection), on the matches with the non-inlier rows set to NaN.
    Returns the ransac_essential dict with Rt_cam [B,3,4], winner [B], counts [B,4] and in_front [B,N] uint8 added."""
    return _essential_pose(ransac_essential, matches, K, depth_thres, threshold, confidence, max_iters, seed)


def _lmeds(name: str, m: Tensor, K: Optional[Tensor], model_points: int, confidence: float, max_iters: int, seed: int,
           want_hyp_medians: bool, want_masked: bool):
    """The common body of lmeds_fundamental (K None, model_points 7) and lmeds_essential (model_points 5)."""
    B, N = m.shape[0], m.shape[1]
    L = _lib.lib()
    dev = m.device
    niters = int(L.dfepe_lmeds_num_iters(model_points, float(confidence), int(max_iters)))
    if niters < 0:
        _lib.check(niters, "dfepe_lmeds_num_iters")
    roots = 3 if model_points == 7 else 10
    ws = _workspace(L.dfepe_lmeds_workspace_bytes(B, model_points, float(confidence), int(max_iters)), dev)
    out = _estimate_out(name, torch.float32, "best_hyp", B, N, dev,
                        [("min_median", (B,), torch.float64), ("sigma", (B,), torch.float64),
                         ("hyp_medians", (B, niters, roots) if want_hyp_medians else None, torch.float64)], bool(want_masked))
    tail = (B, N, float(confidence), int(max_iters), int(seed) & ((1 << 64) - 1), _ptr(ws), _ptr(out[name]), _ptr(out["mask"]),
            _ptr(out["n_inliers"]), _ptr(out["iters_run"]), _ptr(out["best_hyp"]), _ptr(out["min_median"]), _ptr(out["sigma"]),
            _ptr(out["hyp_medians"]), _ptr(out["masked"]), _stream())
    with _on(dev):
        rc = L.dfepe_lmeds_fundamental(_ptr(m), *tail) if K is None else L.dfepe_lmeds_essential(_ptr(m), _ptr(K), *tail)
    _lib.check(rc, "dfepe_lmeds_fundamental" if K is None else "dfepe_lmeds_essential")
    return out


def lmeds_fundamental(matches: Tensor, confidence: float = 0.99, max_iters: int = 1000, seed: int = 0, want_hyp_medians: bool = False,
                      want_masked: bool = False):
    """matches [B,N,4] pixels -> least-median-of-squares F of every pair: OpenCV 3.4's LMedS, which cv2.findFundamentalMat(..,
    cv2.RANSAC, ..) runs instead of RANSAC below 15 correspondences (utils_opencv.py:157; include/dfepe.h spells out the six
    steps).  No threshold: the inlier bound comes from the winning median.
    Returns dict(F [B,3,3] (F22 = 1; zeros without a model), mask [B,N] uint8, n_inliers [B], iters_run [B], best_hyp [B,2]
    (iteration, root; -1 without a model), min_median [B] float64, sigma [B] float64, hyp_medians [B,niters,3] float64 | None
    (-1: no root, -2: no sample; niters = 300 for the default confidence), masked [B,N,4] | None (non-inlier rows NaN)).
    No host synchronisation.  8 <= N <= 4096."""
    m = _prep(matches, "matches")
    _shape(m, "matches (pixel x1,y1,x2,y2)", None, None, 4)
    if m.shape[1] < _lib.LMEDS_MIN_N:
        raise _lib.DfepeError(f"lmeds_fundamental: {m.shape[1]} correspondences per pair; the LMedS estimator needs at least "
                              f"{_lib.LMEDS_MIN_N} (with 7 OpenCV solves the one sample directly, which is not built)")
    return _lmeds("F", m, None, 7, confidence, max_iters, seed, want_hyp_medians, want_masked)


def lmeds_pose(matches: Tensor, K: Tensor, confidence: float = 0.99, max_iters: int = 1000, seed: int = 0, depth_thres: float = 50.0,
               K_pose: Optional[Tensor] = None):
    """ransac_pose with lmeds_fundamental in place of ransac_fundamental: what utils_opencv.recover_camera_opencv computes for a
    pair with fewer than 15 correspondences (utils_opencv.py:157-177).  Returns the lmeds_fundamental dict with E [B,3,3], Rt_cam
    [B,3,4], winner [B], counts [B,4] and in_front [B,N] uint8 added."""
    return _fundamental_pose(lmeds_fundamental, matches, K, K_pose, depth_thres, confidence, max_iters, seed)


def lmeds_essential(matches: Tensor, K: Tensor, confidence: float = 0.999, max_iters: int = 1000, seed: int = 0,
                    want_hyp_medians: bool = False, want_masked: bool = False):
    """matches [B,N,4] pixels, K [B,3,3] -> least-median-of-squares E of every pair by five-point models: OpenCV 3.4's
    findEssentialMat(method=LMEDS) (include/dfepe.h, dfepe_lmeds_essential).  Returns the dict of lmeds_fundamental with E [B,3,3]
    (unit Frobenius norm; zeros without a model) in place of F and hyp_medians [B,niters,10].  No host synchronisation.
    6 <= N <= 4096."""
    m, K = _prep(matches, "matches"), _prep(K, "K")
    _shape(m, "matches (pixel x1,y1,x2,y2)", None, None, 4)
    _shape(K, "K (one intrinsic matrix per pair)", m.shape[0], 3, 3)
    if m.shape[1] < _lib.LMEDS5_MIN_N:
        raise _lib.DfepeError(f"lmeds_essential: {m.shape[1]} correspondences per pair; the five-point LMedS estimator needs at least "
                              f"{_lib.LMEDS5_MIN_N}")
    return _lmeds("E", m, K, 5, confidence, max_iters, seed, want_hyp_medians, want_masked)


def lmeds_essential_pose(matches: Tensor, K: Tensor, confidence: float = 0.999, max_iters: int = 1000, seed: int = 0,
                         depth_thres: float = 50.0):
    """ransac_essential_pose with lmeds_essential in place of ransac_essential (the same camera recover_pose_camera(K) for the
    estimate and for the pose).  Returns the lmeds_essential dict with Rt_cam [B,3,4], winner [B], counts [B,4] and in_front [B,N]
    uint8 added."""
    return _essential_pose(lmeds_essential, matches, K, depth_thres, confidence, max_iters, seed)


def ransac_homography(matches: Tensor, n_valid: Optional[Tensor] = None, threshold: float = 3.0, confidence: float = 0.995,
                      max_iters: int = 2000, seed: int = 0, refine: bool = True, all_points: bool = False,
                      want_hyp_counts: bool = False, want_model: bool = False) -> dict:
    """matches [B,N,4] pixels (x1, y1, x2, y2) -> robust homography of every pair by OpenCV 3.4's findHomography(RANSAC) algorithm
    (descriptor_evaluation.py:93, evaluate_frontend.py:234; include/dfepe.h spells out the sampler, the 4-point solve, the error,
    the stopping rule, the refit over the inliers and the Levenberg-Marquardt refinement).  n_valid [B] int32 on the device or
    None: pair b uses its first n_valid[b] rows.  all_points: cv2's method = 0 (least squares over all points, mask all ones);
    refine=False leaves out the refinement.  Returns dict(H [B,3,3] float64 (H22 = 1; zeros without a model), mask [B,N] uint8,
    n_inliers [B], iters_run [B], best_iter [B] (-1 without a sampled winner), hyp_counts [B,max_iters] | None (-1: no model,
    -2: no sample), H_model [B,3,3] float64 | None (the winning sample's H before the refit)).  No host synchronisation;
    capturable.  1 <= N <= 4096."""
    m = _prep(matches, "matches")
    _shape(m, "matches (pixel x1,y1,x2,y2)", None, None, 4)
    B, N = m.shape[0], m.shape[1]
    if N < 1 or N > _lib.HOMOGRAPHY_MAX_N:
        raise _lib.DfepeError(f"ransac_homography: {N} correspondences per pair; the estimator takes 1 .. {_lib.HOMOGRAPHY_MAX_N}")
    L = _lib.lib()
    dev = m.device
    nv = _n_valid_arg(n_valid, B, dev, "ransac_homography")
    flags = (_lib.HOMOGRAPHY_ALL_POINTS if all_points else 0) | (0 if refine else _lib.HOMOGRAPHY_NO_REFINE)
    ws = _workspace(L.dfepe_homography_workspace_bytes(B, N, int(max_iters)), dev)
    out = _estimate_out("H", torch.float64, "best_iter", B, N, dev,
                        [("hyp_counts", (B, int(max_iters)) if want_hyp_counts else None, torch.int32),
                         ("H_model", (B, 3, 3) if want_model else None, torch.float64)])
    with _on(dev):
        rc = L.dfepe_ransac_homography(_ptr(m), _ptr(nv), B, N, float(threshold), float(confidence), int(max_iters), int(seed) & ((1 << 64) - 1),
                                       flags, _ptr(ws), _ptr(out["H"]), _ptr(out["H_model"]), _ptr(out["mask"]), _ptr(out["n_inliers"]),
                                       _ptr(out["iters_run"]), _ptr(out["best_iter"]), _ptr(out["hyp_counts"]), _stream())
    _lib.check(rc, "dfepe_ransac_homography")
    return out


def homography_transfer(H: Tensor, matches: Tensor, n_valid: Optional[Tensor] = None, epi: float = 3.0):
    """H [B,3,3], matches [B,N,4] -> (dist [B,N] fp32 = |H x1 - x2|, mask [B,N] uint8 = dist < epi): evaluate_frontend.getInliers
    (evaluate_frontend.py:210-228) for B pairs, evaluated in fp64.  Rows past n_valid get 0 and 0.  No host synchronisation."""
    m = _prep(matches, "matches")
    _shape(m, "matches (pixel x1,y1,x2,y2)", None, None, 4)
    B, N = m.shape[0], m.shape[1]
    Hd = _h9(H, "H", B)
    dev = m.device
    nv = _n_valid_arg(n_valid, B, dev, "homography_transfer")
    dist = torch.empty(B, N, device=dev)
    mask = torch.empty(B, N, device=dev, dtype=torch.uint8)
    with _on(dev):
        rc = _lib.lib().dfepe_homography_transfer(_ptr(Hd), _ptr(m), _ptr(nv), B, N, float(epi), _ptr(dist), _ptr(mask), _stream())
    _lib.check(rc, "dfepe_homography_transfer")
    return dist, mask


def homography_corners(H_est: Tensor, H_gt: Tensor, height: int, width: int, thresh: Tensor):
    """H_est, H_gt [B,3,3]; thresh [T] on the device -> (mean_dist [B] float64, correct [B,T] uint8): the mean distance of the
    four image corners warped by both homographies and `mean_dist <= thresh` (descriptor_evaluation.compute_homography, lines
    104-123).  An all-zero H_est (no model) gives NaN and 0.  No host synchronisation."""
    _on_gpu(H_est, "H_est")
    B = H_est.shape[0]
    He, Hg = _h9(H_est, "H_est", B), _h9(H_gt, "H_gt", B)
    dev = He.device
    if not torch.is_tensor(thresh) or not thresh.is_cuda or thresh.dim() != 1:
        raise _lib.DfepeError("homography_corners: thresh must be a 1-D tensor on the GPU")
    th = thresh.to(torch.float64).contiguous()
    T = th.shape[0]
    md = torch.empty(B, device=dev, dtype=torch.float64)
    ok = torch.empty(B, T, device=dev, dtype=torch.uint8)
    with _on(dev):
        rc = _lib.lib().dfepe_homography_corners(_ptr(He), _ptr(Hg), B, int(height), int(width), _ptr(th), T, _ptr(md), _ptr(ok), _stream())
    _lib.check(rc, "dfepe_homography_corners")
    return md, ok
