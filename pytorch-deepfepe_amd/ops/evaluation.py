"""Evaluation on the device: odometry and the KITTI table, the validation summary, the detector evaluation and the inlier tables
(csrc/odometry.hip, trajectory.hip, metrics.hip, detector_eval.hip, corr_eval.hip)."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from ._base import Tensor, _h9, _n_valid_arg, _on, _on_gpu, _prep, _ptr, _shape, _stream, _workspace


# ------------------------------------------------------------------------------------------------
# odometry evaluation: pose chain and snippet ATE / RE (deepFEPE/utils/eval_tools.py:252-375)
# ------------------------------------------------------------------------------------------------
def _pose12(t: Tensor, name: str, lead: int) -> Tensor:
    """[..., 3, 4] or [..., 12] with `lead` leading dimensions -> contiguous float64 [..., 12] on the GPU."""
    _on_gpu(t, name)
    t = t.detach().to(torch.float64)
    if t.dim() == lead + 2:
        if tuple(t.shape[-2:]) != (3, 4):
            raise ValueError(f"{name}: poses are 3x4 (or 12 numbers, row-major), got {tuple(t.shape)}")
        t = t.reshape(*t.shape[:-2], 12)
    if t.dim() != lead + 1 or t.shape[-1] != 12:
        raise ValueError(f"{name}: expected {lead} leading dimension(s) and 3x4 poses, got {tuple(t.shape)}")
    return t.contiguous()


def _lengths_arg(lengths, S: int, hi: int, dev, name: str):
    """lengths as a device int32 [S] -- and, when they are host values, checked against [0, hi] here (a device tensor cannot be
    checked without a synchronisation: its range is the caller's contract, and the kernels clamp it to their buffers)."""
    if lengths is None:
        return None
    if isinstance(lengths, Tensor) and lengths.is_cuda:
        _shape(lengths, name, S)
        return lengths.to(torch.int32).contiguous()
    host = [int(v) for v in (lengths.tolist() if isinstance(lengths, Tensor) else lengths)]
    if len(host) != S or any(v < 0 or v > hi for v in host):
        raise ValueError(f"{name} must be {S} values in [0, {hi}], got {host}")
    return torch.tensor(host, dtype=torch.int32, device=dev)


def pose_chain(rel: Tensor, lengths=None, cam2body: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """Relative poses -> trajectory, Exp_table_processor.get_abs_poses for a batch of sequences: rel [S,n,3,4] (or [S,n,12])
    -> abs [S,n+1,3,4] float64 with abs[s,0] the identity and abs[s,k] = inv(P_k ... P_1) (general inverse).  cam2body
    [S,3,4] (one per sequence) or [S,n,3,4] (one per pose): P_k is first taken to body coordinates, inv(C) P_k C
    (relative_pose_cam_to_body).  lengths [S] (host values or a device tensor) for a padded batch: entries past lengths[s]
    are not written (they keep what `out` held; without `out` they are zero).  One launch, no host synchronisation."""
    r = _pose12(rel, "rel", 2)
    S, n = r.shape[0], r.shape[1]
    dev = r.device
    c, stride = None, 0
    if cam2body is not None:
        if cam2body.dim() == 2 or (cam2body.dim() == 3 and cam2body.shape[-1] == 4):  # [S,12] or [S,3,4]: one per sequence
            c = _pose12(cam2body, "cam2body", 1)
            _shape(c, "cam2body", S, 12)
        else:
            c, stride = _pose12(cam2body, "cam2body", 2), 12
            _shape(c, "cam2body", S, n, 12)
    ln = _lengths_arg(lengths, S, n, dev, "lengths")
    if out is None:
        out = torch.zeros(S, n + 1, 12, device=dev, dtype=torch.float64) if ln is not None else \
            torch.empty(S, n + 1, 12, device=dev, dtype=torch.float64)
    elif out.dtype != torch.float64 or not out.is_contiguous() or out.numel() != S * (n + 1) * 12 or out.device != dev:
        raise ValueError("out must be a contiguous float64 tensor of S (n + 1) 12 elements on rel's device")
    with _on(dev):
        rc = _lib.lib().dfepe_pose_chain(_stream(), _ptr(r), _ptr(ln), _ptr(c), stride, S, n, _ptr(out))
    _lib.check(rc, "dfepe_pose_chain")
    return out.view(S, n + 1, 3, 4)


def snippet_errors(est: Tensor, gt: Tensor, seq_length: int = 5, windows=None, compensate: bool = True,
                   want_compensated: bool = False, capacity: Optional[int] = None) -> dict:
    """The snippet ATE / RE of Exp_table_processor.pose_seq_ate for a batch of trajectories: est, gt [S,m,3,4] (or [S,m,12])
    absolute poses; window w of a sequence covers poses w .. w + seq_length - 1.  windows [S] (host values, checked here, or a
    device tensor, the caller's contract: windows[s] + seq_length - 1 <= the sequence's number of poses): how many windows each
    sequence has; default m - seq_length, the reference's count (it never scores the last window).  capacity: rows in the
    outputs (default: the largest host value of windows, or m - seq_length + 1 for a device tensor).
    compensate=False scores the poses as given (a stand-alone compute_pose_error).
    -> dict: errors [S,W,2] float32 (ATE, RE), scale_factors [S,W] float64, aligned_poses [S,W,3,4] float64, stats [S,4] float64
    (ATE mean, ATE std, RE mean, RE std; NaN without windows), with want_compensated also compensated [S,W,L,3,4] (the
    estimate's snippets after compensate_poses).  Rows past windows[s] are zero.  One launch, no host synchronisation."""
    L = int(seq_length)
    if not 1 <= L <= _lib.SNIPPET_MAX_L:
        raise _lib.DfepeError(f"seq_length must be in [1, {_lib.SNIPPET_MAX_L}], got {L}")
    e, g = _pose12(est, "est", 2), _pose12(gt, "gt", 2)
    S, m = e.shape[0], e.shape[1]
    _shape(g, "gt", S, m, 12)
    dev = e.device
    most = max(m - L + 1, 0)
    if windows is None:
        windows = [max(m - L, 0)] * S
    wn = _lengths_arg(windows, S, most, dev, "windows")
    if capacity is None:
        capacity = most if isinstance(windows, Tensor) and windows.is_cuda else max([int(v) for v in windows], default=0)
    W = int(capacity)
    errors = torch.zeros(S, W, 2, device=dev, dtype=torch.float32)
    scale = torch.zeros(S, W, device=dev, dtype=torch.float64)
    aligned = torch.zeros(S, W, 12, device=dev, dtype=torch.float64)
    comp = torch.zeros(S, W, L, 12, device=dev, dtype=torch.float64) if want_compensated else None
    stats = torch.empty(S, 4, device=dev, dtype=torch.float64)
    with _on(dev):
        rc = _lib.lib().dfepe_snippet_errors(_stream(), _ptr(e), _ptr(g), _ptr(wn), S, m, W, L, 0 if compensate else 1,
                                             _ptr(errors), _ptr(scale), _ptr(aligned), _ptr(comp), _ptr(stats))
    _lib.check(rc, "dfepe_snippet_errors")
    out = {"errors": errors, "scale_factors": scale, "aligned_poses": aligned.view(S, W, 3, 4), "stats": stats}
    if want_compensated:
        out["compensated"] = comp.view(S, W, L, 3, 4)
    return out


# ------------------------------------------------------------------------------------------------
# KITTI odometry table: alignment, segment errors, ATE, RPE (the KITTI devkit / kitti-odom-eval evaluation)
# ------------------------------------------------------------------------------------------------
def _traj_args(est: Tensor, gt: Tensor, est_lengths, gt_lengths):
    e, g = _pose12(est, "est", 2), _pose12(gt, "gt", 2)
    S, n = g.shape[0], g.shape[1]
    if e.shape[0] != S or e.shape[1] > n:
        raise ValueError(f"est must have gt's batch and at most its frames, got {tuple(e.shape)} against {tuple(g.shape)}")
    dev = g.device
    m = e.shape[1]
    if m < n:  # the kernels take one n_max: the estimate is padded and its length says so
        e = torch.cat([e, torch.zeros(S, n - m, 12, device=dev, dtype=torch.float64)], dim=1)
        if est_lengths is None:
            est_lengths = torch.full((S,), m, dtype=torch.int32, device=dev)
    return e, g, S, n, _lengths_arg(est_lengths, S, m, dev, "est_lengths"), _lengths_arg(gt_lengths, S, n, dev, "gt_lengths")


def trajectory_align(est: Tensor, gt: Tensor, mode: str = "scale_7dof", est_lengths=None, gt_lengths=None) -> dict:
    """Steps 1 and 2 of the KITTI odometry evaluation for a batch of sequences: est [S,m,3,4], gt [S,n,3,4] (or [..,12]) absolute
    poses, m <= n, frame i of one corresponding to frame i of the other; est_lengths, gt_lengths [S] (host values, checked here,
    or device tensors, clamped by the kernel) for padded batches.  Both trajectories are re-based on their first pose; mode is
    one of _lib.TRAJ_MODES: "none", "scale" (least-squares scale of the translations), "scale_7dof" (Umeyama's scale only),
    "7dof", "6dof" (Umeyama's similarity / rigid transform applied to every pose).
    -> dict: est [S,n,3,4] (aligned; zero past a sequence's m), gt [S,n,3,4] (re-based; zero past its n), r [S,3,3], t [S,3],
    c [S] float64.  One launch, no host synchronisation."""
    if mode not in _lib.TRAJ_MODES:
        raise ValueError(f"mode must be one of {_lib.TRAJ_MODES}, got {mode!r}")
    e, g, S, n, el, gl = _traj_args(est, gt, est_lengths, gt_lengths)
    dev = g.device
    eo = torch.zeros(S, n, 12, device=dev, dtype=torch.float64)
    go = torch.zeros(S, n, 12, device=dev, dtype=torch.float64)
    rtc = torch.empty(S, 13, device=dev, dtype=torch.float64)
    with _on(dev):
        rc = _lib.lib().dfepe_trajectory_align(_stream(), _ptr(e), _ptr(g), _ptr(el), _ptr(gl), S, n, _lib.TRAJ_MODES.index(mode),
                                               _ptr(eo), _ptr(go), _ptr(rtc))
    _lib.check(rc, "dfepe_trajectory_align")
    return {"est": eo.view(S, n, 3, 4), "gt": go.view(S, n, 3, 4), "r": rtc[:, :9].reshape(S, 3, 3), "t": rtc[:, 9:12], "c": rtc[:, 12]}


def kitti_odometry_errors(est: Tensor, gt: Tensor, step: int = 10, est_lengths=None, gt_lengths=None) -> dict:
    """Steps 3 to 5 of the KITTI odometry evaluation on aligned trajectories (trajectory_align's est and gt): est [S,m,3,4],
    gt [S,n,3,4], lengths as there (trajectory_align returns a shorter estimate padded to n frames: its length goes in est_lengths
    here, as compat.eval_tools does).  For every first frame 0, step, 2 step, ... and every length 100 .. 800 m the segment's
    rotation and translation error per metre, then the whole-trajectory ATE and the RPE.
    -> dict: rows [S,F,8,5] float64 with F = ceil(n / step): [first, r_err, t_err, len, speed] (zero where not valid), valid
    [S,F,8] bool, count [S] int32, summary [S,5] float64: t_rel (%), r_rel (deg / 100 m), ATE (m), RPE (m), RPE (deg), and dist
    [S,n] float64, the ground truth's path length.  One launch, no host synchronisation."""
    step = int(step)
    if step < 1:
        raise ValueError(f"step must be at least 1, got {step}")
    e, g, S, n, el, gl = _traj_args(est, gt, est_lengths, gt_lengths)
    dev = g.device
    F = (n + step - 1) // step
    dist = torch.zeros(S, n, device=dev, dtype=torch.float64)
    rows = torch.zeros(S, F, 8, 5, device=dev, dtype=torch.float64)
    valid = torch.zeros(S, F, 8, device=dev, dtype=torch.uint8)
    count = torch.empty(S, device=dev, dtype=torch.int32)
    summary = torch.empty(S, 5, device=dev, dtype=torch.float64)
    with _on(dev):
        rc = _lib.lib().dfepe_kitti_odometry_errors(_stream(), _ptr(e), _ptr(g), _ptr(el), _ptr(gl), S, n, step, F, _ptr(dist),
                                                    _ptr(rows), _ptr(valid), _ptr(count), _ptr(summary))
    _lib.check(rc, "dfepe_kitti_odometry_errors")
    return {"rows": rows, "valid": valid.view(torch.bool), "count": count, "summary": summary, "dist": dist}


# ------------------------------------------------------------------------------------------------
# validation summary reductions ("next" row f-2)
# ------------------------------------------------------------------------------------------------
METRIC_THS = (0.0, 0.01, 0.03, 0.05, 0.1, 0.3, 0.5, 1.0, 2.0, 5.0, 10.0, 90.0, 180.0)


def metrics_summary(epi_est: Tensor, epi_gt: Optional[Tensor], err_q: Tensor, err_t: Tensor) -> dict:
    """Device-side reductions of write_metrics_summary (train_good_utils.py:758-856) for one experiment tag: epi_est / epi_gt
    = epipolar distances of every correspondence (any shape, same numel), err_q / err_t [B] pose errors in degrees.
    Two launches and ONE device-to-host copy of 288 bytes.  Returns python floats: ratio_0.1, ratio_1, F1_0.1, F1_1 (None
    without epi_gt), median / max of err_q and err_t, and ratio_q / ratio_t = cumulative fractions below METRIC_THS[1:].
    The median is np.median of the errors widened to float64: the float64 mean of the two middle float32 order statistics, not
    rounded back to float32.  The maximum is np.amax for any vector with an entry >= 0 or NaN (NaN wins, -0.0 never does).  Empty
    inputs give zeros.  tests/metrics_ref.py restates all of it; tests/test_metrics_edges_gpu.py compares exactly."""
    import numpy as np

    e = _prep(epi_est.reshape(-1), "epi_est")
    g = None if epi_gt is None else _prep(epi_gt.reshape(-1), "epi_gt")
    q, t = _prep(err_q.reshape(-1), "err_q"), _prep(err_t.reshape(-1), "err_t")
    if g is not None and g.numel() != e.numel():
        raise ValueError("epi_gt must have as many entries as epi_est")
    if q.numel() != t.numel():
        raise ValueError("err_q and err_t must have the same length")
    L = _lib.lib()
    nbytes = int(L.dfepe_metrics_summary_bytes())
    out = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=e.device)
    with _on(e.device):
        rc = L.dfepe_metrics_summary(_ptr(e) if e.numel() else None, _ptr(g), e.numel(), _ptr(q), _ptr(t), q.numel(), _ptr(out), _stream())
    _lib.check(rc, "dfepe_metrics_summary")
    raw = out.cpu().numpy().tobytes()[:nbytes]
    counts = np.frombuffer(raw, dtype=np.uint64, count=8).astype(np.float64)
    hist = np.frombuffer(raw, dtype=np.uint64, count=24, offset=64).astype(np.float64).reshape(2, 12)
    mx = np.frombuffer(raw, dtype=np.float32, count=2, offset=64 + 192)
    mids = np.frombuffer(raw, dtype=np.float32, count=4, offset=64 + 192 + 8).reshape(2, 2)
    n, B = max(e.numel(), 1), max(q.numel(), 1)

    def f1(tp, fp, fn):
        return float(2 * tp / (2 * tp + fp + fn)) if (2 * tp + fp + fn) > 0 else 0.0

    res = {"ratio_0.1": float(counts[0] / n), "ratio_1": float(counts[1] / n),
           "F1_0.1": f1(*counts[2:5]) if g is not None else None, "F1_1": f1(*counts[5:8]) if g is not None else None,
           "median_err_q": float(0.5 * (float(mids[0, 0]) + float(mids[0, 1]))), "median_err_t": float(0.5 * (float(mids[1, 0]) + float(mids[1, 1]))),
           "max_err_q": float(mx[0]), "max_err_t": float(mx[1]),
           "ratio_q": (np.cumsum(hist[0]) / B).tolist(), "ratio_t": (np.cumsum(hist[1]) / B).tolist()}
    return res


# ------------------------------------------------------------------------------------------------
# front-end detector evaluation: repeatability, localization error, matching score, nn mean AP
# ------------------------------------------------------------------------------------------------
def _f64(t: Tensor, name: str) -> Tensor:
    _on_gpu(t, name)
    return t.to(torch.float64).contiguous()  # float32 -> float64 is exact


def keypoint_repeatability(kp1: Tensor, kp2: Tensor, H: Tensor, height: int, width: int, keep_k: int, thresh: Tensor,
                           n1: Optional[Tensor] = None, n2: Optional[Tensor] = None) -> dict:
    """kp1 [B,N1,C], kp2 [B,N2,C] rows (x, y[, prob]) of image 1 and image 2, C in {2, 3}; H [B,3,3] image 1 -> image 2; thresh [T]
    on the device -> compute_repeatability (evaluations/detector_evaluation.py:150-279) of every pair at every threshold, in fp64
    (float32 inputs are upcast, which is exact).  n1, n2 [B] int32 on the device or None: pair b uses its first n[b] rows.
    Returns dict(repeatability, loc_err [B,T] float64 (0 and -1 where nothing is counted), count1, count2 [B,T] int32, kept1, kept2
    [B] int32 (the set sizes after the filter and select_k_best), n_unwarped [B] int32 (the matching score's count of image-2
    points whose inverse warp lies in the image, both ends inclusive)).  Equal probabilities at the k-th place: the higher index
    is kept; keep_k = 0 keeps every point (numpy's [-0:]).  The inputs are not written to.  No host synchronisation.
    N1, N2 <= 4096."""
    a, b = _f64(kp1, "kp1"), _f64(kp2, "kp2")
    if a.dim() != 3 or b.dim() != 3 or a.shape[0] != b.shape[0] or a.shape[2] != b.shape[2] or a.shape[2] not in (2, 3):
        raise ValueError(f"keypoints must be [B,N1,C] and [B,N2,C] with C in (2, 3), got {tuple(a.shape)} and {tuple(b.shape)}")
    B, N1, C = a.shape
    N2 = b.shape[1]
    if max(N1, N2) > _lib.DETECTOR_EVAL_MAX_N:
        raise _lib.DfepeError(f"keypoint_repeatability: {max(N1, N2)} keypoints per image; at most {_lib.DETECTOR_EVAL_MAX_N}")
    if int(keep_k) < 0 or int(height) < 1 or int(width) < 1:
        raise ValueError("keypoint_repeatability: keep_k must be >= 0, height and width >= 1")
    Hd = _h9(H, "H", B)
    dev = a.device
    if not torch.is_tensor(thresh) or not thresh.is_cuda or thresh.dim() != 1:
        raise _lib.DfepeError("keypoint_repeatability: thresh must be a 1-D tensor on the GPU")
    th = thresh.to(torch.float64).contiguous()
    T = th.shape[0]
    c1, c2 = _n_valid_arg(n1, B, dev, "keypoint_repeatability"), _n_valid_arg(n2, B, dev, "keypoint_repeatability")
    L = _lib.lib()
    ws = _workspace(L.dfepe_keypoint_repeatability_workspace_bytes(B, N1, N2), dev)
    out = {
        "repeatability": torch.empty(B, T, device=dev, dtype=torch.float64),
        "loc_err": torch.empty(B, T, device=dev, dtype=torch.float64),
        "count1": torch.empty(B, T, device=dev, dtype=torch.int32),
        "count2": torch.empty(B, T, device=dev, dtype=torch.int32),
        "kept1": torch.empty(B, device=dev, dtype=torch.int32),
        "kept2": torch.empty(B, device=dev, dtype=torch.int32),
        "n_unwarped": torch.empty(B, device=dev, dtype=torch.int32),
    }
    with _on(dev):
        rc = L.dfepe_keypoint_repeatability(_ptr(a), _ptr(b), _ptr(c1), _ptr(c2), _ptr(Hd), B, N1, N2, C, int(height), int(width), int(keep_k),
                                            _ptr(th), T, _ptr(ws), _ptr(out["repeatability"]), _ptr(out["loc_err"]), _ptr(out["count1"]),
                                            _ptr(out["count2"]), _ptr(out["kept1"]), _ptr(out["kept2"]), _ptr(out["n_unwarped"]), _stream())
    _lib.check(rc, "dfepe_keypoint_repeatability")
    return out


def average_precision(labels: Tensor, scores: Tensor, n_valid: Optional[Tensor] = None, want_counts: bool = False) -> dict:
    """labels [B,M] (non-zero: positive), scores [B,M] -> sklearn.metrics.average_precision_score of every pair
    (evaluate_frontend.py:244-275) as AP = (1/P) sum over positives of TP(s_i) / CNT(s_i), which groups tied scores as scikit-learn
    does and needs no sort.  n_valid [B] int32 on the device or None.  Returns dict(ap [B] float64 (0 without a valid entry or a
    positive), n_pos [B] int32, tp_at, cnt_at [B,M] int32 | None (want_counts; 0 past n_valid)).  No host synchronisation.
    M <= 4096."""
    sc = _f64(scores, "scores")
    _on_gpu(labels, "labels")
    if sc.dim() != 2 or labels.shape != sc.shape:
        raise ValueError(f"labels and scores must both be [B,M], got {tuple(labels.shape)} and {tuple(sc.shape)}")
    B, M = sc.shape
    if M > _lib.DETECTOR_EVAL_MAX_N:
        raise _lib.DfepeError(f"average_precision: {M} entries per pair; at most {_lib.DETECTOR_EVAL_MAX_N}")
    lb = (labels != 0).to(torch.uint8).contiguous()
    dev = sc.device
    nv = _n_valid_arg(n_valid, B, dev, "average_precision")
    out = {
        "ap": torch.empty(B, device=dev, dtype=torch.float64),
        "n_pos": torch.empty(B, device=dev, dtype=torch.int32),
        "tp_at": torch.empty(B, M, device=dev, dtype=torch.int32) if want_counts else None,
        "cnt_at": torch.empty(B, M, device=dev, dtype=torch.int32) if want_counts else None,
    }
    with _on(dev):
        rc = _lib.lib().dfepe_average_precision(_ptr(lb), _ptr(sc), _ptr(nv), B, M, _ptr(out["ap"]), _ptr(out["n_pos"]), _ptr(out["tp_at"]),
                                                _ptr(out["cnt_at"]), _stream())
    _lib.check(rc, "dfepe_average_precision")
    return out


def matching_score(n_inliers: Tensor, n_kp1: Tensor, n_unwarped: Tensor) -> Tensor:
    """n_inliers, n_kp1, n_unwarped [B] integer tensors on the device -> mscore [B] float64 = 2 n_inliers / (n_kp1 + n_unwarped)
    (evaluate_frontend.py:181); a zero denominator gives what the division gives.  No host synchronisation."""
    args = []
    for t, name in ((n_inliers, "n_inliers"), (n_kp1, "n_kp1"), (n_unwarped, "n_unwarped")):
        _on_gpu(t, name)
        if t.dim() != 1 or t.shape != n_inliers.shape or t.dtype.is_floating_point:
            raise ValueError(f"{name} must be an integer tensor of shape [{n_inliers.shape[0]}], got {t.dtype} {tuple(t.shape)}")
        args.append(t.to(torch.int32).contiguous())
    B = args[0].shape[0]
    dev = args[0].device
    out = torch.empty(B, device=dev, dtype=torch.float64)
    with _on(dev):
        rc = _lib.lib().dfepe_matching_score(_ptr(args[0]), _ptr(args[1]), _ptr(args[2]), B, _ptr(out), _stream())
    _lib.check(rc, "dfepe_matching_score")
    return out


# ------------------------------------------------------------------------------------------------
# correspondence evaluation (evaluation_epiDist.py val_feature, eval_tools.Result_processor): inlier ratios by match score
# ------------------------------------------------------------------------------------------------
INLIER_TABLE_OUTPUTS = ("cnt", "num", "ratio", "dist_out")


def _thds_arg(thds, dev, name: str) -> Tensor:
    """A threshold list as a float64 [T] device tensor: a device tensor is taken as it is; host values are uploaded (inside a
    graph capture pass a device tensor)."""
    if torch.is_tensor(thds):
        if not thds.is_cuda:
            raise _lib.DfepeError(f"{name} must live on the GPU when it is a tensor (this package has no CPU path)")
        t = thds.to(device=dev, dtype=torch.float64).contiguous()
    else:
        t = torch.tensor([float(v) for v in thds], dtype=torch.float64).to(dev)
    if t.dim() != 1 or not 1 <= t.shape[0] <= _lib.INLIER_TABLE_MAX_THDS:
        raise ValueError(f"{name} must hold 1 .. {_lib.INLIER_TABLE_MAX_THDS} thresholds, got shape {tuple(t.shape)}")
    return t


def inlier_table(matches: Optional[Tensor] = None, F: Optional[Tensor] = None, scores: Optional[Tensor] = None,
                 n_valid: Optional[Tensor] = None, inlier_thds=(1.0,), mask_thds=None, want=("cnt", "num", "ratio"),
                 dist: Optional[Tensor] = None) -> dict:
    """matches [B,N,4] pixels (x1, y1, x2, y2) with F [B,3,3], or dist [B,N] (a distance computed before), exactly one of the two;
    scores [B,N] or None (no mask: every match is kept, and mask_thds must be None or hold one value); n_valid [B] int32 on the
    device or None: pair b uses its first clamp(n_valid[b], 0, N) rows; inlier_thds [Ti], mask_thds [Tm] (1 .. 16 each; device
    tensors, or host values that are uploaded) -> dict of the outputs named in ``want``:
      cnt [B,Tm,Ti] int32 = #{score < mask_thd and dist < inlier_thd}, num [B,Tm] int32 = #{score < mask_thd} (num_corrs),
      ratio [B,Tm,Ti] float64 = cnt / num (NaN for a pair with nothing kept), dist_out [B,N] float32 (0 past n_valid)
    Result_processor.inlier_ratio (deepFEPE/utils/eval_tools.py:70-104) over epi_distance_np's dist3 (dsac_tools/utils_F.py:363-385)
    for B pairs, Tm mask thresholds and Ti inlier thresholds in one launch; the distance and both strict comparisons are fp64.
    No host synchronisation; capturable."""
    if (matches is None) == (dist is None):
        raise ValueError("inlier_table takes matches (with F) or dist, exactly one of the two")
    want = tuple(want)
    if not want or any(w not in INLIER_TABLE_OUTPUTS for w in want):
        raise ValueError(f"want must name at least one of {INLIER_TABLE_OUTPUTS}, got {want}")
    if matches is not None:
        m = _prep(matches, "matches")
        _shape(m, "matches (pixel x1,y1,x2,y2)", None, None, 4)
        B, N = m.shape[0], m.shape[1]
        if F is None:
            raise ValueError("inlier_table: matches need F")
        Fd, d, dev = _h9(F, "F", B), None, m.device
    else:
        d = _prep(dist, "dist")
        _shape(d, "dist", None, None)
        B, N = d.shape
        m, Fd, dev = None, None, d.device
    sc = None
    if scores is not None:
        sc = _prep(scores, "scores")
        _shape(sc, "scores", B, N)
    elif mask_thds is not None and len(mask_thds) != 1:
        raise ValueError("inlier_table: without scores nothing is masked; mask_thds must be None or hold one value")
    nv = _n_valid_arg(n_valid, B, dev, "inlier_table")
    it = _thds_arg(inlier_thds, dev, "inlier_thds")
    mt = _thds_arg(mask_thds, dev, "mask_thds") if sc is not None and mask_thds is not None else None
    if sc is not None and mt is None:
        raise ValueError("inlier_table: scores need mask_thds")
    Ti, Tm = it.shape[0], (mt.shape[0] if mt is not None else 1)
    out = {
        "cnt": torch.empty(B, Tm, Ti, device=dev, dtype=torch.int32) if "cnt" in want else None,
        "num": torch.empty(B, Tm, device=dev, dtype=torch.int32) if "num" in want else None,
        "ratio": torch.empty(B, Tm, Ti, device=dev, dtype=torch.float64) if "ratio" in want else None,
        "dist_out": torch.empty(B, N, device=dev, dtype=torch.float32) if "dist_out" in want else None,
    }
    with _on(dev):
        rc = _lib.lib().dfepe_inlier_table(_ptr(m), _ptr(Fd), _ptr(d), _ptr(sc), _ptr(nv), B, N, _ptr(it), Ti, _ptr(mt), Tm, _ptr(out["cnt"]),
                                           _ptr(out["num"]), _ptr(out["ratio"]), _ptr(out["dist_out"]), _stream())
    _lib.check(rc, "dfepe_inlier_table")
    return {k: v for k, v in out.items() if v is not None}


def inlier_table_mean(ratio: Tensor, num: Tensor):
    """ratio [B,Tm,Ti] float64, num [B,Tm] int32 (inlier_table's) -> (mean [Tm,Ti] float64, num_T [Tm,B] int32): the table's mean
    over the pairs, added in index order and NaN-propagating as numpy's table.mean(axis=0) is (eval_tools.py:99-100), and the
    counts in the layout ap_inlier_thd returns.  B == 0 gives a NaN mean.  One launch, no host synchronisation; capturable."""
    for t, name in ((ratio, "ratio"), (num, "num")):
        _on_gpu(t, name)
    _shape(ratio, "ratio", None, None, None)
    B, Tm, Ti = ratio.shape
    _shape(num, "num", B, Tm)
    if not (1 <= Tm <= _lib.INLIER_TABLE_MAX_THDS and 1 <= Ti <= _lib.INLIER_TABLE_MAX_THDS):
        raise ValueError(f"ratio must be [B,Tm,Ti] with 1 .. {_lib.INLIER_TABLE_MAX_THDS} thresholds each, got {tuple(ratio.shape)}")
    r = ratio.to(torch.float64).contiguous()
    n = num.to(torch.int32).contiguous()
    dev = r.device
    mean = torch.empty(Tm, Ti, device=dev, dtype=torch.float64)
    num_T = torch.empty(Tm, B, device=dev, dtype=torch.int32)
    with _on(dev):
        rc = _lib.lib().dfepe_inlier_table_mean(_ptr(r), _ptr(n), B, Tm, Ti, _ptr(mean), _ptr(num_T), _stream())
    _lib.check(rc, "dfepe_inlier_table_mean")
    return mean, num_T
