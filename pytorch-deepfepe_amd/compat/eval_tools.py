"""Mirror of the odometry evaluation of deepFEPE/utils/eval_tools.py (Exp_table_processor: compensate_poses :252-265,
get_abs_poses :268-284, compute_pose_error :309-331, pose_seq_ate :334-375) and of the camera-to-body step in front of it
(relative_pose_cam_to_body, the function nested at Train_model_pipeline.py:1098-1108), backed by dfepe_pose_chain and
dfepe_snippet_errors (include/dfepe.h); and the step the reference leaves to an external tool, the KITTI odometry table
(kitti_odometry_eval, odometry_table, read_kitti_poses, write_kitti_result); and of the correspondence table, Result_processor (eval_tools.py:27-174, at the end of this file), backed by
dfepe_inlier_table and dfepe_inlier_table_mean.

Two surfaces:

  * Exp_table_processor keeps the reference's signatures and return types: numpy in, numpy out (float64, the errors float32, the
    dict keys errors / scale_factors / aligned_poses, `assert len(est) <= len(gt)`, the last window never scored).  The inputs
    go to the current GPU, the kernels run, the results come back -- a drop-in for notebooks/exp_process_table.ipynb.
  * odometry_summary takes val_rt_batch's device Rt_cam and stays on the device: camera-to-body, trajectory, snippet errors and
    their mean / std in two launches, without a host synchronisation, capturable in a hipGraph.

Differences from the reference, all documented where they arise: everything is computed in float64 (the reference compensates a
float32 ground truth in float32 arithmetic because numpy.stack keeps the dtype; here it is widened first); compute_pose_error and
pose_seq_ate take snippets of at most 64 poses (the reference's use is 5); the stand-alone compute_pose_error returns ATE and RE
as float64 scalars that carry float32 precision (the kernel's error array is float32, as pose_seq_ate's is).
"""
from __future__ import annotations

import logging
import os

import numpy as np
import torch

from .. import _lib, ops

Tensor = torch.Tensor


def _dev():
    if not torch.cuda.is_available():
        raise _lib.DfepeError("the odometry evaluation runs on the GPU (this package has no CPU path)")
    return torch.device("cuda", torch.cuda.current_device())


def _to_dev(poses) -> Tensor:
    """numpy / list of [3,4] or [4,4] poses -> float64 [n,3,4] on the current GPU"""
    a = np.stack([np.asarray(p, dtype=np.float64) for p in poses]) if len(poses) else np.zeros((0, 3, 4))
    if a.ndim != 3 or a.shape[1] not in (3, 4) or a.shape[2] != 4:
        raise ValueError(f"poses must be [n,3,4] or [n,4,4], got {a.shape}")
    return torch.from_numpy(np.ascontiguousarray(a[:, :3])).to(_dev())


def relative_pose_cam_to_body(relative_scene_pose, Rt_cam2_gt):
    """transform the camera pose from camera coordinate to body coordinate: inv(Rt_cam2_gt) @ relative_scene_pose @ Rt_cam2_gt
    on 4x4 host matrices, as the reference's nested function (Train_model_pipeline.py:1098-1108).  This per-pair host helper
    is the reference's own expression; on the device the same step is the cam2body argument of ops.pose_chain /
    odometry_summary, where it is folded into the chain kernel."""
    return np.linalg.inv(Rt_cam2_gt) @ relative_scene_pose @ Rt_cam2_gt


class Exp_table_processor:
    """The four odometry methods of the reference's Exp_table_processor (the rest of that class reads and tabulates files)."""

    @staticmethod
    def compensate_poses(poses):
        """poses np[batch, 3, 4] -> np[batch, 3, 4] float64: the first pose's translation subtracted from every translation,
        then every pose multiplied from the left by the inverse of the first pose's 3x3.  Any batch length: longer ones go
        through the kernel 63 poses at a time behind a copy of the first pose."""
        P = _to_dev(poses)
        n, K = P.shape[0], _lib.SNIPPET_MAX_L
        if n == 0:
            raise ValueError("compensate_poses needs at least one pose")
        if n <= K:
            r = ops.snippet_errors(P[None], P[None], seq_length=n, windows=[1], want_compensated=True)
            return r["compensated"][0, 0].cpu().numpy()
        rest = P[1:]
        pad = (-len(rest)) % (K - 1)
        rest = torch.cat([rest, P[:1].expand(pad, 3, 4)]).view(-1, K - 1, 3, 4)
        batch = torch.cat([P[:1].expand(len(rest), 1, 3, 4), rest], dim=1).contiguous()
        c = ops.snippet_errors(batch, batch, seq_length=K, windows=[1] * len(batch), want_compensated=True)["compensated"][:, 0]
        return torch.cat([c[0, :1], c[:, 1:].reshape(-1, 3, 4)])[:n].cpu().numpy()

    @staticmethod
    def get_abs_poses(poses, if_print=False):
        """poses: iterable of 4x4 relative poses -> np[n+1, 3, 4] float64, the identity first, then inv(P_k ... P_1)[:3]."""
        poses = list(poses)
        out = ops.pose_chain(_to_dev(poses)[None])[0].cpu().numpy()
        if if_print:
            for p in out[1:6]:
                print(f"pose abs: {p}")
        return out

    @staticmethod
    def compute_pose_error(gt, pred):
        """gt, pred np[L, 3, 4], L <= 64 -> {"ATE", "RE", "scale_factor"} (numpy float64 scalars), the poses scored as given.
        The parameter names are the reference's; pose_seq_ate passes the ESTIMATE as `gt` and the ground truth as `pred`."""
        a, b = _to_dev(gt), _to_dev(pred)
        if a.shape != b.shape:
            raise ValueError(f"gt and pred must have one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
        L = a.shape[0]
        r = ops.snippet_errors(a[None], b[None], seq_length=L, windows=[1], compensate=False)
        # the kernel's error array is float32 (pose_seq_ate's): ATE and RE are returned as float64 scalars, as the reference's
        # are, but carry float32 precision; the scale factor is the full float64
        e = r["errors"][0, 0].double().cpu().numpy()
        return {"ATE": np.float64(e[0]), "RE": np.float64(e[1]), "scale_factor": np.float64(r["scale_factors"][0, 0].item())}

    @staticmethod
    def pose_seq_ate(est_poses, gt_poses, seq_length=5):
        """compute absolute translation error on small snippets: est_poses np[N, 3, 4], gt_poses np[>= N, 3, 4] ->
        {"errors": np[N - seq_length, 2] float32 (ATE, RE), "scale_factors": list of float64, "aligned_poses": list of np[3, 4]}.
        As in the reference the last window (start N - seq_length) is not scored, and the mean / std are printed."""
        assert len(est_poses) <= len(gt_poses)
        est_length = len(est_poses) - seq_length
        if est_length < 0:
            raise ValueError("negative dimensions are not allowed")  # the reference's numpy.zeros((est_length, 2))
        E = _to_dev(est_poses)
        G = _to_dev(gt_poses[:len(est_poses)])
        r = ops.snippet_errors(E[None], G[None], seq_length=seq_length, windows=[est_length])
        errors = r["errors"][0].cpu().numpy()
        scale = r["scale_factors"][0].cpu().numpy()
        aligned = r["aligned_poses"][0].cpu().numpy()
        with np.errstate(all="ignore"):
            mean_errors, std_errors = (errors.mean(0), errors.std(0)) if len(errors) else (np.full(2, np.nan), np.full(2, np.nan))
        print("")
        print("Results")
        print("\t {:>10}, {:>10}".format("ATE", "RE"))
        print("mean \t {:10.4f}, {:10.4f}".format(*mean_errors))
        print("std \t {:10.4f}, {:10.4f}".format(*std_errors))
        return {"errors": errors, "scale_factors": [s for s in scale], "aligned_poses": [p for p in aligned]}


def _rows3(t: Tensor) -> Tensor:
    return t[..., :3, :] if t.shape[-2] == 4 else t


def odometry_summary(Rt_cam: Tensor, Rt_cam2_gt, gt_poses: Tensor, seq_length: int = 5, lengths=None) -> dict:
    """From val_rt_batch's camera motions to the reported odometry metric, on the device.
      Rt_cam      [n,3,4] (one sequence, val_rt_batch's "Rt_cam") or [S,n,3,4] (a padded batch of sequences)
      Rt_cam2_gt  the samples' camera-to-body transforms, [.., 3 or 4, 4]: one per pose ([n,..] / [S,n,..]) or one per
                  sequence ([..] / [S,..]); None scores the camera motions as they are
      gt_poses    [n+1,3,4] / [S,n+1,3,4] ground-truth absolute poses (any float dtype; widened to float64)
      lengths     [S] relative poses per sequence of a padded batch (host values or a device tensor), default n
    -> dict of device tensors: abs_poses [S,n+1,3,4], errors [S,W,2] float32 with W = n + 1 - seq_length (the reference never
    scores the last window), scale_factors [S,W], aligned_poses [S,W,3,4], ATE_mean, ATE_std, RE_mean, RE_std [S] float64;
    without the leading S for a single sequence.  Rows past a sequence's own windows are zero.  Two launches, no host
    synchronisation (with lengths on the host they are uploaded; inside a graph capture pass a device tensor or None)."""
    single = Rt_cam.dim() == 3
    rel = Rt_cam[None] if single else Rt_cam
    gt = gt_poses[None] if single else gt_poses
    S, n = rel.shape[0], rel.shape[1]
    c = None
    if Rt_cam2_gt is not None:
        c = _rows3(Rt_cam2_gt)
        if single:
            c = c[None]
    abs_poses = ops.pose_chain(rel, lengths=lengths, cam2body=c)
    W = max(n + 1 - seq_length, 0)
    if lengths is None:
        windows = torch.full((S,), W, dtype=torch.int32, device=rel.device)  # filled on the device: no upload, no wait
    elif isinstance(lengths, Tensor) and lengths.is_cuda:
        windows = (lengths.to(torch.int32) + (1 - seq_length)).clamp_(min=0)
    else:
        host = lengths.tolist() if isinstance(lengths, Tensor) else list(lengths)
        windows = [max(int(v) + 1 - seq_length, 0) for v in host]
    r = ops.snippet_errors(abs_poses, gt, seq_length=seq_length, windows=windows, capacity=W)
    st = r["stats"]
    out = {"abs_poses": abs_poses, "errors": r["errors"], "scale_factors": r["scale_factors"], "aligned_poses": r["aligned_poses"],
           "ATE_mean": st[:, 0], "ATE_std": st[:, 1], "RE_mean": st[:, 2], "RE_std": st[:, 3]}
    return {k: v[0] for k, v in out.items()} if single else out


# ---- the KITTI odometry table (README "Evaluate visual odometry", step 3: kitti-odom-eval) ---------------------------------------
# The reference exports the absolute poses and hands them to the kitti-odom-eval tool, whose five numbers per sequence are what it
# publishes (results/*/result.txt).  The functions below are that step on the device: dfepe_trajectory_align and
# dfepe_kitti_odometry_errors (include/dfepe.h) behind ops.trajectory_align / ops.kitti_odometry_errors.
KITTI_RESULT_LINES = ("Trans. err. (%)", "Rot. err. (deg/100m)", "ATE (m)", "RPE (m)", "RPE (deg)")


def _table(est: Tensor, gt: Tensor, alignment: str, step: int, est_lengths, gt_lengths) -> dict:
    if est_lengths is None and est.shape[1] < gt.shape[1]:
        # trajectory_align returns the estimate padded to the ground truth's frames: the second launch must be told its length too
        est_lengths = torch.full((est.shape[0],), est.shape[1], dtype=torch.int32, device=gt.device)
    al = ops.trajectory_align(est, gt, alignment, est_lengths=est_lengths, gt_lengths=gt_lengths)
    r = ops.kitti_odometry_errors(al["est"], al["gt"], step=step, est_lengths=est_lengths, gt_lengths=gt_lengths)
    sm = r["summary"]
    return {"t_rel": sm[:, 0], "r_rel": sm[:, 1], "ATE": sm[:, 2], "RPE_trans": sm[:, 3], "RPE_rot": sm[:, 4], "summary": sm,
            "segments": r["rows"], "valid": r["valid"], "count": r["count"], "dist": r["dist"], "aligned_poses": al["est"],
            "gt_poses": al["gt"], "r": al["r"], "t": al["t"], "scale": al["c"]}


def kitti_odometry_eval(est_abs, gt_abs, alignment: str = "scale_7dof", step: int = 10, lengths=None) -> dict:
    """The kitti-odom-eval numbers of one sequence ([m,3,4] estimate, [n,3,4] ground truth, m <= n) or of a padded batch
    ([S,m,3,4], [S,n,3,4]; lengths = (est_lengths, gt_lengths), each [S] or None), on host arrays or device tensors.
    alignment: "none", "scale", "scale_7dof" (the default, and the mode that reproduces the reference's published numbers),
    "7dof" or "6dof"; step: the distance between first frames of the segments (the devkit's 10).
    -> dict: t_rel (%), r_rel (deg / 100 m), ATE (m), RPE_trans (m), RPE_rot (deg), summary (the five in that order), segments
    [F,8,5] rows [first, r_err, t_err, len, speed], valid [F,8], count, dist, aligned_poses, gt_poses, r, t, scale.  Device tensors
    in give device tensors out, without a host synchronisation; host arrays in give numpy arrays (and python floats / an int for
    the scalars of a single sequence) out."""
    host = not isinstance(est_abs, Tensor)
    est = torch.as_tensor(np.asarray(est_abs, np.float64)).to(_dev()) if host else est_abs
    gt = torch.as_tensor(np.asarray(gt_abs, np.float64)).to(_dev()) if not isinstance(gt_abs, Tensor) else gt_abs
    est, gt = _rows3(est), _rows3(gt)
    single = est.dim() == 3
    if single:
        est, gt = est[None], gt[None]
    el, gl = lengths if lengths is not None else (None, None)
    out = _table(est, gt, alignment, step, el, gl)
    if single:
        out = {k: v[0] for k, v in out.items()}
    if host:
        out = {k: v.cpu().numpy() for k, v in out.items()}
        if single:
            out = {k: (v.item() if v.ndim == 0 else v) for k, v in out.items()}
    return out


def odometry_table(Rt_cam: Tensor, Rt_cam2_gt, gt_poses: Tensor, alignment: str = "scale_7dof", step: int = 10, lengths=None) -> dict:
    """From val_rt_batch's camera motions to the KITTI odometry table, on the device: ops.pose_chain (with the camera-to-body
    conjugation), then the two launches of kitti_odometry_eval.  Rt_cam, Rt_cam2_gt, gt_poses and lengths (relative poses per
    sequence) as in odometry_summary; -> kitti_odometry_eval's dict plus abs_poses, without the leading S for a single sequence.
    Three launches, no host synchronisation (inside a graph capture pass lengths as a device tensor or None)."""
    single = Rt_cam.dim() == 3
    rel = Rt_cam[None] if single else Rt_cam
    gt = _rows3(gt_poses[None] if single else gt_poses)
    c = None
    if Rt_cam2_gt is not None:
        c = _rows3(Rt_cam2_gt)
        if single:
            c = c[None]
    abs_poses = ops.pose_chain(rel, lengths=lengths, cam2body=c)
    frames = None
    if lengths is not None:
        if isinstance(lengths, Tensor) and lengths.is_cuda:
            frames = lengths.to(torch.int32) + 1
        else:
            frames = [int(v) + 1 for v in (lengths.tolist() if isinstance(lengths, Tensor) else lengths)]
    out = _table(abs_poses, gt, alignment, step, frames, frames)
    out["abs_poses"] = abs_poses
    return {k: v[0] for k, v in out.items()} if single else out


def read_kitti_poses(path) -> np.ndarray:
    """A KITTI pose file (one 3x4 pose, 12 numbers, per line) -> np[n,3,4] float64."""
    a = np.loadtxt(path, dtype=np.float64, ndmin=2)
    if a.shape[1] != 12:
        raise ValueError(f"{path}: expected 12 numbers per line, got {a.shape[1]}")
    return a.reshape(-1, 3, 4)


def write_kitti_result(out_dir, seq, result) -> None:
    """Write kitti_odometry_eval's result of one sequence in the layout of the reference's shipped results: <out_dir>/result.txt
    with the five numbers (three decimals) and <out_dir>/errors/<seq>.txt with one row `first_frame r_err t_err len speed` per
    scored segment.  seq: the sequence number or its two-digit name."""
    def val(k):
        return float(result[k].item() if hasattr(result[k], "item") else result[k])

    name = f"{int(seq):02d}"
    rows = result["segments"]
    valid = result["valid"]
    if isinstance(rows, Tensor):
        rows, valid = rows.cpu().numpy(), valid.cpu().numpy()
    rows = np.asarray(rows, np.float64).reshape(-1, 5)[np.asarray(valid, bool).reshape(-1)]
    os.makedirs(os.path.join(out_dir, "errors"), exist_ok=True)
    with open(os.path.join(out_dir, "errors", name + ".txt"), "w") as f:
        for r in rows:
            f.write(f"{int(r[0])} {float(r[1])!r} {float(r[2])!r} {int(r[3])} {float(r[4])!r}\n")
    with open(os.path.join(out_dir, "result.txt"), "w") as f:
        f.write(f"Sequence: \t {int(seq)} \n")
        for label, key in zip(KITTI_RESULT_LINES, ("t_rel", "r_rel", "ATE", "RPE_trans", "RPE_rot")):
            f.write(f"{label}: \t {val(key):.3f} \n")
        f.write("\n")


# ---- the correspondence table (run_eval_good.py --runCorr -> evaluation_epiDist.py val_feature -> Result_processor) ---------------
def _ship(dev, *arrays):
    """Host arrays -> device tensors of the same dtypes and shapes through ONE host-to-device copy: the arrays are laid one after
    the other (each on a 16-byte boundary) in a byte buffer, and the device buffer is cut up again."""
    arrays = [np.ascontiguousarray(a) for a in arrays]
    offs, total = [], 0
    for a in arrays:
        offs.append(total)
        total += (a.nbytes + 15) // 16 * 16
    blob = np.zeros(max(total, 16), np.uint8)
    for a, o in zip(arrays, offs):
        blob[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
    t = torch.from_numpy(blob).to(dev)
    return [t[o:o + a.nbytes].view(getattr(torch, a.dtype.name)).view(a.shape) for a, o in zip(arrays, offs)]


def _chunks(values, size=_lib.INLIER_TABLE_MAX_THDS):
    return [values[i:i + size] for i in range(0, len(values), size)]


def _corr_tables(result_list, thd_list, mask_list, mask_thds):
    """Per-pair host arrays -> (mean [Tm,Ti], num_T [Tm,B], ratio [B,Tm,Ti]) numpy: padded once to [B,Nmax] plus n_valid, shipped
    in one copy, evaluated by ops.inlier_table and ops.inlier_table_mean (one pair of launches per 16 x 16 thresholds)."""
    ests = [np.asarray(re, np.float32).reshape(-1) for re in result_list]
    masks = None
    if mask_list is not None:
        masks = []
        for i, est_arr in enumerate(ests):
            m = np.asarray(mask_list[i], np.float32).reshape(-1)
            assert (
                m.shape[0] == est_arr.shape[0]
            ), "mask size not equal to estimated arr"
            masks.append(m)
    ithds = [float(t) for t in thd_list]
    mthds = [float(t) for t in mask_thds] if masks is not None else [0.0]
    B, Ti, Tm = len(ests), len(ithds), len(mthds)
    if B == 0 or Ti == 0 or Tm == 0:
        return np.full((Tm, Ti), np.nan), np.zeros((Tm, B), np.int64), np.zeros((B, Tm, Ti))
    N = max(len(e) for e in ests)
    dist, sc = np.zeros((B, N), np.float32), np.zeros((B, N), np.float32)
    for b, e in enumerate(ests):
        dist[b, :len(e)] = e
        if masks is not None:
            sc[b, :len(e)] = masks[b]
    nv = np.asarray([len(e) for e in ests], np.int32)
    d_dist, d_sc, d_nv, d_it, d_mt = _ship(_dev(), dist, sc, nv, np.asarray(ithds, np.float64), np.asarray(mthds, np.float64))
    mean, num_T, ratio = np.zeros((Tm, Ti)), np.zeros((Tm, B), np.int64), np.zeros((B, Tm, Ti))
    for m0 in range(0, Tm, _lib.INLIER_TABLE_MAX_THDS):
        m1 = min(m0 + _lib.INLIER_TABLE_MAX_THDS, Tm)
        for t0 in range(0, Ti, _lib.INLIER_TABLE_MAX_THDS):
            t1 = min(t0 + _lib.INLIER_TABLE_MAX_THDS, Ti)
            r = ops.inlier_table(dist=d_dist, scores=d_sc if masks is not None else None, n_valid=d_nv, inlier_thds=d_it[t0:t1],
                                 mask_thds=d_mt[m0:m1] if masks is not None else None, want=("num", "ratio"))
            mn, nT = ops.inlier_table_mean(r["ratio"], r["num"])
            mean[m0:m1, t0:t1], num_T[m0:m1], ratio[:, m0:m1, t0:t1] = mn.cpu().numpy(), nT.cpu().numpy(), r["ratio"].cpu().numpy()
    return mean, num_T, ratio


class Result_processor(object):
    """The reference's Result_processor (deepFEPE/utils/eval_tools.py:27-174) with its constructor, signatures and return types;
    the tables are computed on the device (dfepe_inlier_table, dfepe_inlier_table_mean).  Distances and scores travel as float32,
    which is what ops.inlier_table's dist_out and the matcher's scores are; a float64 list is rounded to float32 first."""

    def __init__(self, result_dict_entry):
        self.result_dict_all = {}
        self.result_dict_entry = result_dict_entry
        self.result_processed = {}
        for ent in result_dict_entry:
            self.result_dict_all[ent] = []

    def add_config(self, config):
        pass

    def load_result(self, result_dict):
        """result_dict: dictionary with entries"""
        for ent in self.result_dict_entry:
            if ent not in result_dict:
                logging.warning(f"{ent} not in the result dictionary")
            else:
                self.result_dict_all[ent].append(result_dict[ent])

    def output_result(self, method=[None], **params):
        for m in method:
            if m is not None:
                func = getattr(self, m)
                func(params[m])

    def inlier_ratio(self, result_list, thd_list, mask_list=None, mask_thd=1, if_print=False):
        """result_list: one nested result of a sequence (per pair, the distances of its matches); mask_list: the scores of the
        results (mscores for correspondences) -> {"inlier_ratio": np[len(thd_list)] = the per-pair ratios' mean, "num_corrs":
        np[pairs]}.  A pair with nothing kept has the ratio 0 / 0 = NaN, and so has the mean, as in the reference.  val_feature
        ends by passing an entry NAME as result_list (evaluation_epiDist.py:243-245), which the reference's loop cannot digest; a
        string is looked up in result_dict_all here."""
        if isinstance(result_list, str):
            result_list = self.result_dict_all[result_list]
        mean, num_T, _ = _corr_tables(result_list, thd_list, mask_list, [mask_thd])
        results = {"inlier_ratio": mean[0], "num_corrs": num_T[0]}
        if if_print:
            print(f"inlier ratio thd: {thd_list}, result: {results}")
        return results

    def get_entry_from_result(self, entry, if_print=False):
        if entry in self.result_dict_all:
            return self.result_dict_all[entry]
        else:
            logging.error(f"{entry} is not in the dictionary.")

    def ap_inlier_thd(self, inlier_entry, inlier_thds, mask_thds, mask_entry="mscores", if_print=False):
        """Unpinned: the reference's method passes a ``mask_entry=`` keyword that its inlier_ratio does not take, so it raises
        there.  This is its evident intent: both entries are looked up in result_dict_all, and the inlier ratios under every mask
        threshold are computed in ONE launch -> {"inlier_thd": np[len(mask_thds), len(inlier_thds)], "num_corrs":
        np[len(mask_thds), pairs]}."""
        result_list = self.result_dict_all[inlier_entry]
        mask_list = None if mask_entry is None else self.result_dict_all[mask_entry]
        table, num_corrs, _ = _corr_tables(result_list, inlier_thds, mask_list, list(mask_thds))
        if mask_list is None:
            table, num_corrs = np.repeat(table, len(mask_thds), 0), np.repeat(num_corrs, len(mask_thds), 0)
        print(f"table: {table.shape}")
        results = {"inlier_thd": table, "num_corrs": num_corrs}
        if if_print:
            print(f"inlier ratio thd: {inlier_thds}, mask thd: {list(mask_thds)}, result: {results}")
        return results

    def save_result(self, filename, item):
        if item == "result_dict_all":
            np.savez_compressed(filename, **self.result_dict_all)

    @staticmethod
    def get_mask(arr, thd):
        return np.array(arr) < thd

    def inlier_ratio_nested(self, est_nested, thd_list):
        """est_nested: per pair, the distances of its matches -> np[len(thd_list)], the mean over the pairs of the inlier ratios"""
        return _corr_tables(est_nested, thd_list, None, None)[0][0]

    @staticmethod
    def inlier_ratio_from_est(est_arr, thd_list):
        """inlier_ratio_from_est(est_arr, thd_list) -> list"""
        return list(_corr_tables([est_arr], thd_list, None, None)[2][0, 0])
