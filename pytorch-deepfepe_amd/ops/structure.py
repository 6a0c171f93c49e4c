"""Two-view structure: the optimal correction of matches, triangulation, depths and reprojection (csrc/correct_matches.hip,
triangulate.hip)."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from ._base import Tensor, _on, _on_gpu, _prep, _ptr, _shape, _stream


def correct_matches(F: Tensor, pts1: Tensor, pts2: Tensor, want_cost: bool = False):
    """The optimal correction of correspondences onto an epipolar geometry (Hartley & Sturm), cv2.correctMatches(F, pts1, pts2)
    for a batch: new1, new2 [B,M,2] float32 with new2^T F new1 = 0 and |pts1 - new1|^2 + |pts2 - new2|^2 minimal; with want_cost
    also that minimum [B,M] in px^2.  F [B,3,3], or [3,3] for all pairs, of any float dtype: it is converted to float64, which the
    kernel reads (include/dfepe.h says why).  pts1, pts2 [B,M,2] pixels on the GPU.  A point on an epipole gives NaN, as in cv2.
    One launch, no host synchronisation, no autograd: these are ground-truth data."""
    p, q = _prep(pts1.detach(), "pts1"), _prep(pts2.detach(), "pts2")
    _shape(p, "pts1 (pixel x, y)", None, None, 2)
    B, M = p.shape[0], p.shape[1]
    _shape(q, "pts2", B, M, 2)
    _on_gpu(F, "F")
    Fd = F.detach().to(torch.float64).contiguous()
    if Fd.dim() == 2:
        _shape(Fd, "F", 3, 3)
    else:
        _shape(Fd, "F", B, 3, 3)
    dev = p.device
    new1, new2 = torch.empty(B, M, 2, device=dev), torch.empty(B, M, 2, device=dev)
    cost = torch.empty(B, M, device=dev) if want_cost else None
    with _on(dev):
        rc = _lib.lib().dfepe_correct_matches(_stream(), _ptr(Fd), 0 if Fd.dim() == 2 else 9, _ptr(p), _ptr(q), B, M, _ptr(new1),
                                              _ptr(new2), _ptr(cost))
    _lib.check(rc, "dfepe_correct_matches")
    return (new1, new2, cost) if want_cost else (new1, new2)


# ------------------------------------------------------------------------------------------------
# two-view structure: triangulation, depths, reprojection (csrc/triangulate.hip)
# ------------------------------------------------------------------------------------------------
def _per_pair(t: Tensor, name: str, B: int, *row) -> int:
    """t is [*row] (one matrix for all pairs: stride 0) or [B, *row]; returns the stride in floats."""
    if t.dim() == len(row):
        _shape(t, name, *row)
        return 0
    _shape(t, name, B, *row)
    n = 1
    for d in row:
        n *= d
    return n


def triangulate(P1: Tensor, P2: Tensor, matches: Tensor) -> Tensor:
    """cv2.triangulatePoints for a batch: P1, P2 [3,4] or [B,3,4] projection matrices, matches [B,N,4] pixels (x1, y1, x2, y2)
    -> Xh [B,N,4] float32, per correspondence the unit null vector of the DLT matrix with w = Xh[..., 3] >= 0 (include/dfepe.h:
    fp64 arithmetic, one rounding; a non-finite row gives NaNs).  One launch, no host synchronisation, no autograd."""
    m = _prep(matches.detach(), "matches")
    _shape(m, "matches (pixel x1,y1,x2,y2)", None, None, 4)
    B, N = m.shape[0], m.shape[1]
    P1, P2 = _prep(P1.detach(), "P1"), _prep(P2.detach(), "P2")
    s1, s2 = _per_pair(P1, "P1", B, 3, 4), _per_pair(P2, "P2", B, 3, 4)
    Xh = torch.empty(B, N, 4, device=m.device)
    with _on(m.device):
        rc = _lib.lib().dfepe_triangulate(_ptr(P1), s1, _ptr(P2), s2, _ptr(m), B, N, _ptr(Xh), _stream())
    _lib.check(rc, "dfepe_triangulate")
    return Xh


def two_view_structure(Rt: Tensor, K: Tensor, matches: Tensor, camera_motion: bool = True, winner: Optional[Tensor] = None,
                       scale: Optional[Tensor] = None, clamp: Optional[float] = None, want=("X", "z1", "z2")) -> dict:
    """The 3-D points of a pose's correspondences and their depths in both cameras (the reference's get_depth after
    cv2.recoverPose): Rt [B,3,4] (camera motion as cheirality() returns it, or scene motion with camera_motion=False), K [B,3,3],
    matches [B,N,4] pixels -> dict of the entries named in ``want``: X [B,N,3] in the frame of camera 1, z1, z2 [B,N].
    ``winner`` [B] int32 (cheirality's): a pair with winner < 0 gets NaN rows.  ``scale`` [B] multiplies X, z1 and z2
    (t_scene_scale); ``clamp`` > 0 clamps the scaled depths to [-clamp, clamp].  One launch, no host synchronisation."""
    m = _prep(matches.detach(), "matches")
    _shape(m, "matches (pixel x1,y1,x2,y2)", None, None, 4)
    B, N = m.shape[0], m.shape[1]
    Rt, K = _prep(Rt.detach(), "Rt"), _prep(K.detach(), "K")
    _shape(Rt, "Rt", B, 3, 4)
    _shape(K, "K (one intrinsic matrix per pair)", B, 3, 3)
    want = tuple(want)
    if not want or any(w not in ("X", "z1", "z2") for w in want):
        raise ValueError(f"want must name at least one of X, z1, z2, got {want}")
    if winner is not None and (winner.shape != (B,) or winner.dtype != torch.int32 or not winner.is_contiguous() or not winner.is_cuda):
        raise ValueError("winner must be the contiguous [B] int32 output of cheirality")
    if scale is not None:
        scale = _prep(scale.detach(), "scale").reshape(-1)
        _shape(scale, "scale", B)
    dev = m.device
    out = {k: torch.empty((B, N, 3) if k == "X" else (B, N), device=dev) for k in want}
    with _on(dev):
        rc = _lib.lib().dfepe_two_view_structure(_ptr(Rt), _lib.POSE_CAMERA_MOTION if camera_motion else 0, _ptr(K), _ptr(m), B, N,
                                                 _ptr(winner), _ptr(scale), float(clamp) if clamp else 0.0, _ptr(out.get("X")),
                                                 _ptr(out.get("z1")), _ptr(out.get("z2")), _stream())
    _lib.check(rc, "dfepe_two_view_structure")
    return out


def reproject(X: Tensor, Rt: Tensor, K: Tensor, image_w: float, image_h: float, camera_motion: bool = False) -> dict:
    """Project points into an image (utils_vis.reproj_and_scatter without the drawing): X [B,M,3], Rt [3,4] or [B,3,4] (scene
    motion, or camera motion with camera_motion=True), K [3,3] or [B,3,3] -> dict(x [B,M,2] pixels, z [B,M] depth, inside [B,M]
    uint8 = utils_misc.within(x, y, image_w, image_h) of the float32 x; no depth test).  One launch, no host synchronisation."""
    X = _prep(X.detach(), "X")
    _shape(X, "X", None, None, 3)
    B, M = X.shape[0], X.shape[1]
    Rt, K = _prep(Rt.detach(), "Rt"), _prep(K.detach(), "K")
    sr, sk = _per_pair(Rt, "Rt", B, 3, 4), _per_pair(K, "K", B, 3, 3)
    dev = X.device
    out = {"x": torch.empty(B, M, 2, device=dev), "z": torch.empty(B, M, device=dev), "inside": torch.empty(B, M, device=dev, dtype=torch.uint8)}
    with _on(dev):
        rc = _lib.lib().dfepe_reproject(_ptr(X), _ptr(Rt), sr, _lib.POSE_CAMERA_MOTION if camera_motion else 0, _ptr(K), sk, B, M,
                                        float(image_w), float(image_h), _ptr(out["x"]), _ptr(out["z"]), _ptr(out["inside"]), _stream())
    _lib.check(rc, "dfepe_reproject")
    return out
