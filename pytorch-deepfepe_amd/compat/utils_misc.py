"""Mirror of the helpers of deepFEPE/dsac_tools/utils_misc.py that the hot path and its callers use: homogeneous-coordinate
helpers, the cross-product matrix, rigid-transform inversion / padding and the crop-or-pad index draw.  These are tiny
host-side or elementwise operations (no kernel needed); signatures and numerics follow the reference.  The virtual-point
generator at the end (get_virt_x1x2_grid / _np / get_virt_x1x2, and get_virt_x1x2_batch for a whole batch on the device) is the
exception: its cv2.correctMatches is ops.correct_matches, one launch of a HIP kernel."""
import numpy as np
import torch

from .. import ops


def within(x, y, xlim, ylim):
    """Which points lie inside [0, xlim] x [0, ylim], borders included (utils_misc.py:12-15); numpy, NaN is outside."""
    val_inds = (x >= 0) & (y >= 0)
    val_inds = val_inds & (x <= xlim) & (y <= ylim)
    return val_inds


def identity_Rt(dtype=np.float32):
    """[I | 0] as a 3x4 numpy array (utils_misc.py:17-18)."""
    return np.hstack((np.eye(3, dtype=dtype), np.zeros((3, 1), dtype=dtype)))


def _skew_symmetric(v):
    """[v]_x for v [3,1] -> [3,3], or [B,3,1] -> [B,3,3] (utils_misc.py:20-37)."""
    if v.dim() == 2:
        x, y, z = v[0, 0], v[1, 0], v[2, 0]
        o = torch.zeros_like(x)
        return torch.stack((o, -z, y, z, o, -x, -y, x, o)).view(3, 3)
    x, y, z = v[:, 0, 0], v[:, 1, 0], v[:, 2, 0]
    o = torch.zeros_like(x)
    return torch.stack((o, -z, y, z, o, -x, -y, x, o), dim=1).view(-1, 3, 3)


def skew_symmetric_np(v):
    """numpy twin of _skew_symmetric (utils_misc.py:39-56)."""
    v = np.asarray(v)
    if v.ndim == 2:
        x, y, z = v[0, 0], v[1, 0], v[2, 0]
        o = np.zeros_like(x)
        return np.stack((o, -z, y, z, o, -x, -y, x, o)).reshape(3, 3)
    x, y, z = v[:, 0, 0], v[:, 1, 0], v[:, 2, 0]
    o = np.zeros_like(x)
    return np.stack((o, -z, y, z, o, -x, -y, x, o), axis=1).reshape(-1, 3, 3)


def _homo(x):
    """Append a column of ones: [N,2] -> [N,3] or [B,N,2] -> [B,N,3] (utils_misc.py:58-69).  The reference prints the
    tensor's size, dtype and device on every call (:60); that debugging output is not reproduced."""
    assert x.dim() in (2, 3)
    return torch.cat((x, torch.ones(*x.shape[:-1], 1, dtype=x.dtype, device=x.device)), x.dim() - 1)


def _de_homo(x_homo):
    """Divide by the last coordinate + 1e-10 and drop it (utils_misc.py:71-80)."""
    assert x_homo.dim() in (2, 3)
    return x_homo[..., :-1] / (x_homo[..., -1] + 1e-10).unsqueeze(-1)


def homo_np(x):
    """[N,D] -> [N,D+1] (utils_misc.py:82-87)."""
    return np.hstack((x, np.ones((x.shape[0], 1), dtype=x.dtype)))


def de_homo_np(x_homo):
    """[N,D] -> [N,D-1], D in {3,4} (utils_misc.py:89-96)."""
    assert x_homo.shape[1] in (3, 4)
    return x_homo[:, :-1] / np.expand_dims(x_homo[:, -1] + 1e-10, -1)


def Rt_pad(Rt):
    """3x4 [R|t] -> 4x4 [[R|t],[0,0,0,1]] (utils_misc.py:98-101)."""
    assert Rt.shape == (3, 4)
    return np.vstack((Rt, np.array([[0.0, 0.0, 0.0, 1.0]], dtype=Rt.dtype)))


def Rt_depad(Rt01):
    """4x4 -> 3x4 (utils_misc.py:123-126)."""
    assert Rt01.shape == (4, 4)
    return Rt01[:3, :]


def inv_Rt_np(Rt):
    """[R|t]^-1 = [R^T | -R^T t], numpy (utils_misc.py:109-115)."""
    assert Rt.shape == (3, 4)
    R, t = Rt[:, :3], Rt[:, 3:4]
    return np.hstack((R.T, -R.T @ t))


def _inv_Rt(Rt):
    """[R|t]^-1 = [R^T | -R^T t] for a 3x4 tensor (utils_misc.py:117-123); differentiable."""
    assert tuple(Rt.shape) == (3, 4)
    R, t = Rt[:, :3], Rt[:, 3:4]
    return torch.cat((R.t(), -R.t() @ t), 1)


def crop_or_pad_choice(in_num_points, out_num_points, shuffle=False):
    """Indices that crop or pad ``in_num_points`` items to ``out_num_points`` (utils_misc.py:139-161).  Host-side and
    drawn from numpy's global RNG with the reference's call sequence (one permutation when shuffling, one
    ``np.random.choice`` when padding), so a seeded run selects the same correspondences as the reference."""
    choice = np.random.permutation(in_num_points) if shuffle else np.arange(in_num_points)
    assert out_num_points > 0, "out_num_points = %d must be positive int!" % out_num_points
    if in_num_points >= out_num_points:
        return choice[:out_num_points]
    pad = np.random.choice(choice, out_num_points - in_num_points, replace=True)
    return np.concatenate([choice, pad])


def get_virt_x1x2_grid(im_shape):
    """The 10 x 10 grid of pixel positions, the same in both images, as float32 [100,2] (utils_misc.py:163-171, line for line)."""
    step = 0.1
    sz1 = im_shape
    sz2 = im_shape
    xx, yy = np.meshgrid(np.arange(0, 1, step), np.arange(0, 1, step))
    pts1_virt_b = np.float32(np.vstack((sz1[1] * xx.flatten(), sz1[0] * yy.flatten())).T)
    pts2_virt_b = np.float32(np.vstack((sz2[1] * xx.flatten(), sz2[0] * yy.flatten())).T)
    return pts1_virt_b, pts2_virt_b


def _correct_matches_np(F_gt, first, second):
    """cv2.correctMatches(F_gt, first[None], second[None]) for numpy input: one launch on the current GPU, float32 [1,M,2] back."""
    dev = torch.device("cuda")
    F = torch.as_tensor(np.asarray(F_gt, dtype=np.float64), device=dev)
    a = torch.as_tensor(np.ascontiguousarray(first, dtype=np.float32), device=dev).unsqueeze(0)
    b = torch.as_tensor(np.ascontiguousarray(second, dtype=np.float32), device=dev).unsqueeze(0)
    new_a, new_b = ops.correct_matches(F, a, b)
    return new_a.cpu().numpy(), new_b.cpu().numpy()


def get_virt_x1x2_np(im_shape, F_gt, K, pts1_virt_b, pts2_virt_b):
    """The virtual correspondences of the F-loss: the given points moved onto the geometry F_gt by the optimal correction
    (utils_misc.py:173-199).  Returns numpy (pts1_virt_normalized, pts2_virt_normalized) float64 [M,3] and (pts1_virt,
    pts2_virt) float32 [M,3], homogeneous.  Two quirks of the reference are kept:
      - the call is correctMatches(F_gt, pts2_virt_b, pts1_virt_b) and its first output becomes pts1_virt (:176): the corrected
        points do satisfy pts2_virt^T F_gt pts1_virt = 0, but each started from the other image's input (harmless while the
        two grids are equal);
      - pts2_virt_normalized is computed from pts1_virt, not pts2_virt (:198).
    A point on an epipole comes back NaN from the correction and is set to 0 (:177-178)."""
    pts1_virt, pts2_virt = _correct_matches_np(F_gt, pts2_virt_b, pts1_virt_b)
    pts1_virt[np.isnan(pts1_virt)] = 0.
    pts2_virt[np.isnan(pts2_virt)] = 0.
    pts1_virt = homo_np(pts1_virt[0])
    pts2_virt = homo_np(pts2_virt[0])
    pts1_virt_normalized = (np.linalg.inv(K) @ pts1_virt.T).T
    pts2_virt_normalized = (np.linalg.inv(K) @ pts1_virt.T).T  # sic: from pts1_virt (:198)
    return pts1_virt_normalized, pts2_virt_normalized, pts1_virt, pts2_virt


def get_virt_x1x2(im_shape, F_gt, K, pts1_virt_b=None, pts2_virt_b=None):
    """get_virt_x1x2_np with the grid of im_shape as the default points and float32 CPU tensors returned, as the reference's
    loader stores them (utils_misc.py:201-230; same two quirks, :206 and :228)."""
    if pts1_virt_b is None and pts2_virt_b is None:
        pts1_virt_b, pts2_virt_b = get_virt_x1x2_grid(im_shape)
    pts1_virt_normalized, pts2_virt_normalized, pts1_virt, pts2_virt = get_virt_x1x2_np(im_shape, F_gt, K, pts1_virt_b, pts2_virt_b)
    return torch.from_numpy(pts1_virt_normalized).float(), torch.from_numpy(pts2_virt_normalized).float(), \
        torch.from_numpy(pts1_virt).float(), torch.from_numpy(pts2_virt).float()


_virt_grids = {}  # (device, im_shape) -> the grid [100,2] on that device


def get_virt_x1x2_batch(im_shape, F_gts, Ks):
    """get_virt_x1x2 for a batch that is already on the device: F_gts, Ks [B,3,3] -> (pts1_virt_normalized,
    pts2_virt_normalized, pts1_virt, pts2_virt), each [B,100,3] float32 on F_gts' device -- what a training step feeds
    get_all_loss_DeepF as pts*_virt_normalized / pts*_virt_ori instead of carrying them through the loader.  One launch for the
    batch, the grid cached per (device, im_shape), no host synchronisation.  F_gts is used in float64 if it is given so (the
    correction reads F in fp64); inv(K) @ x is computed in float64 like the reference's numpy, then rounded.  Both quirks of
    get_virt_x1x2_np are kept."""
    dev = F_gts.device
    key = (dev, tuple(int(v) for v in im_shape[:2]))
    grid = _virt_grids.get(key)
    if grid is None:
        grid = _virt_grids[key] = torch.as_tensor(get_virt_x1x2_grid(im_shape)[0], device=dev)
    B = F_gts.shape[0]
    pts_b = grid.unsqueeze(0).expand(B, -1, -1)
    pts1_virt, pts2_virt = ops.correct_matches(F_gts, pts_b, pts_b)  # correctMatches(F_gt, pts2_virt_b, pts1_virt_b): equal grids
    pts1_virt = _homo(torch.where(torch.isnan(pts1_virt), torch.zeros_like(pts1_virt), pts1_virt))
    pts2_virt = _homo(torch.where(torch.isnan(pts2_virt), torch.zeros_like(pts2_virt), pts2_virt))
    # inv(K) by cofactors in float64: row i of the inverse is the cross product of the two other columns over the determinant
    K = Ks.to(torch.float64)
    c0, c1, c2 = K[:, :, 0], K[:, :, 1], K[:, :, 2]
    r0 = torch.linalg.cross(c1, c2)
    K_inv = torch.stack((r0, torch.linalg.cross(c2, c0), torch.linalg.cross(c0, c1)), 1) / (c0 * r0).sum(1)[:, None, None]
    pts1_virt_normalized = (pts1_virt.double() @ K_inv.transpose(1, 2)).float()
    pts2_virt_normalized = pts1_virt_normalized.clone()  # sic: from pts1_virt (:228)
    return pts1_virt_normalized, pts2_virt_normalized, pts1_virt, pts2_virt
