"""Mirror of deepFEPE/dsac_tools/utils_vis.py, its numeric part only: reproj_and_scatter (utils_vis.py:150-169), which the loaders
use to turn lidar points into ground-truth correspondences (datasets/kitti_odo_corr.py:577-586, kitti_tools/utils_kitti.py:249-279).
The projection and the in-image test run in one launch of libdfepe_hip.so (ops.reproject); the drawing functions of the
reference module need matplotlib and cv2 and are not mirrored."""
import numpy as np
import torch

from .. import ops


def reproj_and_scatter(Rt, X_rect, im_rgb, kitti_two_frame_loader=None, visualize=True, title_appendix='', param_list=[],
                       set_lim=False, debug=True, s=10):
    """Same call and return as the reference, numpy in and out: project X_rect [N,3] with K [Rt] and return
    (val_inds [N] bool: utils_misc.within(x, y, im_shape[1], im_shape[0]) of the projected points -- no depth test --, x1 [N,2]).
    K and im_shape come from ``param_list`` = [K, im_shape], or from the loader's attributes when ``kitti_two_frame_loader`` is
    given.  x1 holds the kernel's float32 values (fp64 arithmetic, one rounding; include/dfepe.h, dfepe_reproject), widened to
    float64.  ``im_rgb``, ``title_appendix``, ``set_lim`` and ``s`` only concern the drawing and are unused;
    ``visualize=True`` -- the reference's default -- needs matplotlib and raises NotImplementedError: pass visualize=False."""
    if visualize:
        raise NotImplementedError("reproj_and_scatter(visualize=True): drawing the points needs matplotlib, which is not used here")
    if kitti_two_frame_loader is None:
        if debug:
            print('Reading from input list of param_list=[K, im_shape].')
        K = param_list[0]
        im_shape = param_list[1]
    else:
        K = kitti_two_frame_loader.K
        im_shape = kitti_two_frame_loader.im_shape
    X = np.asarray(X_rect)
    if X.shape[0] == 0:
        return np.zeros(0, dtype=bool), np.zeros((0, 2))
    dev = torch.device("cuda")
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)
    out = ops.reproject(t(X[:, :3]).unsqueeze(0), t(np.asarray(Rt)[:3, :4]), t(np.asarray(K)[:3, :3]), float(im_shape[1]), float(im_shape[0]))
    return out["inside"][0].cpu().numpy() > 0, out["x"][0].cpu().double().numpy()
