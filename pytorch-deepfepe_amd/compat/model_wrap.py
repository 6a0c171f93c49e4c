"""Drop-in for the one class the hot path's callers take from the un-vendored ``superpoint`` package
(``superpoint.models.model_wrap.PointTracker``; deepFEPE/train_good.py:74,222, utils/eval_tools.py:664-672): the matcher,
which is all get_matches_from_SP calls on it, and the two-frame state (update, get_matches, get_mscores, clear_desc) that
evaluation_epiDist.py's val_feature drives."""
import numpy as np
import torch

from .. import _lib, ops


class PointTracker(object):
    def __init__(self, max_length=2, nn_thresh=0.7):
        if max_length < 2:
            raise ValueError("max_length must be greater than or equal to 2.")
        self.maxl = max_length
        self.nn_thresh = nn_thresh
        self.last_desc = None
        self.last_pts = None
        self.matches = np.zeros((4, 0))
        self.mscores = np.zeros((0,))

    # ---- the two-frame state val_feature uses (evaluation_epiDist.py:151-221).  The superpoint package is not part of the
    # reference's tree, so these four follow the published tracker and are unpinned; this text is their specification.
    def update(self, pts, desc):
        """Add a frame: pts [3,n] (x, y, confidence; numpy), desc [D,n] unit-norm columns.  The matches of the previous frame to
        this one (mutual nearest neighbours closer than nn_thresh, in increasing index of the previous frame's points) are kept for
        get_matches / get_mscores; the frame becomes the previous one.  Only the two-frame tracker (max_length = 2) is built:
        longer tracks raise.  The matching runs on the GPU (dfepe_nn_match_two_way); the descriptors of the previous frame stay
        there."""
        if self.maxl != 2:
            raise ValueError("only the two-frame tracker (max_length = 2) is built; longer tracks are not")
        if pts is None or desc is None:
            print("PointTracker: Warning, no points were added to tracker.")
            return
        pts = np.asarray(pts)
        assert pts.shape[1] == desc.shape[1]
        d = torch.as_tensor(desc)
        if not torch.cuda.is_available():
            raise _lib.DfepeError("PointTracker.update needs a GPU (no CPU implementation)")
        d = d.to(torch.device("cuda", torch.cuda.current_device()) if not d.is_cuda else d.device, torch.float32)
        self.matches, self.mscores = np.zeros((4, 0)), np.zeros((0,))
        if self.last_desc is not None and self.last_pts is not None:
            m = self.nn_match_two_way(self.last_desc, d, self.nn_thresh)
            self.matches = np.concatenate([self.last_pts[:, m[0].astype(int)], pts[:2, m[1].astype(int)]], axis=0)
            self.mscores = m[2]
        self.last_desc = d
        self.last_pts = pts[:2].copy()

    def get_matches(self):
        """[4,n] = (x1, y1, x2, y2) of the last two frames' matches (the frames' own coordinates, untouched); [4,0] before the
        second frame."""
        return self.matches

    def get_mscores(self):
        """[n]: the matches' descriptor distances, in get_matches' order."""
        return self.mscores

    def clear_desc(self):
        """Forget the previous frame's descriptors: the next frame starts a new pair."""
        self.last_desc = None

    def nn_match_two_way(self, desc1, desc2, nn_thresh):
        """desc1 [D,N1], desc2 [D,N2] (numpy or torch, unit-norm columns) -> numpy float64 [3,n]: index in 1, index in 2,
        L2 distance of every mutual nearest-neighbour pair closer than ``nn_thresh``.  The matrices are staged on the GPU
        (the reference hands this method host arrays, train_good_utils.py:687-691); batches should call
        ``compat.train_good_utils.get_matches_from_SP`` / ``ops.nn_match_two_way`` instead, which never leave the device."""
        d1, d2 = torch.as_tensor(desc1), torch.as_tensor(desc2)
        assert d1.shape[0] == d2.shape[0]
        if d1.shape[1] == 0 or d2.shape[1] == 0:
            return np.zeros((3, 0))
        if nn_thresh < 0.0:
            raise ValueError("'nn_thresh' should be non-negative")
        if not torch.cuda.is_available():
            raise _lib.DfepeError("PointTracker.nn_match_two_way needs a GPU (no CPU implementation)")
        dev = d1.device if d1.is_cuda else torch.device("cuda", torch.cuda.current_device())
        a = d1.to(dev, torch.float32).t().contiguous().unsqueeze(0)
        b = d2.to(dev, torch.float32).t().contiguous().unsqueeze(0)
        m1, m2, sc, cnt = ops.nn_match_two_way(a, b, float(nn_thresh))
        n = int(cnt[0].item())
        out = np.zeros((3, n))
        out[0] = m1[0, :n].cpu().numpy()
        out[1] = m2[0, :n].cpu().numpy()
        out[2] = sc[0, :n].cpu().numpy()
        return out
