"""Mirror of deepFEPE/dsac_tools/H_loss.py: HLoss, the mean Sampson distance of a hypothesis."""
import torch

from . import utils_F


class HLoss:
    """loss = HLoss()(H, X, Y): torch.mean(_sampson_dist(H, X, Y, if_homo=False)) (H_loss.py:18-29), H [3,3] with X, Y [N,2] or
    batched; differentiable in H, X and Y through the kernel's adjoint."""

    def __init__(self):
        pass

    def __call__(self, H, X, Y):
        errors = utils_F._sampson_dist(H, X, Y, if_homo=False)
        return torch.mean(errors)
