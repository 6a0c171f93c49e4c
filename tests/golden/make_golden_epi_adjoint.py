#!/usr/bin/env python3
"""Golden vectors for the adjoints of the epipolar distances, from the reference itself: _sym_epi_dist, _sampson_dist, _epi_distance
and compute_epi_residual of deepFEPE/dsac_tools/utils_F.py (:291-361, :400-413) in float64, with the reference's OWN
torch.autograd.grad with respect to F, X and Y.  The reference is imported at generation time only, utils_F.py with the stub modules
of make_golden.py (cv2 and the superpoint package, which the functions used here never call), as make_golden_corr_eval.py does.
Only data is written.

    python tests/golden/make_golden_epi_adjoint.py <path to the reference checkout>     # rewrites tests/golden/epi_adjoint.npz

tests/golden/epi_adjoint.npz (described here, not in MANIFEST.txt).  The inputs are epi_adjoint_cases.golden_cases(): the "scene"
family, B = 2 pairs of N = 21 points, for every function, if_homo both ways, the clamp on and off; the float32 inputs are widened to
float64, the upstream weight is the case's g.  Per case k (in the order of golden_cases()):
    k_F, k_X, k_Y, k_g float32                the inputs, as golden_cases() returns them (the test checks that they still are)
    k_value float64 [B,N] ([3,B,N] for _epi_distance)      the batched form
    k_gF [B,3,3], k_gX, k_gY [B,N,2|3] float64             torch.autograd.grad(sum(g * value), (F, X, Y))
    k_value2, k_gF2, k_gX2, k_gY2                           the 2-D form on pair 0 (F[0], X[0], Y[0]); not for compute_epi_residual,
                                                            which has no 2-D form
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]


def load_reference(root):
    import make_golden as mg

    mg.REF = root
    mg.install_stubs()
    with contextlib.redirect_stdout(io.StringIO()):
        import deepFEPE.dsac_tools.utils_F as utils_F
    return utils_F


def evaluate(uF, case, single):
    import torch

    sel = (lambda a: a[0]) if single else (lambda a: a)
    F, X, Y = (torch.tensor(sel(case[k]).astype(np.float64), requires_grad=True) for k in ("F", "X", "Y"))
    g = torch.tensor((case["g"][:, 0] if case["kind"] == 2 else case["g"][0]) if single else case["g"], dtype=torch.float64)
    kind, homo, cl = case["kind"], case["homo"], case["clamp_at"]
    if kind == 0:
        v = uF._sym_epi_dist(F, X, Y, if_homo=homo, clamp_at=cl)
    elif kind == 1:
        v = uF._sampson_dist(F, X, Y, if_homo=homo)
    elif kind == 2:
        v = torch.stack(uF._epi_distance(F, X, Y, if_homo=homo))
    else:
        v = uF.compute_epi_residual(X, Y, F, clamp_at=cl)
    assert v.dtype == torch.float64
    gF, gX, gY = torch.autograd.grad((g * v).sum(), (F, X, Y))
    return [t.detach().numpy() for t in (v, gF, gX, gY)]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    import epi_adjoint_cases as ac

    uF = load_reference(sys.argv[1])
    out = {}
    for k, case in enumerate(ac.golden_cases()):
        for key in ("F", "X", "Y", "g"):
            out[f"{k}_{key}"] = case[key]
        for name, val in zip(("value", "gF", "gX", "gY"), evaluate(uF, case, False)):
            out[f"{k}_{name}"] = val
        if case["kind"] != 3:
            for name, val in zip(("value2", "gF2", "gX2", "gY2"), evaluate(uF, case, True)):
                out[f"{k}_{name}"] = val
    path = os.path.join(HERE, "epi_adjoint.npz")
    np.savez_compressed(path, **out)
    print(f"epi_adjoint.npz: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
