#!/usr/bin/env python3
"""Golden vectors for the adjoint of the textbook eight-point solvers, from the reference itself: _F_from_XY and _E_from_XY of
deepFEPE/dsac_tools/utils_F.py (:223-275, :104-155), with the reference's OWN torch.autograd.grad with respect to X, Y and the weight
vector ws (W = torch.diag(ws)), in float64 and in float32.  The reference is imported at generation time only, utils_F.py with the stub
modules of make_golden.py (cv2 and the superpoint package, which the functions used here never call), as make_golden_dsac.py does.
Only data is written.

    python tests/golden/make_golden_eight_point_adjoint.py <path to the reference checkout>   # rewrites eight_point_adjoint.npz

tests/golden/eight_point_adjoint.npz (described here, not in MANIFEST.txt).  The inputs are eight_point_adjoint_cases.golden_cases():
pair 0 of scene cases with N in {9, 10, 16, 65} (N = 9 is the smallest N at which the reference's some=True SVD still has a ninth
right singular vector), both solvers (_E_from_XY with if_normzliedK=True: the points are K^-1 points already), `normalize` both ways,
W None and torch.diag(ws).  The float32 inputs are widened to float64; the upstream matrix is the case's g.  Per case k:
    k_X, k_Y [N,2], k_g [3,3] float32, k_ws [N] float32 (absent without W)    the inputs, as golden_cases() returns them
    k_out [3,3] float64                     the reference's float64 output (LAPACK's sign: compare after aligning to it)
    k_gX, k_gY [N,2], k_gws [N] float64     torch.autograd.grad(sum(g * out), (X, Y, ws)) in float64
    k_yard_gX, k_yard_gY, k_yard_gws        max |the same gradient from the reference's float32 run, aligned to the float64 sign
                                            - the float64 one|: the yardstick
The run prints the yardsticks and, per case, how far a float64 evaluation that differentiates THROUGH the Hartley transforms (what
compat/_autograd_paths.eight_point does; the reference detaches them, utils_F.py:25,35) is from the reference's gradient, in
yardsticks: the separation that makes the comparison a test of the Hartley rule.  With normalize=False the two are the same function.
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


def evaluate(uF, case, dtype):
    import torch

    X = torch.tensor(case["X"].astype(np.float64), dtype=dtype, requires_grad=True)
    Y = torch.tensor(case["Y"].astype(np.float64), dtype=dtype, requires_grad=True)
    ws = None if case["ws"] is None else torch.tensor(case["ws"].astype(np.float64), dtype=dtype, requires_grad=True)
    W = None if ws is None else torch.diag(ws)
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)  # the reference's torch.tensor([[S1, 0, ...]]) takes the default dtype
    try:
        with contextlib.redirect_stdout(io.StringIO()):  # the reference prints shapes on the way
            if case["essential"]:
                out = uF._E_from_XY(X, Y, None, W=W, if_normzliedK=True, normalize=case["normalize"])
            else:
                out = uF._F_from_XY(X, Y, W=W, normalize=case["normalize"])
    finally:
        torch.set_default_dtype(old)
    assert out.dtype == dtype
    g = torch.tensor(case["g"].astype(np.float64), dtype=dtype)
    grads = torch.autograd.grad((g * out).sum(), (X, Y) if ws is None else (X, Y, ws))
    return out.detach().double().numpy(), [t.detach().double().numpy() for t in grads]


def through_hartley(case):
    """float64 gradients of the same solver with the Hartley transforms differentiated (not the reference's rule)."""
    import torch

    X = torch.tensor(case["X"].astype(np.float64), requires_grad=True)
    Y = torch.tensor(case["Y"].astype(np.float64), requires_grad=True)
    ws = None if case["ws"] is None else torch.tensor(case["ws"].astype(np.float64), requires_grad=True)

    def norm(P):
        c = P.mean(0)
        s = (2.0 ** 0.5) / (P - c).norm(dim=1).mean()
        zero, one = s.new_zeros(()), s.new_ones(())
        T = torch.stack((torch.stack((s, zero, -s * c[0])), torch.stack((zero, s, -s * c[1])), torch.stack((zero, zero, one))))
        return s * (P - c) / (1.0 + 1e-10), T

    p1, T1 = norm(X) if case["normalize"] else (X, None)
    p2, T2 = norm(Y) if case["normalize"] else (Y, None)
    x1, y1, x2, y2 = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    A = torch.stack((x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, torch.ones_like(x1)), 1)
    if ws is not None:
        A = ws[:, None] * A
    f = torch.linalg.svd(A, full_matrices=False)[2][-1]
    U, S, Vh = torch.linalg.svd(f.reshape(3, 3))
    S = S.new_tensor([1.0, 1.0, 0.0]) if case["essential"] else S * S.new_tensor([1.0, 1.0, 0.0])
    out = U @ torch.diag(S) @ Vh
    if case["normalize"]:
        out = T2.t() @ out @ T1
    g = torch.tensor(case["g"].astype(np.float64))
    grads = torch.autograd.grad((g * out).sum(), (X, Y) if ws is None else (X, Y, ws))
    return out.detach().numpy(), [t.detach().numpy() for t in grads]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    import torch

    import eight_point_adjoint_cases as ec

    uF = load_reference(sys.argv[1])
    out = {}
    for k, case in enumerate(ec.golden_cases()):
        o64, g64 = evaluate(uF, case, torch.float64)
        o32, g32 = evaluate(uF, case, torch.float32)
        sg = 1.0 if (o32 * o64).sum() >= 0 else -1.0
        oh, gh = through_hartley(case)
        sh = 1.0 if (oh * o64).sum() >= 0 else -1.0
        for key in ("X", "Y", "g"):
            out[f"{k}_{key}"] = case[key]
        if case["ws"] is not None:
            out[f"{k}_ws"] = case["ws"]
        out[f"{k}_out"] = o64
        line = []
        for name, a64, a32, ah in zip(("gX", "gY", "gws"), g64, g32, gh):
            yard = np.abs(sg * a32 - a64).max()
            out[f"{k}_{name}"] = a64
            out[f"{k}_yard_{name}"] = np.float64(yard)
            line.append(f"{name} yard {yard:.2e} ({yard / np.abs(a64).max():.1e} of max), through-Hartley {np.abs(sh * ah - a64).max() / yard:.1f} yards")
        print(f"case {k}: N {case['N']} {'E' if case['essential'] else 'F'} normalize={case['normalize']} W={'diag' if case['ws'] is not None else 'None'}: "
              + "; ".join(line))
    path = os.path.join(HERE, "eight_point_adjoint.npz")
    np.savez_compressed(path, **out)
    print(f"eight_point_adjoint.npz: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
