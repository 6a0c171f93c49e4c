#!/usr/bin/env python3
"""Golden vectors for the DSAC hypothesis loop, from the reference itself: class DSAC of deepFEPE/dsac_tools/dsac.py with HLoss of
dsac_tools/H_loss.py, run in the reference's own float32 on the CPU.  The reference is imported at generation time only, with the stub
modules of make_golden.py (cv2 and the superpoint package, which nothing used here calls), as make_golden_epi_adjoint.py does.  Two
repairs are needed before the class runs at all, neither touching its arithmetic: `utils_F.E_to_F`, which dsac.py:67 calls and the
reference's tree does not define, is aliased to `utils_F._E_to_F`, the function it means; and H_gt, on which __call__ calls .cpu() (:113)
and which it never uses, is a zero matrix, not None.  Only data is written.

    python tests/golden/make_golden_dsac.py <path to the reference checkout>     # rewrites tests/golden/dsac.npz

tests/golden/dsac.npz (described here, not in MANIFEST.txt).  The inputs are dsac_cases.golden_cases(): the "scene" family, N <= 65,
hyps <= 16, thresh = 100, beta = 0.02, Python's `random` seeded per case.  Per case k:
    k_X, k_Y [N,2], k_K [3,3] float32         the inputs, as golden_cases() returns them (the test checks that they still are)
    k_seed, k_hyps                            random.seed(k_seed) comes right before the call
    k_idx [hyps,10] int32                     the sampled correspondences, recovered by replaying the seed
    k_inlier_scores, k_sampson_dists [hyps,N], k_quality [N,1] float32, k_best_H_idx, k_max_score     what the reference's run set / returned
    k_f64_<name>                              tests/dsac_ref.py's float64 values of the same quantities (stage by stage, each on the
                                              previous stage's float64 values)
    k_yard_<name>                             max |reference float32 - float64| of that quantity: the yardstick
"""
import contextlib
import io
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]


def load_reference(root):
    import make_golden as mg

    mg.REF = root
    mg.install_stubs()
    with contextlib.redirect_stdout(io.StringIO()):
        import dsac_tools.dsac as dsac
        import dsac_tools.H_loss as H_loss
        import dsac_tools.utils_F as utils_F
    utils_F.E_to_F = utils_F._E_to_F
    return dsac, H_loss


def float64_run(case, idx):
    import dsac_ref as dr

    X, Y, K = case["X"][None], case["Y"][None], case["K"][None]
    E, _ = dr.stage1(X, Y, K, idx[None])
    s2 = dr.stage2(E, X, Y, K, case["thresh"], case["beta"])
    score = s2["score"][0]
    ns, nc = np.zeros(case["N"]), np.zeros(case["N"])
    for h in range(len(idx)):
        ns[idx[h]] += score[h]
        nc[idx[h]] += 1.0
    return {"inlier_scores": s2["soft"][0], "sampson_dists": s2["sampson"][0], "quality": (ns / (nc + 1e-10))[:, None],
            "max_score": np.float64(score.max()), "best_H_idx": np.int64(dr.first_best(score)), "hyp_scores": score}


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    import torch

    import dsac_cases as dc

    dsac, H_loss = load_reference(sys.argv[1])
    out = {}
    for k, case in enumerate(dc.golden_cases()):
        N, hyps, seed = case["N"], case["hyps"], case["seed"]
        random.seed(seed)
        idx = np.array([random.sample(range(N), 10) for _ in range(hyps)], np.int32)
        d = dsac.DSAC(hyps, case["thresh"], case["beta"], case["alpha"], torch.from_numpy(case["K"]), H_loss.HLoss())
        random.seed(seed)
        with contextlib.redirect_stdout(io.StringIO()):
            quality = d(torch.from_numpy(case["X"]), torch.from_numpy(case["Y"]), torch.zeros(3, 3))
        assert quality.dtype == torch.float32 and d.best_corres_idx == idx[d.best_H_idx].tolist()
        ref = {"inlier_scores": d.inlier_scores.numpy(), "sampson_dists": d.sampson_dists.numpy(), "quality": quality.numpy(),
               "max_score": np.float32(float(d.max_score)), "best_H_idx": np.int64(d.best_H_idx)}
        f64 = float64_run(case, idx)
        for key in ("X", "Y", "K"):
            out[f"{k}_{key}"] = case[key]
        out[f"{k}_seed"], out[f"{k}_hyps"], out[f"{k}_idx"] = np.int64(seed), np.int64(hyps), idx
        for name, val in ref.items():
            out[f"{k}_{name}"] = val
            out[f"{k}_f64_{name}"] = f64[name]
            if name != "best_H_idx":
                out[f"{k}_yard_{name}"] = np.float64(np.abs(np.asarray(val, np.float64) - f64[name]).max())
        out[f"{k}_f64_hyp_scores"] = f64["hyp_scores"]
        top = np.sort(f64["hyp_scores"])[::-1]
        print(f"case {k}: N {N} hyps {hyps}: best {int(ref['best_H_idx'])} (float64 {int(f64['best_H_idx'])}, top two scores "
              f"{top[0]:.6f} {top[1] if len(top) > 1 else float('nan'):.6f}), yardsticks " +
              ", ".join(f"{n} {float(out[f'{k}_yard_{n}']):.3g}" for n in ref if n != "best_H_idx"))
    path = os.path.join(HERE, "dsac.npz")
    np.savez_compressed(path, **out)
    print(f"dsac.npz: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
