#!/usr/bin/env python3
"""Golden vectors that pin the WHOLE model at the reference's own training shape (every shipped config runs
DeepFNet with good_num 1000, depth 5, a few pairs per batch, deepFEPE/configs/kitti_corr_baseline.yaml:12-13,35).

The reference itself runs (imported unmodified, see make_golden.py), twice per case: in float64 -- the truth that is stored --
and in float32 -- of which ONLY its distance from the truth is stored (``ref32_dist_*``): that distance is the yardstick the GPU
test holds this package to (tests/test_refcfg_gpu.py: within 4 x of it).  The inputs are rounded to float32 FIRST and the
float64 run consumes those float32 values cast up; the parameters are filled into the float32 module (synth.fill_params_deterministic,
then the last conv of both estimators scaled by ``head``) and the float64 module is that module cast up: both precisions and the GPU see
identical numbers.  The float32 run has the float64 run's SVD sign imposed on every fit's (out, residual) by the few lines of
``impose_gauge`` below, applied at run time around net.fit.forward (the sign is LAPACK's arbitrary one).

Cases: n1000 (B = 4, N = 1000), n2000 (B = 2, N = 2000); depth 5, if_quality False, scene make_scene(seed 31, outlier_ratio 0.2,
noise_px 0.5), parameters seed 5.  ``head`` is the largest of HEADS for which the reference ALONE meets CAPS on both cases (asserted;
nothing is written otherwise): with the seeded random parameters unscaled the reference's float32 run leaves its own float64 run by
layer 3, so nothing can be pinned there.  n1000_adam: three Adam steps (lr 1e-4, loss_F + loss_q + 0.1 loss_t) at head 0.05.

Distances (the GPU test uses the same):
  per-point arrays (logits, weights, residual, epi_res, d loss / d logits), per layer: max |a - truth|
  F per layer: max over the pairs of |unit(a) - unit(truth)|_Frobenius
  losses, q / t errors: |a - truth| (q / t: max over the pairs of a layer; loss_layers: max over the layers)
  gradient of a parameter p: |g - g64| / max(|g64|, 1e-3 * largest |g64| over the parameters)                           (*)
Gradient norms and the 4 projections per parameter are scalars: one scalar's distance from the truth is near zero by chance one
time in six, so it is no yardstick of its own.  Both are bounded by / estimate |g - g64| (| |g| - |g64| | <= |g - g64|; the root mean
square of the projections on unit-variance Gaussian directions has expectation |g - g64|), so ``ref32_dist_grad_<objective>`` -- (*)
of the reference's float32 run on the FULL tensors, which only this generator has -- is the yardstick of all three.

Directions: for the parameter of index i in the sorted names and k in 0..3,
torch.randn(numel, generator=torch.Generator().manual_seed(DIR_SEED * 1000003 + 4 * i + k), dtype=float64).

    python tests/golden/make_golden_refcfg.py      # rewrites tests/golden/refcfg.npz (build container only)
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (stubs, synth, quiet)

DEPTH = 5
SCENE_SEED, PARAM_SEED, DIR_SEED = 31, 5, 977
HEADS = (0.5, 0.2, 0.1, 0.05)
CASES = {"n1000": (4, 1000), "n2000": (2, 2000)}
CAPS = {"logits": 2e-4, "unitF": 2e-5, "grad": 1e-2}
ADAM_HEAD, ADAM_STEPS, ADAM_LR, ADAM_CAP = 0.05, 3, 1e-4, 1e-5
# tensors whose full gradient is stored: first conv and head conv of each estimator, gamma / beta of the 1024-wide InstanceNorm
SMALL = ("input_weights.fw.0.weight", "input_weights.fw.15.weight", "update_weights.fw.0.weight", "update_weights.fw.15.weight",
         "update_weights.fw.7.weight", "update_weights.fw.7.bias")
LOSS_PARAMS = {"depth": DEPTH, "clamp_at": 0.02, "if_tri_depth": False, "if_sample_loss": False, "topK": 8, "matches_good_unique_nums": None}
SCENE_KEYS = ("matches_xy_ori", "Ks", "delta_Rtijs_4_4", "qs_cam", "ts_cam", "pts1_virt_ori", "pts2_virt_ori")
# stored as float32(float64 value): the per-point arrays other than the logits, the full small gradients and the Adam displacements.
# weights_layers is not stored at all: it is softmax(logits_layers) over the points (deepFEPE/models/DeepFNet.py:443,512), which the
# tests evaluate in float64 from the stored float64 logits.  That, and the byte planes below, is what keeps the file within 1 MiB.
ROUNDED = ("residual_layers", "epi_res_layers", "dlogits_F", "dlogits_qt")


def put(out, key, a):
    """Large float arrays are stored as byte planes (uint8 [itemsize, size]: byte k of every element together, which deflate packs
    ~10 % tighter) under ``key + "__planes"`` with ``key + "__shape"``; tests/refcfg_fixture.py:get undoes it exactly."""
    a = np.asarray(a)
    if a.dtype.kind == "f" and a.size >= 2000:
        out[key + "__planes"] = np.ascontiguousarray(np.ascontiguousarray(a).reshape(-1).view(np.uint8).reshape(-1, a.itemsize).T)
        out[key + "__shape"] = np.array(a.shape)
    else:
        out[key] = a


def directions(i, numel):
    return torch.stack([torch.randn(numel, generator=torch.Generator().manual_seed(DIR_SEED * 1000003 + 4 * i + k), dtype=torch.float64)
                        for k in range(4)])


def build_nets(DeepFNet, head):
    with mg.quiet():
        net32 = DeepFNet(depth=DEPTH, image_size=mg.IMAGE_SIZE, if_quality=False, is_cuda=False, if_cpu_svd=False)
    mg.synth.fill_params_deterministic(net32, seed=PARAM_SEED)
    with torch.no_grad():
        for est in (net32.input_weights, net32.update_weights):
            est.fw[-1].weight.mul_(head)
    net64 = copy.deepcopy(net32).double()
    net64.norm_HW.ones_b = net64.norm_HW.ones_b.double()
    for a in ("ones_b", "zero_b", "T_b", "mask"):
        setattr(net64.fit, a, getattr(net64.fit, a).double())
    return net32, net64


def impose_gauge(net, out_layers_ref):
    """From here on every fit of ``net`` returns (out, residual) in the sign of out_layers_ref[call index]."""
    inner, call = net.fit.forward, {"i": 0}

    def forward(*a, **kw):
        out, residual = inner(*a, **kw)
        ref = out_layers_ref[call["i"] % len(out_layers_ref)]
        call["i"] += 1
        s = torch.sign((out.detach().double() * ref).flatten(1).sum(1)).to(out.dtype)
        return out * s[:, None, None], residual * s[:, None]

    net.fit.forward = forward


def evaluate(net, sc, dt, tgu, grads=True):
    s = {k: sc[k].to(dt) for k in SCENE_KEYS}
    with mg.quiet():
        outs = net({"matches_xy_ori": s["matches_xy_ori"], "matches_good_unique_nums": None, "t_scene_scale": None})
        losses, _, _, _, _, _, E_layers = tgu.get_all_loss_DeepF(outs, s["pts1_virt_ori"], s["pts2_virt_ori"], s["Ks"], LOSS_PARAMS,
                                                                 get_residual_summaries=False)
        rt = tgu.get_Rt_loss(E_layers, s["Ks"], s["matches_xy_ori"][:, :, :2], s["matches_xy_ori"][:, :, 2:], s["delta_Rtijs_4_4"],
                             s["qs_cam"], s["ts_cam"], device="cpu")
    q_l2, t_l2 = torch.stack(rt["q_l2_error_layers_list"]), torch.stack(rt["t_l2_error_layers_list"])
    loss_q, loss_t = torch.clamp(q_l2, 0.0, 0.1).mean(), torch.clamp(t_l2, 0.0, 0.5).mean()
    loss_qt = loss_q * 1.0 + loss_t * 0.1
    r = {"logits_layers": torch.stack(outs["logits_layers"]).squeeze(2), "weights_layers": torch.stack(outs["weights_layers"]).squeeze(2),
         "out_layers": torch.stack(outs["out_layers"]), "residual_layers": torch.stack(outs["residual_layers"]),
         "epi_res_layers": torch.stack(outs["epi_res_layers"]).squeeze(2), "loss_layers": torch.stack(losses["loss_layers"]),
         "loss_F": losses["loss_F"], "E_layers": torch.stack(E_layers), "q_l2_layers": q_l2.reshape(DEPTH, -1),
         "t_l2_layers": t_l2.reshape(DEPTH, -1), "loss_qt": loss_qt}
    r = {k: v.detach().double() for k, v in r.items()}
    r["_loss_adam"] = losses["loss_F"] + loss_q + 0.1 * loss_t
    if grads:
        names = sorted(n for n, _ in net.named_parameters())
        params = dict(net.named_parameters())
        wrt = [params[n] for n in names] + list(outs["logits_layers"])
        for tag, loss in (("F", losses["loss_F"]), ("qt", loss_qt)):
            g = torch.autograd.grad(loss, wrt, retain_graph=True)
            r["_grads_" + tag] = [x.detach().double() for x in g[:len(names)]]
            r["dlogits_" + tag] = torch.stack(g[len(names):]).squeeze(2).detach().double()
    return r


def unit(F):
    return F / F.flatten(-2).norm(dim=-1)[..., None, None]


def grad_dist(g, g64):
    n64 = torch.stack([x.norm() for x in g64])
    return torch.stack([(a - b).norm() for a, b in zip(g, g64)]) / torch.maximum(n64, 1e-3 * n64.max())


def distances(a, t):
    """The float32 run ``a`` against the truth ``t``, in the metrics of the module docstring."""
    d = {}
    for k in ("logits_layers", "weights_layers", "residual_layers", "epi_res_layers", "dlogits_F", "dlogits_qt"):
        d[k] = (a[k] - t[k]).abs().flatten(1).max(1)[0]
    d["unitF_layers"] = (unit(a["out_layers"]) - unit(t["out_layers"])).flatten(2).norm(dim=2).max(1)[0]
    d["loss_layers"] = (a["loss_layers"] - t["loss_layers"]).abs().max()
    for k in ("loss_F", "loss_qt"):
        d[k] = (a[k] - t[k]).abs()
    for k in ("q_l2_layers", "t_l2_layers"):
        d[k] = (a[k] - t[k]).abs().max(1)[0]
    for tag in ("F", "qt"):
        d["grad_" + tag] = grad_dist(a["_grads_" + tag], t["_grads_" + tag])
    return d


def within_caps(d):
    return (float(d["logits_layers"].max()) <= CAPS["logits"] and float(d["unitF_layers"].max()) <= CAPS["unitF"]
            and float(d["grad_F"].max()) <= CAPS["grad"] and float(d["grad_qt"].max()) <= CAPS["grad"])


def run_case(DeepFNet, tgu, B, N, head):
    sc = mg.synth.make_scene(B, N, seed=SCENE_SEED, outlier_ratio=0.2, noise_px=0.5, dtype=torch.float32, depth_layers=DEPTH)
    net32, net64 = build_nets(DeepFNet, head)
    t = evaluate(net64, sc, torch.float64, tgu)
    impose_gauge(net32, t["out_layers"])
    a = evaluate(net32, sc, torch.float32, tgu)
    return sc, net32, net64, t, a, distances(a, t)


def pack_case(out, pre, sc, net64, t, d):
    names = sorted(n for n, _ in net64.named_parameters())
    for k in SCENE_KEYS:
        put(out, pre + k, mg.npy(sc[k]))
    out[pre + "state_keys"] = np.array(sorted(net64.state_dict().keys()))
    out[pre + "param_checksum"] = np.array([float(p.detach().abs().sum()) for _, p in sorted(net64.named_parameters())])
    for k in ("logits_layers", "out_layers", "loss_layers", "loss_F", "E_layers", "q_l2_layers", "t_l2_layers", "loss_qt"):
        put(out, pre + k, mg.npy(t[k]))
    for k in ROUNDED:
        put(out, pre + k, mg.npy(t[k]).astype(np.float32))
    for tag in ("F", "qt"):
        g = t["_grads_" + tag]
        out[pre + f"grad_norms_{tag}"] = np.array([float(x.norm()) for x in g])
        out[pre + f"grad_proj_{tag}"] = np.stack([mg.npy(directions(i, x.numel()) @ x.flatten()) for i, x in enumerate(g)])
        for n in SMALL:
            put(out, pre + f"grad_{tag}_{n}", mg.npy(g[names.index(n)]).astype(np.float32))
    for k, v in d.items():
        out[pre + "ref32_dist_" + k] = mg.npy(v)


def adam_case(DeepFNet, tgu, out):
    """Three Adam steps of the reference in float64 (stored) and in float32 (distance only), on the n1000 scene at ADAM_HEAD."""
    B, N = CASES["n1000"]
    sc = mg.synth.make_scene(B, N, seed=SCENE_SEED, outlier_ratio=0.2, noise_px=0.5, dtype=torch.float32, depth_layers=DEPTH)
    net32, net64 = build_nets(DeepFNet, ADAM_HEAD)
    p0 = {n: p.detach().clone() for n, p in net64.named_parameters()}
    losses, gauges = {}, []
    for tag, net, dt in (("f64", net64, torch.float64), ("f32", net32, torch.float32)):
        if tag == "f32":
            impose_gauge(net, [g for step in gauges for g in step])
        opt = torch.optim.Adam(net.parameters(), lr=ADAM_LR)
        losses[tag] = []
        for _ in range(ADAM_STEPS):
            r = evaluate(net, sc, dt, tgu, grads=False)
            if tag == "f64":
                gauges.append(r["out_layers"])
            opt.zero_grad()
            r["_loss_adam"].backward()
            opt.step()
            losses[tag].append(float(r["_loss_adam"].detach().double()))
    l64, l32 = np.array(losses["f64"]), np.array(losses["f32"])
    rel = np.abs(l32 - l64) / np.abs(l64)
    pre = "n1000_adam_"
    out[pre + "head"], out[pre + "lr"], out[pre + "steps"] = np.array(ADAM_HEAD), np.array(ADAM_LR), np.array(ADAM_STEPS)
    out[pre + "loss_steps"] = l64
    out[pre + "out_layers_steps"] = np.stack([mg.npy(g) for g in gauges])
    out[pre + "ref32_dist_loss_steps"] = np.abs(l32 - l64)
    p32 = dict(net32.named_parameters())
    for n in SMALL:
        disp = dict(net64.named_parameters())[n].detach() - p0[n]
        disp32 = p32[n].detach().double() - p0[n]  # p0 is the float32 start cast up: the same for both runs
        put(out, pre + "disp_" + n, mg.npy(disp).astype(np.float32))
        out[pre + "ref32_dist_disp_" + n] = mg.npy((disp32 - disp).norm() / disp.norm())
    return rel


def main():
    mg.install_stubs()
    with mg.quiet():
        from deepFEPE.models.DeepFNet import DeepFNet
        import train_good_utils as tgu
    torch.set_num_threads(4)
    chosen, log = None, []
    for head in HEADS:
        runs = {name: run_case(DeepFNet, tgu, B, N, head) for name, (B, N) in CASES.items()}
        for name, r in runs.items():
            d = r[-1]
            log.append(f"head {head} {name}: logits {float(d['logits_layers'].max()):.1e} unitF {float(d['unitF_layers'].max()):.1e} "
                       f"grad F {float(d['grad_F'].max()):.1e} qt {float(d['grad_qt'].max()):.1e}")
            print(log[-1])
        if all(within_caps(r[-1]) for r in runs.values()):
            chosen = head
            break
    assert chosen is not None, "the reference's own float32 run meets the caps at no head of " + str(HEADS)
    out = {"head": np.array(chosen), "scene_seed": np.array(SCENE_SEED), "param_seed": np.array(PARAM_SEED), "dir_seed": np.array(DIR_SEED),
           "depth": np.array(DEPTH), "heads_tried": np.array(HEADS), "small": np.array(SMALL),
           "cap_logits": np.array(CAPS["logits"]), "cap_unitF": np.array(CAPS["unitF"]), "cap_grad": np.array(CAPS["grad"])}
    for name, (sc, net32, net64, t, a, d) in runs.items():
        assert within_caps(d)
        pack_case(out, name + "_", sc, net64, t, d)
    rel = adam_case(DeepFNet, tgu, out)
    print("adam: relative float32-to-float64 loss distance per step", rel.tolist())
    adam_ok = bool((rel <= ADAM_CAP).all())
    if not adam_ok:
        for k in [k for k in out if k.startswith("n1000_adam_")]:
            del out[k]
    out["adam_cap"] = np.array(ADAM_CAP)
    path = os.path.join(HERE, "refcfg.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= 1024 * 1024, size
    line = (f"refcfg.npz: {len(out)} arrays, {size} bytes (make_golden_refcfg.py: the reference's DeepFNet at depth 5, B x N = 4 x 1000 and "
            f"2 x 2000, float64 truth + its own float32 run's distances; head {chosen}; stored as the float32 rounding of the float64 values: "
            f"{', '.join(ROUNDED)}, grad_<objective>_<small tensor>, disp_<small tensor>; weights_layers = softmax(logits_layers), not stored; three Adam steps at head {ADAM_HEAD}: "
            + ("float32-to-float64 loss distance " + ", ".join(f"{x:.1e}" for x in rel) + f" <= {ADAM_CAP:g}, stored" if adam_ok else
               "float32-to-float64 loss distance " + ", ".join(f"{x:.1e}" for x in rel) + f" exceeds {ADAM_CAP:g} with exactly rounded inputs: left out") + ")\n")
    mpath = os.path.join(HERE, "MANIFEST.txt")
    with open(mpath) as f:
        lines = [l for l in f if not l.startswith("refcfg.npz:")]
    with open(mpath, "w") as f:
        f.writelines(lines + [line])
    print(line)


if __name__ == "__main__":
    main()
