"""The whole model at the reference's own training shape against the reference's own float64 run (tests/golden/refcfg.npz, written by
tests/golden/make_golden_refcfg.py): compat.DeepFNet with the default (fused) estimators, depth 5, 4 x 1000 and 2 x 2000 points, F-loss
and pose loss, every output and every parameter gradient.  GPU box only.

At this shape the package runs kernels its N = 100 golden test never reaches: the split-K estimator products with the register-resident
normalisation and adjoint (dfepe_est_norm_fwd_r / dfepe_est_in_bwd_r), update_weights four times on one parameter preparation, and the
cooperative 4-wavefront workgroup per pair in the fit.  Nothing in the ABI reports which fit kernel ran: the cooperative route follows
from the rule in csrc/fit_plan.h (128 < N <= 2048; forward fit of pixel matches up to 1280 pairs, backward fit up to 3072) for every fit
of the default step here; the same step is run a second
time with DFEPE_W8PT_ROW_PER_PAIR on every fit (one 16-lane row per pair), and BOTH routes are held to the fixture.

Yardstick: every compared quantity sits within max(4 x ref32_dist, floor) of the float64 truth, where ref32_dist is the distance of the
reference's OWN float32 run from that truth in the same metric (never this package), 4 = two independent fp32 evaluations of one function
(sqrt 2) times a maximum over 1e4 - 1e6 entries (~2), and floor = 1e-6 of the largest entry of the quantity's truth (~16 float32 ulps).
The fixture's parameters are the seeded ones with the last conv of both estimators scaled by head = 0.2: unscaled, the reference's
float32 run leaves its own float64 run by layer 3 (logits 3.6e-1, gradients > 100 %), and nothing can be pinned.

Norms and projections of a gradient are scalars, and one scalar's distance from the truth is near zero by chance one time in six: their
yardstick is the reference's |g32 - g64| on the FULL tensor (make_golden_refcfg.py), which bounds the one and is the expectation of the
other.  Their floor is that of the listed quantity -- "all gradient norms", "the projections": 1e-6 of the largest of the 44.

No pair, layer or parameter is masked.  The conv biases that cancel in an InstanceNorm need no exemption: this package's exact zero is
closer to the float64 run's ~1e-17 than the reference's float32 rounding noise is.

MEASURED (MI355X; the test prints every figure): all 4 x 2 x 2 runs pass, and this package is closer to the float64
truth than the reference's own float32 run in every quantity governed by 4 x ref32_dist -- worst ratio distance / ref32_dist 0.95 (weights
of layer 1 at 2 x 2000: 3.8e-10 against 4.1e-10).  Distance to the truth, worst over cases and routes (ratio): logits 5.8e-6 (0.71), weights
5.0e-9 (0.95), unit F 5.1e-7 (0.25), residual 5.2e-10 (0.41), epi_res 8.5e-6 (0.34), d loss / d logits 4.4e-8 (0.48), loss_layers 2.2e-9,
loss_F 1.3e-9 (0.20), q_l2 2.3e-8 (0.58), t_l2 3.1e-7 (0.40), full gradients / norms / projections of the 32 parameters that have a
gradient: 0.82 at 2 x 2000, 0.31 at 4 x 1000 (e.g. update_weights.fw.7.weight: 1.7e-4 of its norm against the reference's 3.4e-3).
Governed by the floor: loss_qt at 4 x 1000 (both float32 runs round to the same float, 1.0e-8 from the truth), t_l2 of the last layer at
2 x 2000 (ratio 0.30), and norm + projections of the 12 parameters whose gradient is zero in exact arithmetic: the ten conv biases in front
of an InstanceNorm (exact zero here) and the two head biases, which cancel in the softmax -- both float32 evaluations are a sum of
thousands of rounded d loss / d logits, 3e-7 ... 1.3e-5 of 1e-3 of the largest norm here, 4e-7 ... 1.9e-5 in the reference: one scalar of
noise each (ratios 0.08 ... 11), decided by the floor of 1e-3 in these units.
The two routes differ from each other by less than either differs from the truth, except d loss_F / d logits at 2 x 2000: 1.64e-9 between
them, 1.60e-9 to the truth (ulps of the largest entry, 3.4e-4).  The torch.cat and the zero-copy route are bit-identical.
Adam: loss 5.3e-9, 2.3e-9, 1.6e-8 from the truth (ratios 0.08, 0.01, 0.06), displacements <= 0.23 of the reference's float32 distance.
Sensitivity (scratch builds, one run each): dfepe_est_norm_fwd_r summing S - 1 of S partials, its eps 1e-5 -> 1e-4, the cooperative fit's
epi_res clamp 0.5 -> 0.4 -- each fails all five tests here (logits off by 0.5 ... 1.1, 3e-3 ... 2e-2, 0.15 ... 0.33); the earlier suite catches
them in 36, 39 and 9 tests (test_estimator_mfma_gpu / test_estimator_r6_gpu; test_w8pt_gpu / test_compat_gpu)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refcfg_fixture as rf  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def fx(golden):
    return rf.Fixture(golden("refcfg"))


def dev32(fx, key):
    return torch.from_numpy(np.asarray(fx[key], dtype=np.float32)).to(DEV)


def cpu64(t):
    return t.detach().to("cpu", torch.float64)


def make_net(dfepe, fx, head):
    net = dfepe.compat.DeepFNet.DeepFNet(depth=rf.DEPTH, image_size=rf.IMAGE_SIZE, if_quality=False)
    rf.build_cpu_params(net, dfepe.synth, fx["param_seed"], head)
    return net


def row_fit_function(ops):
    """The fit of DeepFNet._fit (ops.w8pt_raw_logits) with DFEPE_W8PT_ROW_PER_PAIR on the forward and the adjoint launch."""

    class RowFit(torch.autograd.Function):
        @staticmethod
        def forward(ctx, matches, logits, W, H, want_epi):
            ctx.set_materialize_grads(False)
            F, residual, epi, save, w = ops.w8pt_forward(matches, None, logits, True, W, H, 0.5, want_epi, want_save=True, logits=True,
                                                         row_per_pair=True)
            ctx.save_for_backward(matches, w, save, F)
            ctx.cfg = (W, H, want_epi)
            return (F, residual, epi, w) if want_epi else (F, residual, w)

        @staticmethod
        def backward(ctx, gF, gRes, *rest):
            matches, w, save, F = ctx.saved_tensors
            W, H, want_epi = ctx.cfg
            gEpi, gW = rest if want_epi else (None, rest[0])
            if gF is None and gRes is None and gEpi is None and gW is None:
                return None, None, None, None, None
            cf = lambda t: None if t is None else t.contiguous().float()  # noqa: E731
            g = ops.w8pt_backward(matches, None, w, True, W, H, 0.5, save, F, cf(gF), cf(gRes), cf(gEpi), logits=True, gW_extra=cf(gW),
                                  row_per_pair=True)
            return None, g, None, None, None

    return RowFit


def install_fit(dfepe, net, gauge, row):
    """``gauge``: None (the model as users run it), "+1" (the wrapper's sign is identically +1) or a list of [B,3,3] reference F, one per
    fit call, whose sign is imposed on (out, residual) the way test_deepfnet_full_model_matches_reference_golden does."""
    if gauge is None and not row:
        return
    inner, call = net._fit, {"i": 0}
    RowFit = row_fit_function(dfepe.ops)
    H, W = float(rf.IMAGE_SIZE[0]), float(rf.IMAGE_SIZE[1])

    def fit(matches, logits, data_batch, want_epi, dst=None):
        if row:
            o = RowFit.apply(matches.contiguous(), logits.reshape(logits.shape[0], -1).contiguous(), W, H, want_epi)
            o = o[:-1] + (o[-1].unsqueeze(1),)
        else:
            o = inner(matches, logits, data_batch, want_epi, dst)
        if isinstance(gauge, str):
            s = torch.ones(o[0].shape[0], device=o[0].device)
        else:
            s = torch.sign((o[0].detach() * gauge[call["i"]]).flatten(1).sum(1))
        call["i"] += 1
        return (o[0] * s[:, None, None], o[1] * s[:, None]) + tuple(o[2:])

    net._fit = fit


def step(dfepe, fx, case, net, monkeypatch, objective=None):
    """One forward (+ one backward of ``objective``: "F", "qt" or "adam") of ``net`` on the case's scene."""
    tg = dfepe.compat.train_good_utils
    b = {k: dev32(fx, f"{case}_{k}") for k in rf.SCENE_KEYS}
    taken = {"n": 0}
    inner = dfepe.ops.estimator_input

    def counted(*a, **kw):
        taken["n"] += 1
        return inner(*a, **kw)

    monkeypatch.setattr(dfepe.ops, "estimator_input", counted)
    outs = net({"matches_xy_ori": b["matches_xy_ori"], "matches_good_unique_nums": None, "t_scene_scale": None})
    monkeypatch.setattr(dfepe.ops, "estimator_input", inner)
    losses, _, _, _, _, _, E_layers = tg.get_all_loss_DeepF(outs, b["pts1_virt_ori"], b["pts2_virt_ori"], b["Ks"], dict(rf.LOSS_PARAMS),
                                                            get_residual_summaries=False)
    geo = tg.get_Rt_loss(E_layers, b["Ks"], None, None, b["delta_Rtijs_4_4"], b["qs_cam"], b["ts_cam"], device=DEV)
    q_l2, t_l2 = torch.stack(list(geo["q_l2_error_layers_list"])), torch.stack(list(geo["t_l2_error_layers_list"]))
    loss_q, loss_t = torch.clamp(q_l2, 0.0, 0.1).mean(), torch.clamp(t_l2, 0.0, 0.5).mean()
    loss_qt = loss_q * 1.0 + loss_t * 0.1
    r = {"zero_copy_inputs": taken["n"], "grad_fns": [type(l.grad_fn).__name__ for l in outs["logits_layers"]]}
    loss = {"F": losses["loss_F"], "qt": loss_qt, "adam": losses["loss_F"] + loss_q + 0.1 * loss_t, None: None}[objective]
    if loss is not None:
        for l in outs["logits_layers"]:
            l.retain_grad()
        for p in net.parameters():
            p.grad = None
        loss.backward()
        r["dlogits"] = torch.stack([cpu64(l.grad) for l in outs["logits_layers"]]).squeeze(2)
        r["grads"] = {n: (torch.zeros(p.shape, dtype=torch.float64) if p.grad is None else cpu64(p.grad)) for n, p in net.named_parameters()}
        r["loss"] = cpu64(loss)
    r.update({"logits_layers": torch.stack([cpu64(x) for x in outs["logits_layers"]]).squeeze(2),
              "weights_layers": torch.stack([cpu64(x) for x in outs["weights_layers"]]).squeeze(2),
              "out_layers": torch.stack([cpu64(x) for x in outs["out_layers"]]),
              "residual_layers": torch.stack([cpu64(x) for x in outs["residual_layers"]]),
              "epi_res_layers": torch.stack([cpu64(x) for x in outs["epi_res_layers"]]).squeeze(2),
              "loss_layers": torch.stack([cpu64(x) for x in losses["loss_layers"]]).reshape(-1), "loss_F": cpu64(losses["loss_F"]).reshape(()),
              "loss_qt": cpu64(loss_qt).reshape(()), "q_l2_layers": cpu64(q_l2).reshape(rf.DEPTH, -1), "t_l2_layers": cpu64(t_l2).reshape(rf.DEPTH, -1)})
    return r


def distances_to_fixture(r, fx, case, tag):
    """[(name, distance, ref32_dist, largest entry of the truth)] in the metrics of make_golden_refcfg.py."""
    rows = []
    truth = {k: fx.t(f"{case}_{k}") for k in ("logits_layers", "residual_layers", "epi_res_layers", "out_layers", "loss_layers", "loss_F", "loss_qt",
                                             "q_l2_layers", "t_l2_layers")}
    truth["weights_layers"] = fx.weights(case)
    truth["dlogits_" + tag] = fx.t(f"{case}_dlogits_{tag}")
    got = dict(r)
    got["dlogits_" + tag] = r["dlogits"]
    ref = lambda k: np.atleast_1d(fx[f"{case}_ref32_dist_{k}"])  # noqa: E731
    for k in ("logits_layers", "weights_layers", "residual_layers", "epi_res_layers", "dlogits_" + tag):
        assert got[k].shape == truth[k].shape, (k, got[k].shape, truth[k].shape)
        for l in range(truth[k].shape[0]):
            rows.append((f"{k}[{l}]", float((got[k][l] - truth[k][l]).abs().max()), float(ref(k)[l]), float(truth[k][l].abs().max())))
    uf = rf.unit_f_dist(got["out_layers"], truth["out_layers"])
    for l in range(rf.DEPTH):
        rows.append((f"unitF[{l}]", float(uf[l]), float(ref("unitF_layers")[l]), float(rf.unit(truth["out_layers"][l]).abs().max())))
    rows.append(("loss_layers", float((got["loss_layers"] - truth["loss_layers"]).abs().max()), float(ref("loss_layers")[0]),
                 float(truth["loss_layers"].abs().max())))
    for k in ("loss_F", "loss_qt"):
        rows.append((k, float((got[k] - truth[k].reshape(())).abs()), float(ref(k)[0]), float(truth[k].abs().max())))
    for k in ("q_l2_layers", "t_l2_layers"):
        for l in range(rf.DEPTH):
            rows.append((f"{k}[{l}]", float((got[k][l] - truth[k][l]).abs().max()), float(ref(k)[l]), float(truth[k][l].abs().max())))
    # parameter gradients: norms, 4 projections per parameter, the full small tensors; yardstick of all three = the reference's float32
    # run's |g - g64| on the full tensor (the generator's docstring says why a scalar's own distance is no yardstick)
    names = sorted(r["grads"])
    assert len(names) == 44
    n64, p64, yard = fx.t(f"{case}_grad_norms_{tag}"), fx.t(f"{case}_grad_proj_{tag}"), fx[f"{case}_ref32_dist_grad_{tag}"]
    # The floor: "all gradient norms" is ONE quantity (a 44-vector) and so are the 44 x 4 projections -- 1e-6 of the largest norm /
    # projection, here divided by the parameter's denominator like the distance; each full small tensor is a quantity of its own.
    den = rf.grad_denominators(n64)
    for i, n in enumerate(names):
        g = r["grads"][n].flatten()
        rows.append((f"gnorm {n}", float((g.norm() - n64[i]).abs() / den[i]), float(yard[i]), float(n64.max() / den[i])))
        proj = rf.directions(fx["dir_seed"], i, g.numel()) @ g
        rows.append((f"gproj {n}", float((proj - p64[i]).pow(2).mean().sqrt() / den[i]), float(yard[i]), float(p64.abs().max() / den[i])))
        if n in fx.small():
            g64 = fx.t(f"{case}_grad_{tag}_{n}").flatten()
            rows.append((f"gfull {n}", float((g - g64).norm() / den[i]), float(yard[i]), float(g64.abs().max() / den[i])))
    return rows


def report(title, rows):
    """Prints every figure, then returns the rows that miss max(4 x ref32_dist, floor)."""
    bad, floor_governed, worst = [], [], 0.0
    print(f"\n== {title}: distance to the float64 truth | the reference's float32 run | ratio | bound")
    for name, d, ref, top in rows:
        bnd = rf.bound(ref, top)
        by_floor = rf.FLOOR * top > rf.FACTOR * ref
        ratio = d / ref if ref > 0 else float("inf") if d > 0 else 0.0
        if not by_floor:
            worst = max(worst, ratio)
        else:
            floor_governed.append(name)
        flag = "" if d <= bnd else "   <-- MISSES"
        print(f"{name:46s} {d:10.3e} {ref:10.3e} {ratio:8.2f} {bnd:10.3e}{' (floor)' if by_floor else ''}{flag}")
        if not d <= bnd:
            bad.append((name, d, ref, bnd))
    print(f"-- {title}: worst ratio among the quantities governed by 4 x ref32_dist: {worst:.2f}; governed by the floor: {floor_governed}")
    return bad


@pytest.mark.parametrize("tag", ["F", "qt"])
@pytest.mark.parametrize("case", sorted(rf.CASES))
def test_whole_model_matches_the_reference_float64_run_at_its_training_shape(dfepe, fx, monkeypatch, case, tag):
    """See the module docstring.  Four steps of the same model: cooperative fit and row-per-pair fit, both in the fixture's gauge and both
    held to the fixture; then the wrapper with sign = +1 (multiplication by exactly 1.0, still the torch.cat route) and no wrapper at all
    (the zero-copy route production takes: the fit writes weights / epi / residual into the channel-major stores and
    ops.estimator_input hands them on) -- all outputs and parameter gradients of those two bit-identical."""
    net = make_net(dfepe, fx, float(fx["head"]))
    assert sorted(net.state_dict().keys()) == [str(k) for k in fx[case + "_state_keys"]]
    chk = np.array([float(p.detach().double().abs().sum()) for _, p in sorted(net.named_parameters())])
    np.testing.assert_allclose(chk, fx[case + "_param_checksum"], rtol=1e-12)
    net = net.to(DEV)
    gauge = list(dev32(fx, case + "_out_layers"))
    orig_fit = net._fit
    runs, rows = {}, {}
    for route in ("cooperative", "row_per_pair"):
        net._fit = orig_fit
        install_fit(dfepe, net, gauge, row=(route == "row_per_pair"))
        r = runs[route] = step(dfepe, fx, case, net, monkeypatch, tag)
        assert all(name.startswith("_EstimatorPackedFunction") for name in r["grad_fns"][1:]), r["grad_fns"]
        assert r["zero_copy_inputs"] == 0
        rows[route] = distances_to_fixture(r, fx, case, tag)
    bad = {route: report(f"{case} loss_{tag} {route}", rows[route]) for route in rows}
    # the two routes are documented as the same function: where they differ by more than they differ from the truth, say so
    for k, row_name in (("logits_layers", "logits_layers["), ("weights_layers", "weights_layers["), ("out_layers", "unitF["),
                        ("residual_layers", "residual_layers["), ("epi_res_layers", "epi_res_layers["), ("dlogits", "dlogits_")):
        x, y = runs["cooperative"][k], runs["row_per_pair"][k]
        between = float(rf.unit_f_dist(x, y).max()) if k == "out_layers" else float((x - y).abs().max())
        to_truth = max(d for route in rows for name, d, _, _ in rows[route] if name.startswith(row_name))
        print(f"routes: {k:16s} |cooperative - row_per_pair| = {between:.3e}; largest distance of either to the truth = {to_truth:.3e}"
              + ("   <-- the routes differ by more than they differ from the truth" if between > to_truth else ""))
    assert not bad["cooperative"] and not bad["row_per_pair"], bad

    # production plumbing: sign = +1 through the wrapper (torch.cat route) against no wrapper at all (zero-copy route)
    net._fit = orig_fit
    install_fit(dfepe, net, "+1", row=False)
    a = step(dfepe, fx, case, net, monkeypatch, tag)
    assert a["zero_copy_inputs"] == 0
    net._fit = orig_fit
    b = step(dfepe, fx, case, net, monkeypatch, tag)
    assert b["zero_copy_inputs"] == rf.DEPTH - 1, "the production forward did not take the stores / ops.estimator_input route"
    diff = [k for k in ("logits_layers", "weights_layers", "out_layers", "residual_layers", "epi_res_layers", "loss_layers", "loss_F", "loss_qt",
                        "q_l2_layers", "t_l2_layers", "dlogits", "loss") if not torch.equal(a[k], b[k])]
    diff += ["grad " + n for n in a["grads"] if not torch.equal(a["grads"][n], b["grads"][n])]
    for k in diff:
        x, y = (a["grads"][k[5:]], b["grads"][k[5:]]) if k.startswith("grad ") else (a[k], b[k])
        print(f"plumbing: {k} differs between the torch.cat and the zero-copy route by {float((x - y).abs().max()):.3e} (largest entry {float(y.abs().max()):.3e})")
    assert not diff, diff


def test_three_adam_steps_follow_the_reference_trajectory(dfepe, fx, monkeypatch):
    """Three eager Adam steps (lr 1e-4, loss_F + loss_q + 0.1 loss_t, head 0.05, the n1000 scene) against the reference's float64
    trajectory: the loss of every step within max(4 x the reference's float32 distance, 1e-6 of the loss), and the displacement
    p3 - p0 of the small tensors within 4 x the reference's float32 distance.  The estimator parameters are prepared once per forward
    (shared_parameters(): packed vector + weight planes); a preparation that went stale after optimizer.step() is an error of ~1e-1
    here (the loss falls ~9 % per step) where the package's own A/B training tests would both carry it."""
    pre = "n1000_adam_"
    assert pre + "loss_steps" in fx
    net = make_net(dfepe, fx, float(fx[pre + "head"])).to(DEV)
    p0 = {n: p.detach().clone() for n, p in net.named_parameters()}
    gauges = fx[pre + "out_layers_steps"]
    opt = torch.optim.Adam(net.parameters(), lr=float(fx[pre + "lr"]))
    orig_fit = net._fit
    bad = []
    for k in range(int(fx[pre + "steps"])):
        net._fit = orig_fit
        install_fit(dfepe, net, list(torch.from_numpy(gauges[k].astype(np.float32)).to(DEV)), row=False)
        r = step(dfepe, fx, "n1000", net, monkeypatch, "adam")
        opt.step()
        truth, ref = float(fx[pre + "loss_steps"][k]), float(fx[pre + "ref32_dist_loss_steps"][k])
        d, bnd = abs(float(r["loss"]) - truth), rf.bound(ref, abs(truth))
        print(f"adam step {k}: loss {float(r['loss']):.9e} truth {truth:.9e} distance {d:.3e} reference float32 {ref:.3e} ratio {d / ref:.2f} bound {bnd:.3e}")
        if not d <= bnd:
            bad.append(("loss", k, d, bnd))
    params = dict(net.named_parameters())
    for n in fx.small():
        disp64 = fx.t(pre + "disp_" + n)
        disp = cpu64(params[n]) - cpu64(p0[n])
        d, ref = float((disp - disp64).norm() / disp64.norm()), float(fx[pre + "ref32_dist_disp_" + n])
        print(f"adam displacement {n}: relative distance {d:.3e} reference float32 {ref:.3e} ratio {d / ref:.2f}")
        if not d <= rf.FACTOR * ref:
            bad.append((n, d, ref))
    assert not bad, bad
