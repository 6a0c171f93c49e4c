"""tests/golden/refcfg.npz (the reference's own float64 run of the whole model at its training shape: depth 5, 4 x 1000 and 2 x 2000
points, tests/golden/make_golden_refcfg.py) against this repository's two CPU restatements, in float64, without a GPU:

* oracle.deepf_forward / f_loss / rt_loss / qt_training_loss and their float64 autograd;
* compat.ErrorEstimators.ErrorEstimator (the stock mirror, a plain torch module) and the ``net_in`` channel order.

Both sides are float64, so the bounds are 1e-8 of each quantity's largest entry (float64 rounding times a generous conditioning
factor), 1e-9 for the mirror's logits; arrays the fixture stores as the float32 rounding of the float64 values (MANIFEST.txt) are
held to 2e-7 of their largest entry, the storage rounding."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refcfg_fixture as rf  # noqa: E402

F64, F32_STORED = 1e-8, 2e-7


@pytest.fixture(scope="module")
def fx(golden):
    return rf.Fixture(golden("refcfg"))


def close(a, t, rel, what):
    a, t = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(t, dtype=torch.float64)
    assert a.shape == t.shape, (what, a.shape, t.shape)
    d, top = float((a - t).abs().max()), float(t.abs().max())
    assert d <= rel * top, f"{what}: distance {d:.3e} of a largest entry {top:.3e} (ratio {d / top:.2e}, bound {rel:g})"


def scene(fx, case):
    return {k: fx.t(f"{case}_{k}") for k in rf.SCENE_KEYS}


def mirror(dfepe, fx):
    """compat.DeepFNet with the stock estimators and the fixture's parameters, float64, on the CPU (only its two estimators run)."""
    net = dfepe.compat.DeepFNet.DeepFNet(depth=rf.DEPTH, image_size=rf.IMAGE_SIZE, if_quality=False, fused_estimator=False)
    rf.build_cpu_params(net, dfepe.synth, fx["param_seed"], fx["head"])
    return net.double()


def gauged_fit(oracle, monkeypatch, out_ref):
    """oracle.fit_forward with the fixture's SVD sign imposed on (out, residual), call by call (LAPACK's sign is arbitrary)."""
    inner, call = oracle.fit_forward, {"i": 0}

    def fit(pts1, pts2, w, mode="batched", normalize_svd=True):
        out, residual, aux = inner(pts1, pts2, w, mode, normalize_svd)
        s = torch.sign((out.detach() * out_ref[call["i"]]).flatten(1).sum(1))
        call["i"] += 1
        return out * s[:, None, None], residual * s[:, None], aux

    monkeypatch.setattr(oracle, "fit_forward", fit)


def losses_of(oracle, outs, sc):
    losses, _, _, E_layers = oracle.f_loss(outs, sc["pts1_virt_ori"], sc["pts2_virt_ori"], sc["Ks"], rf.DEPTH, rf.LOSS_PARAMS["clamp_at"])
    pose = oracle.rt_loss(E_layers, sc["delta_Rtijs_4_4"], sc["qs_cam"], sc["ts_cam"])
    loss_qt = oracle.qt_training_loss(pose["q_l2"], pose["t_l2"], 0.1, 0.5, 1.0, 0.1)
    return losses, E_layers, pose, loss_qt


@pytest.mark.parametrize("case", sorted(rf.CASES))
def test_oracle_reproduces_the_reference_at_its_training_shape(oracle, fx, monkeypatch, case):
    """The oracle's forward and losses with the fixture's logits fed in, N = 1000 / 2000, depth 5."""
    sc = scene(fx, case)
    gauged_fit(oracle, monkeypatch, fx.t(case + "_out_layers"))
    outs = oracle.deepf_forward(sc["matches_xy_ori"], rf.IMAGE_SIZE, rf.DEPTH, logits_layers=fx.t(case + "_logits_layers"))
    close(torch.stack(outs["out_layers"]), fx.t(case + "_out_layers"), F64, "out_layers")
    close(torch.stack(outs["weights_layers"]).squeeze(2), fx.weights(case), F64, "weights_layers")
    close(torch.stack(outs["residual_layers"]), fx.t(case + "_residual_layers"), F32_STORED, "residual_layers")
    close(torch.stack(outs["epi_res_layers"]).squeeze(2), fx.t(case + "_epi_res_layers"), F32_STORED, "epi_res_layers")
    losses, E_layers, pose, loss_qt = losses_of(oracle, outs, sc)
    close(torch.stack(losses["loss_layers"]), fx.t(case + "_loss_layers"), F64, "loss_layers")
    close(losses["loss_F"], fx.t(case + "_loss_F"), F64, "loss_F")
    close(torch.stack(E_layers), fx.t(case + "_E_layers"), F64, "E_layers")
    close(pose["q_l2"], fx.t(case + "_q_l2_layers"), F64, "q_l2")
    close(pose["t_l2"], fx.t(case + "_t_l2_layers"), F64, "t_l2")
    close(loss_qt, fx.t(case + "_loss_qt"), F64, "loss_qt")


@pytest.mark.parametrize("case", sorted(rf.CASES))
def test_oracle_autograd_reproduces_the_reference_logit_gradients(dfepe, oracle, fx, monkeypatch, case):
    """d loss / d logits of EVERY layer, both objectives.  The gradient at layer l also flows through the later estimator calls, so the
    oracle's recurrent loop runs with the stock mirror as its two estimators (float64, the fixture's parameters): this is the whole model
    on the CPU, and it must land on the fixture's logits, losses and logit gradients."""
    sc = scene(fx, case)
    net = mirror(dfepe, fx)
    gauged_fit(oracle, monkeypatch, fx.t(case + "_out_layers"))
    outs = oracle.deepf_forward(sc["matches_xy_ori"], rf.IMAGE_SIZE, rf.DEPTH, input_weights=net.input_weights, update_weights=net.update_weights)
    logits = outs["logits_layers"]
    close(torch.stack(logits).squeeze(2).detach(), fx.t(case + "_logits_layers"), F64, "logits_layers")
    losses, _, _, loss_qt = losses_of(oracle, outs, sc)
    close(losses["loss_F"].detach(), fx.t(case + "_loss_F"), F64, "loss_F")
    close(loss_qt.detach(), fx.t(case + "_loss_qt"), F64, "loss_qt")
    for tag, loss in (("F", losses["loss_F"]), ("qt", loss_qt)):
        g = torch.autograd.grad(loss, logits, retain_graph=True)
        close(torch.stack(g).squeeze(2), fx.t(f"{case}_dlogits_{tag}"), F32_STORED, "d loss_" + tag + " / d logits")


@pytest.mark.parametrize("case", sorted(rf.CASES))
def test_stock_mirror_reproduces_the_reference_logits_layer_by_layer(dfepe, oracle, fx, monkeypatch, case):
    """compat.ErrorEstimators.ErrorEstimator in float64 with the fixture's parameters: ``input_weights`` on the point channels as
    oracle.estimator_input builds them from the fixture's matches, ``update_weights`` on those channels + the previous layer's weights /
    epi_res / residual in the order of deepFEPE/models/DeepFNet.py:487, reproduce the fixture's logits of every layer to 1e-9.
    The fixture keeps epi_res and residual as float32 roundings (6e-8 relative: more than the 1e-9 held here), so the two channels
    are the oracle's float64 values from the fixture's float64 logits, first checked against the stored roundings."""
    sc = scene(fx, case)
    net = mirror(dfepe, fx)
    assert sorted(net.state_dict().keys()) == [str(k) for k in fx[case + "_state_keys"]]
    chk = np.array([float(p.detach().abs().sum()) for _, p in sorted(net.named_parameters())])
    np.testing.assert_allclose(chk, fx[case + "_param_checksum"], rtol=1e-12)
    gauged_fit(oracle, monkeypatch, fx.t(case + "_out_layers"))
    truth = fx.t(case + "_logits_layers")
    outs = oracle.deepf_forward(sc["matches_xy_ori"], rf.IMAGE_SIZE, rf.DEPTH, logits_layers=truth)
    close(torch.stack(outs["residual_layers"]), fx.t(case + "_residual_layers"), F32_STORED, "residual_layers")
    close(torch.stack(outs["epi_res_layers"]).squeeze(2), fx.t(case + "_epi_res_layers"), F32_STORED, "epi_res_layers")
    pts_in = oracle.estimator_input(outs["pts1"], outs["pts2"])
    weights = fx.weights(case)
    with torch.no_grad():
        got = [net.input_weights(pts_in)]
        for l in range(rf.DEPTH - 1):
            net_in = torch.cat((pts_in, weights[l].unsqueeze(1), outs["epi_res_layers"][l], outs["residual_layers"][l].unsqueeze(1)), 1)
            got.append(net.update_weights(net_in))
    for l in range(rf.DEPTH):
        d = float((got[l].squeeze(1) - truth[l]).abs().max())
        assert d <= 1e-9, (l, d)


def test_fixture_integrity(fx):
    """The recorded head is the largest of the candidates at which the reference's float32 run meets the caps, the caps are the issue's,
    and every recorded distance of that run sits within its cap."""
    assert float(fx["head"]) == 0.2 and [float(h) for h in fx["heads_tried"]] == [0.5, 0.2, 0.1, 0.05]
    assert (float(fx["cap_logits"]), float(fx["cap_unitF"]), float(fx["cap_grad"])) == (2e-4, 2e-5, 1e-2)
    assert int(fx["depth"]) == rf.DEPTH and int(fx["scene_seed"]) == 31 and int(fx["param_seed"]) == 5
    for case, (B, N) in rf.CASES.items():
        assert fx[case + "_logits_layers"].shape == (rf.DEPTH, B, N) and fx[case + "_logits_layers"].dtype == np.float64
        assert fx[case + "_matches_xy_ori"].dtype == np.float32
        assert fx[case + "_ref32_dist_logits_layers"].max() <= 2e-4
        assert fx[case + "_ref32_dist_unitF_layers"].max() <= 2e-5
        for tag in ("F", "qt"):
            d = fx[f"{case}_ref32_dist_grad_{tag}"]
            assert d.shape == (44,) and d.max() <= 1e-2
            assert fx[f"{case}_grad_norms_{tag}"].shape == (44,) and fx[f"{case}_grad_proj_{tag}"].shape == (44, 4)
        for k in ("weights_layers", "residual_layers", "epi_res_layers", "dlogits_F", "dlogits_qt", "loss_layers", "loss_F", "loss_qt",
                  "q_l2_layers", "t_l2_layers"):
            assert np.isfinite(fx[f"{case}_ref32_dist_{k}"]).all(), k
    if "n1000_adam_loss_steps" in fx:
        l64 = fx["n1000_adam_loss_steps"]
        assert l64.shape == (3,) and float(fx["n1000_adam_head"]) == 0.05
        assert (fx["n1000_adam_ref32_dist_loss_steps"] <= float(fx["adam_cap"]) * np.abs(l64)).all() and float(fx["adam_cap"]) == 1e-5
