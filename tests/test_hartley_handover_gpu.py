"""The Hartley record of the forward fit on the GPU (tests/test_hartley_handover_cpu.py states what it is): a launch that writes
the record, launches that read it and plain launches give the same bytes in every output, at the launch level on every rung, through
pipeline.hot_path_fused (eager and as replays of a captured graph) and through the recurrent compat.DeepFNet.  GPU box only."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IMAGE_SIZE = [376, 1241, 3]
H, W = float(IMAGE_SIZE[0]), float(IMAGE_SIZE[1])
RAW, LOGITS = 1, 2


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b, what):
    for k, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None), (what, k)
        if x is not None:
            assert torch.equal(_bits(x), _bits(y)), f"{what}: output {k} differs in {int((_bits(x) != _bits(y)).sum())} words"


def _inputs(B, N, seed, raw=True):
    g = torch.Generator().manual_seed(seed)
    if raw:
        p1 = (torch.rand(B, N, 4, generator=g) * torch.tensor([W, H, W, H])).to(DEV)
        p2 = None
    else:
        p1 = torch.cat((torch.rand(B, N, 2, generator=g) * 2 - 1, torch.ones(B, N, 1)), 2).contiguous().to(DEV)
        p2 = torch.cat((torch.rand(B, N, 2, generator=g) * 2 - 1, torch.ones(B, N, 1)), 2).contiguous().to(DEV)
    return p1, p2, torch.randn(B, N, generator=g).to(DEV), torch.randn(B, N, generator=g).to(DEV)


def _fwd(dfepe, p1, p2, w, raw, logits, hartley=None):
    return dfepe.ops.w8pt_forward(p1, p2, w, raw, W, H, 0.5, want_epi=True, want_save=True, logits=logits, hartley=hartley)


def _three_modes(dfepe, B, N, seed, raw=True, logits=True):
    p1, p2, w1, w2 = _inputs(B, N, seed, raw)
    if not logits:
        w1, w2 = w1.abs() + 0.05, w2.abs() + 0.05
    L = dfepe._lib
    record = torch.full((B, L.HARTLEY_DOUBLES), 3.0, dtype=torch.float64, device=DEV)
    plain1, plain2 = _fwd(dfepe, p1, p2, w1, raw, logits), _fwd(dfepe, p1, p2, w2, raw, logits)
    wrote = _fwd(dfepe, p1, p2, w1, raw, logits, (record, L.HARTLEY_WRITE))
    read = _fwd(dfepe, p1, p2, w2, raw, logits, (record, L.HARTLEY_READ))
    torch.cuda.synchronize()
    assert torch.isfinite(plain1[0]).all() and torch.isfinite(plain2[0]).all()
    _same(wrote, plain1, f"write B={B} N={N}")
    _same(read, plain2, f"read B={B} N={N}")
    assert (record[:, 6] == 0).all() and (record[:, 7] != 0).all() and torch.isfinite(record).all()
    return record


@pytest.mark.parametrize("B", [1, 17, 100])
@pytest.mark.parametrize("N", [8, 17, 100, 113, 128])
def test_write_read_and_plain_launches_give_the_same_bytes(dfepe, B, N):
    """Every correspondences-per-lane rung (1, 2, 7, 8, 8), one pair, a ragged last workgroup (17) and several workgroups (100): F,
    residual, epipolar residual, softmax weights and the 128 floats of the save record."""
    _three_modes(dfepe, B, N, seed=100 * N + B)


def test_homogeneous_points_and_plain_weights(dfepe):
    _three_modes(dfepe, 17, 100, seed=7, raw=False, logits=False)
    _three_modes(dfepe, 17, 33, seed=8, raw=False, logits=True)


def test_lean_launch(dfepe):
    """12 291 pairs at N = 100: over kLeanMinPairs (12 288), so the <= 256-register build runs, with a ragged last workgroup."""
    _three_modes(dfepe, 12291, 100, seed=11)


def test_three_weight_sets_read_one_record(dfepe):
    """n_weight_sets = 3 in read mode: the record is indexed by pair % B, like the correspondences."""
    B, N, S = 17, 100, 3
    lib, L = dfepe._lib.lib(), dfepe._lib
    p1, _, w1, _ = _inputs(B, N, seed=21)
    w = torch.randn(S, B, N, generator=torch.Generator().manual_seed(22)).to(DEV)
    record = torch.zeros(B, L.HARTLEY_DOUBLES, dtype=torch.float64, device=DEV)
    _fwd(dfepe, p1, None, w1, True, True, (record, L.HARTLEY_WRITE))

    def run(mode):
        outs = [torch.empty(S * B, 9, device=DEV), torch.empty(S * B, N, device=DEV), torch.empty(S * B, N, device=DEV),
                torch.empty(S * B, 128, device=DEV), torch.empty(S * B, N, device=DEV)]
        rc = lib.dfepe_w8pt_fwd_shared(p1.data_ptr(), None, w.data_ptr(), B, N, S, RAW | LOGITS, W, H, 0.5, outs[0].data_ptr(),
                                       outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), outs[4].data_ptr(),
                                       record.data_ptr(), mode, dfepe.ops._stream())
        assert rc == 0
        return outs

    plain, read = run(L.HARTLEY_NONE), run(L.HARTLEY_READ)
    torch.cuda.synchronize()
    assert torch.isfinite(plain[0]).all()
    _same(read, plain, "read, three weight sets")


def test_a_record_nobody_wrote_poisons_the_fit_and_faults_nothing(dfepe):
    """A zero-filled record is valid memory with a wrong tag: F and the residual come out NaN (the epipolar residual is a minimum with
    the clamp, which drops the NaN), nothing faults, and the next launch is fine."""
    B, N = 17, 100
    L = dfepe._lib
    p1, _, w1, _ = _inputs(B, N, seed=31)
    F, res, epi, _, _ = _fwd(dfepe, p1, None, w1, True, True, (torch.zeros(B, L.HARTLEY_DOUBLES, dtype=torch.float64, device=DEV), L.HARTLEY_READ))
    torch.cuda.synchronize()
    assert torch.isnan(F).all() and torch.isnan(res).all() and (torch.isnan(epi) | (epi == 0.5)).all()
    assert torch.isfinite(_fwd(dfepe, p1, None, w1, True, True)[0]).all()


def _hw_T():  # given to hot_path_fused, which would otherwise build it from host values: not capturable
    return torch.tensor([[2.0 / W, 0.0, -1.0], [0.0, 2.0 / H, -1.0], [0.0, 0.0, 1.0]], device=DEV)


def _hot_path(dfepe, sc, depth, share, hw_T):
    logits = sc["logits_layers"][:depth].detach().clone().requires_grad_(True)
    o = dfepe.pipeline.hot_path_fused(sc["matches_xy_ori"], logits, sc["Ks"], sc["pts1_virt_ori"], sc["pts2_virt_ori"], sc["qs_cam"],
                                      sc["ts_cam"], sc["R_gt"], IMAGE_SIZE, 0.02, True, hw_T=hw_T, share_hartley=share)
    grad, = torch.autograd.grad(o["loss"], logits)
    flat = {}
    for k, v in o.items():
        if isinstance(v, (list, tuple)):
            flat.update({f"{k}[{i}]": x for i, x in enumerate(v)})
        else:
            flat[k] = v
    flat["grad_logits"] = grad
    return flat


def _same_dict(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        x, y = a[k].detach().reshape(-1).contiguous(), b[k].detach().reshape(-1).contiguous()
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), f"{what}: {k} differs"


def test_hot_path_fused_with_and_without_sharing_eager(dfepe):
    B, N, depth = 48, 100, 3
    sc = dfepe.pipeline.scene_to_device(dfepe.synth.make_scene(B, N, seed=41, outlier_ratio=0.2, depth_layers=depth), DEV)
    hw_T = _hw_T()
    a, b = _hot_path(dfepe, sc, depth, True, hw_T), _hot_path(dfepe, sc, depth, False, hw_T)
    torch.cuda.synchronize()
    assert torch.isfinite(a["grad_logits"]).all() and torch.isfinite(a["F_layers"]).all()
    _same_dict(a, b, "eager")


def test_hot_path_fused_with_and_without_sharing_captured(dfepe):
    """The step captured once per setting and replayed three times: every replay of the sharing graph equals every replay of the
    other, in every returned array and in grad_logits (the graph owns its record: it comes from the capture's pool)."""
    B, N, depth = 48, 100, 3
    sc = dfepe.pipeline.scene_to_device(dfepe.synth.make_scene(B, N, seed=42, outlier_ratio=0.2, depth_layers=depth), DEV)
    replays, hw_T = {}, _hw_T()
    for share in (True, False):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                _hot_path(dfepe, sc, depth, share, hw_T)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode=dfepe.dist.graph_capture_mode()):
            static = _hot_path(dfepe, sc, depth, share, hw_T)
        got = []
        for _ in range(3):
            for v in static.values():
                v.detach().zero_()
            graph.replay()
            torch.cuda.synchronize()
            got.append({k: v.detach().clone() for k, v in static.items()})
        replays[share] = got
    assert torch.isfinite(replays[True][0]["grad_logits"]).all() and replays[True][0]["grad_logits"].abs().max() > 0
    for r in range(3):
        _same_dict(replays[True][r], replays[False][r], f"replay {r}")
        _same_dict(replays[True][r], replays[True][0], f"replay {r} vs replay 0")


def test_deepfnet_with_and_without_sharing(dfepe):
    """The recurrent model (no learned offsets: every layer fits the same matches) at B = 4, N = 100, depth 3 with fixed seeds: outputs
    and parameter gradients are the same bytes with and without the record."""
    B, N, depth = 4, 100, 3
    sc = dfepe.synth.make_scene(B, N, seed=51, outlier_ratio=0.2, noise_px=0.5)
    batch = {"matches_xy_ori": sc["matches_xy_ori"].to(DEV), "matches_good_unique_nums": None, "t_scene_scale": None}
    results = []
    for share in (True, False):
        net = dfepe.compat.DeepFNet.DeepFNet(depth=depth, image_size=IMAGE_SIZE, if_quality=False, share_hartley=share).to(DEV)
        dfepe.synth.fill_params_deterministic(net, 3)
        assert net.share_hartley == share
        outs = net(batch)
        loss = sum((F ** 2).sum() for F in outs["out_layers"]) + sum(r.abs().sum() for r in outs["residual_layers"]) + outs["weights"].square().sum()
        loss.backward()
        torch.cuda.synchronize()
        arrays = {"loss": loss.detach(), "logits": outs["logits"].detach(), "F_est": outs["F_est"].detach(), "weights": outs["weights"].detach()}
        for k in ("out_layers", "residual_layers", "epi_res_layers", "weights_layers", "logits_layers"):
            arrays.update({f"{k}[{i}]": x.detach() for i, x in enumerate(outs[k])})
        grads = {n: p.grad.detach() for n, p in net.named_parameters() if p.grad is not None}
        assert len(grads) > 0 and all(torch.isfinite(g).all() for g in grads.values())
        results.append((arrays, grads))
    _same_dict(results[0][0], results[1][0], "outputs")
    _same_dict(results[0][1], results[1][1], "parameter gradients")
    assert float(np.max([g.abs().max().item() for g in results[0][1].values()])) > 0
