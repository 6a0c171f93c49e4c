"""compat.dsac with a DeviceSampler on the GPU: dsac_batch and DSAC draw their minimal sets on the stream (ops.sample_sets) and
compute exactly what the same idx handed in computes; weights steer the draw; the host draw stays the default, bit for bit; and one
captured forward + backward draws fresh hypotheses on every replay.  GPU box only."""
import os
import random
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dsac_cases as dc  # noqa: E402

DEV = "cuda:0"
B, N = 2, 64
THRESH, BETA, ALPHA = dc.THRESH, dc.BETA, dc.ALPHA


@pytest.fixture(scope="module")
def pts():
    X, Y, K = dc.scene(B, N, seed=31)
    return tuple(torch.from_numpy(a).to(DEV) for a in (X, Y, K))


def _step(dfepe, X, Y, K, H, **kw):
    X, Y = X.clone().requires_grad_(), Y.clone().requires_grad_()
    out = dfepe.compat.dsac_batch(X, Y, K, H, THRESH, BETA, ALPHA, loss_kind=1, **kw)
    gX, gY = torch.autograd.grad(out["exp_loss"].sum() + out["quality"].sum(), (X, Y))
    return {k: v.detach() for k, v in out.items()}, gX, gY


@pytest.mark.parametrize("H", [5, 65])
def test_dsac_batch_with_a_device_sampler_is_dsac_batch_with_that_idx(dfepe, pts, H):
    X, Y, K = pts
    sampler = dfepe.compat.DeviceSampler(7, DEV)
    out, gX, gY = _step(dfepe, X, Y, K, H, sampler=sampler)
    idx = dfepe.ops.sample_sets(B, N, H, 10, seed=7, offset=0, device=DEV)
    assert out["idx"].is_cuda and out["idx"].dtype == torch.int32 and torch.equal(out["idx"], idx)
    assert int(sampler.counter.item()) == 1
    ref, rX, rY = _step(dfepe, X, Y, K, H, idx=idx)
    assert set(ref) == set(out)
    for k in ref:
        assert torch.equal(out[k], ref[k]), k
    assert torch.equal(gX, rX) and torch.equal(gY, rY)
    nxt = dfepe.compat.dsac_batch(X, Y, K, H, THRESH, BETA, ALPHA, sampler=sampler)["idx"]   # the second draw: offset 1
    assert torch.equal(nxt, dfepe.ops.sample_sets(B, N, H, 10, seed=7, offset=1, device=DEV)) and not torch.equal(nxt, idx)


def test_weights_steer_the_draw(dfepe, pts):
    X, Y, K = pts
    w = torch.zeros(B, N, device=DEV)
    keep = torch.zeros(B, N, dtype=torch.bool, device=DEV)
    g = torch.Generator().manual_seed(3)
    for b in range(B):
        keep[b, torch.randperm(N, generator=g)[:20].to(DEV)] = True
    w[keep] = torch.rand(int(keep.sum()), generator=g).to(DEV) + 0.05
    out = dfepe.compat.dsac_batch(X, Y, K, 65, THRESH, BETA, ALPHA, sampler=dfepe.compat.DeviceSampler(11, DEV), weights=w)
    assert (out["counts"][~keep] == 0).all() and (out["counts"][keep] > 0).all()   # 65 x 10 draws over 20: none stays undrawn
    nv = torch.tensor([12, 64], dtype=torch.int32, device=DEV)
    out = dfepe.compat.dsac_batch(X, Y, K, 65, THRESH, BETA, ALPHA, sampler=dfepe.compat.DeviceSampler(11, DEV), n_valid=nv)
    assert (out["counts"][0, 12:] == 0).all() and (out["counts"][0, :12] > 0).all() and out["counts"][1, 12:].sum() > 0


def test_weights_or_n_valid_without_a_sampler_raise(dfepe, pts):
    X, Y, K = pts
    with pytest.raises(ValueError):
        dfepe.compat.dsac_batch(X, Y, K, 5, THRESH, BETA, ALPHA, weights=torch.ones(B, N, device=DEV))
    with pytest.raises(ValueError):
        dfepe.compat.dsac_batch(X, Y, K, 5, THRESH, BETA, ALPHA, n_valid=torch.full((B,), 20, dtype=torch.int32, device=DEV))


def test_the_host_draw_stays_the_default(dfepe, pts):
    X, Y, K = pts
    H = 5
    rng = random.Random(0)
    want = [[rng.sample(range(N), 10) for _ in range(H)] for _ in range(B)]
    out = dfepe.compat.dsac_batch(X, Y, K, H, THRESH, BETA, ALPHA, seed=0)
    assert out["idx"].cpu().tolist() == want
    d = dfepe.compat.DSAC(H, THRESH, BETA, ALPHA, K[0], dfepe.compat.H_loss.HLoss())
    random.seed(0)
    d.expected_loss(X[0], Y[0])
    assert d.best_corres_idx == want[0][d.best_H_idx]          # random.seed(0) and random.Random(0) are one sequence
    random.seed(0)
    d(X[0], Y[0])
    assert d.best_corres_idx == want[0][d.best_H_idx]


@pytest.mark.parametrize("H", [5, 65])
def test_dsac_class_with_a_device_sampler(dfepe, pts, H):
    X, Y, K = pts
    d = dfepe.compat.DSAC(H, THRESH, BETA, ALPHA, K[0], dfepe.compat.H_loss.HLoss(), sampler=dfepe.compat.DeviceSampler(21, DEV))
    idx0 = dfepe.ops.sample_sets(1, N, H, 10, seed=21, offset=0, device=DEV)[0]
    idx1 = dfepe.ops.sample_sets(1, N, H, 10, seed=21, offset=1, device=DEV)[0]
    Xg = X[0].clone().requires_grad_()
    exp_loss, top_loss = d.expected_loss(Xg, Y[0])
    assert d.best_H_idx >= 0 and d.best_corres_idx == idx0[d.best_H_idx].tolist()
    ref = dfepe.ops.dsac(X[:1], Y[:1], K[:1], idx0[None], THRESH, BETA, ALPHA, loss_kind=1)
    assert torch.equal(exp_loss.detach(), ref["exp_loss"][0]) and d.best_H_idx == int(ref["best"][0])
    (g,) = torch.autograd.grad(exp_loss, Xg)
    assert torch.isfinite(g).all() and g.abs().sum() > 0
    q = d(X[0], Y[0])                                           # the reference's call: the sampler's second draw
    assert q.shape == (N, 1) and not q.is_cuda and d.best_corres_idx == idx1[d.best_H_idx].tolist()


def test_one_captured_step_draws_fresh_hypotheses_on_every_replay(dfepe, pts):
    X0, Y0, K = pts
    H, c = 5, 40
    X, Y = X0.clone().requires_grad_(), Y0.clone().requires_grad_()
    sampler = dfepe.compat.DeviceSampler(13, DEV)
    gx, gy = torch.zeros_like(X), torch.zeros_like(Y)
    state = {}

    def step():
        out = dfepe.compat.dsac_batch(X, Y, K, H, THRESH, BETA, ALPHA, loss_kind=1, sampler=sampler)
        a, b = torch.autograd.grad(out["exp_loss"].sum() + out["quality"].sum(), (X, Y))
        gx.copy_(a)
        gy.copy_(b)
        state["out"] = {k: v.detach() for k, v in out.items()}

    def snapshot():
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in state["out"].items()}, gx.clone(), gy.clone()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    captured = state["out"]
    sampler.counter.copy_(torch.tensor([c], dtype=torch.uint32))
    replays = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        replays.append(({k: v.clone() for k, v in captured.items()}, gx.clone(), gy.clone()))
    assert int(sampler.counter.item()) == c + 2
    assert not torch.equal(replays[0][0]["idx"], replays[1][0]["idx"])
    sampler.counter.copy_(torch.tensor([c], dtype=torch.uint32))
    for k, (outs, rx, ry) in enumerate(replays):
        step()
        eager, ex, ey = snapshot()
        assert torch.equal(outs["idx"], dfepe.ops.sample_sets(B, N, H, 10, seed=13, offset=c + k, device=DEV))
        for name, v in eager.items():
            assert torch.equal(outs[name], v), (k, name)
        assert torch.equal(rx, ex) and torch.equal(ry, ey), k
