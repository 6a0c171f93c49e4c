"""dfepe_sample_sets on the GPU: every shared case of tests/sampler_cases.py through the C ABI and the same check() as the host build
(equality with the restatement tests/sampler_ref.py), bit-identity over runs, independence of a pair's sets from the batch and the
number of hypotheses, the workspace refusal, and one hipGraph capture of compat.DeviceSampler.draw that draws the next offset on
every replay.  GPU box only."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_cases as sc  # noqa: E402
import sampler_ref as sr  # noqa: E402

DEV = "cuda:0"


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


def run_abi(dfepe, case, ws_offset=0, expect=0):
    B, H, N, S = case["B"], case["H"], case["N"], case["S"]
    L = dfepe._lib.lib()
    w, nv = _dev(case["weights"]), _dev(case["n_valid"])
    ctr = None if case["counter"] is None else torch.tensor([case["counter"]], dtype=torch.uint32).to(DEV)
    idx = torch.full((B, H, S), -1, device=DEV, dtype=torch.int32)
    fb = torch.full((B,), -1, device=DEV, dtype=torch.int32)
    ws = None
    if w is not None:
        nbytes = L.dfepe_sample_sets_workspace_bytes(B, N, 1)
        assert nbytes == (B * (N + 2) * 8 + 15) // 16 * 16
        ws = torch.full((nbytes // 8 + 2,), -1, device=DEV, dtype=torch.int64)
        assert ws.data_ptr() % 16 == 0
    rc = L.dfepe_sample_sets(torch.cuda.current_stream().cuda_stream, B, N, H, S, case["seed"], case["offset"], _ptr(ctr), _ptr(w), _ptr(nv),
                             _ptr(idx), _ptr(fb), None if ws is None else ws.data_ptr() + ws_offset, )
    assert rc == expect, rc
    torch.cuda.synchronize()
    if ctr is not None:
        assert int(ctr.item()) == case["counter"]  # read, not written
    return idx.cpu().numpy(), fb.cpu().numpy()


def test_uniform_cases_through_the_c_abi(dfepe):
    for case in sc.uniform_cases():
        sc.check(*run_abi(dfepe, case), case)


def test_weighted_cases_through_the_c_abi(dfepe):
    chunk = dfepe._lib.lib().dfepe_sampler_scan_chunk()
    for case in sc.weighted_cases(chunk):
        sc.check(*run_abi(dfepe, case), case)


def test_two_runs_give_the_same_bits(dfepe):
    chunk = dfepe._lib.lib().dfepe_sampler_scan_chunk()
    cases = sc.weighted_cases(chunk)
    for case in (sc.uniform_cases()[20], cases[3], cases[-5]):
        a, b = run_abi(dfepe, case), run_abi(dfepe, case)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), case["name"]


def test_a_pairs_sets_do_not_depend_on_the_batch_or_on_h(dfepe):
    rng = np.random.default_rng(5)
    w = (rng.random((4, 300)) ** 4 + 1e-3).astype(np.float32)
    nv = torch.tensor([300, 150, 12, 299], dtype=torch.int32, device=DEV)
    for weights in (None, _dev(w)):
        kw = dict(seed=99, offset=3)
        small = dfepe.ops.sample_sets(2, 300, 5, 12, weights=None if weights is None else weights[:2].contiguous(), n_valid=nv[:2].contiguous(), device=DEV, **kw)
        large = dfepe.ops.sample_sets(4, 300, 70, 12, weights=weights, n_valid=nv, device=DEV, **kw)
        assert small.shape == (2, 5, 12) and large.shape == (4, 70, 12) and small.dtype == torch.int32
        assert torch.equal(small, large[:2, :5])
        ref, _, _ = sr.sample_sets(4, 300, 70, 12, 99, 3, None, None if weights is None else w, nv.cpu().numpy(), pairs=(1, 3), hyps=(4, 69))
        got = large.cpu().numpy()
        for b in (1, 3):
            for h in (4, 69):
                assert np.array_equal(got[b, h], ref[b, h])


def test_a_misaligned_workspace_is_refused(dfepe):
    case = sc.weighted_cases(dfepe._lib.lib().dfepe_sampler_scan_chunk())[0]
    idx, fb = run_abi(dfepe, case, ws_offset=8, expect=-1)
    assert (idx == -1).all() and (fb == -1).all()  # nothing was launched


def test_fallback_output_and_python_layer(dfepe):
    w = torch.zeros(3, 30, device=DEV)
    w[0, :12] = 1.0
    w[1, :9] = 1.0      # nine drawable: falls back
    w[2] = 1.0
    idx, fb = dfepe.ops.sample_sets(3, 30, 7, seed=1, weights=w, want_fallback=True)
    assert fb.tolist() == [0, 1, 0] and int(idx[0].max()) < 12 and idx.shape == (3, 7, 10)
    idx_u, fb_u = dfepe.ops.sample_sets(3, 30, 7, seed=1, device=DEV, want_fallback=True)
    assert fb_u.tolist() == [0, 0, 0] and torch.equal(idx_u[1], idx[1])     # the fallen-back pair is the uniform draw
    assert dfepe.ops.sample_sets(0, 30, 7, seed=1, device=DEV).shape == (0, 7, 10)


def test_one_captured_draw_advances_on_every_replay(dfepe):
    B, N, H, S, seed, c = 3, 50, 70, 10, 0x1234567887654321, 0xfffffffe  # the counter wraps during the replays
    sampler = dfepe.compat.DeviceSampler(seed, DEV)
    assert sampler.counter.dtype == torch.uint32 and sampler.counter.is_cuda and int(sampler.counter.item()) == 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            sampler.draw(B, N, H, S)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert int(sampler.counter.item()) == 2
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = sampler.draw(B, N, H, S)
    sampler.counter.copy_(torch.tensor([c], dtype=torch.uint32))
    got = []
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        got.append(out.cpu().numpy().copy())
    for k in range(3):
        ref, _, _ = sr.sample_sets(B, N, H, S, seed, 0, (c + k) & 0xffffffff)
        assert np.array_equal(got[k], ref), k
    assert int(sampler.counter.item()) == (c + 3) & 0xffffffff
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])
