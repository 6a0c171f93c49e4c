"""dfepe_dsac_bwd on the GPU: every shared case and edge of tests/dsac_adjoint_cases.py through its check() against the fp64
restatement (tests/dsac_adjoint_ref.py), via the C ABI with the stage totals requested; autograd through ops.dsac; the reference's own
float64 gradient (tests/golden/dsac_adjoint.npz) through compat.DSAC.expected_loss and compat.dsac_batch; bit-identity; and one
hipGraph capture of forward + backward.  GPU box only."""
import os
import random
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dsac_adjoint_cases as ac  # noqa: E402

DEV = "cuda:0"
F32 = np.float32
CASES = ac.all_cases()
FWD_KEYS = ("E_sample", "soft", "score", "E_refit", "loss", "counts")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


def forward(dfepe, case):
    with torch.no_grad():
        return dfepe.ops.dsac(_dev(case["X"]), _dev(case["Y"]), _dev(case["K"]), _dev(case["idx"]), case["thresh"], case["beta"],
                              case["alpha"], loss_kind=case["loss_kind"])


def run_abi(dfepe, case, fwd=None, totals=True, want_x=True, want_y=True, up=None):
    """dfepe_dsac_bwd through the C ABI on the kernel's own forward -> (fwd, got) as check() takes them (numpy), the fit adjoints'
    point gradients read out of the workspace by its documented layout."""
    B, N, H, S = case["B"], case["N"], case["H"], case["S"]
    L = dfepe._lib.lib()
    X, Y, K, idx = (_dev(case[k]) for k in ("X", "Y", "K", "idx"))
    fwd = forward(dfepe, case) if fwd is None else fwd
    up = {k: _dev(v) for k, v in (ac.upstreams(case) if up is None else up).items()}
    z = lambda *s: torch.full(s, float("nan"), device=DEV)  # noqa: E731
    t = {"t_score": z(B, H), "t_loss": z(B, H), "t_E_refit": z(B, H, 3, 3), "t_w": z(H, B, N), "t_E_sample": z(B, H, 3, 3)} if totals else {}
    gX, gY = (z(B, N, 2) if want_x else None), (z(B, N, 2) if want_y else None)
    floats, off = ac.workspace_floats(B, N, H, S)
    assert L.dfepe_dsac_bwd_workspace_bytes(B, N, H, S) == 4 * floats
    ws = torch.zeros(floats, device=DEV)
    rc = L.dfepe_dsac_bwd(torch.cuda.current_stream().cuda_stream, _ptr(X), _ptr(Y), _ptr(K), _ptr(idx), B, N, H, S, case["thresh"],
                          case["beta"], case["alpha"], case["loss_kind"], *(_ptr(fwd[k]) for k in FWD_KEYS),
                          *(_ptr(up.get(k)) for k in ac.ALL_UP), _ptr(gX), _ptr(gY),
                          *(_ptr(t.get(k)) for k in ac.TOTALS), _ptr(ws))
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in t.items()}
    got["g_X"], got["g_Y"] = (None if gX is None else gX.cpu().numpy()), (None if gY is None else gY.cpu().numpy())
    w = ws.cpu().numpy()
    for name, shape in (("gpn1", (B, N, 2)), ("gpn2", (B, N, 2)), ("gg1", (B, H, S, 2)), ("gg2", (B, H, S, 2))):
        got[name] = w[off[name]:off[name] + int(np.prod(shape))].reshape(shape).copy()
    return {k: fwd[k].cpu().numpy() for k in FWD_KEYS}, got


def _case(name, up=None):
    return next(c for c in CASES if c["name"] == name and (up is None or c["up"] == up))


@pytest.mark.parametrize("k", range(len(CASES)), ids=[ac.name_of(c) for c in CASES])
def test_case_passes_the_check(dfepe, k):
    case = CASES[k]
    fwd, got = run_abi(dfepe, case)
    ac.check(case, fwd, got)


def test_autograd_through_ops_equals_the_c_call(dfepe):
    """ops.dsac(...)["exp_loss"].sum().backward(), and the same for quality, populate X.grad and Y.grad with what the C call writes
    for that one upstream of ones."""
    case = CASES[4]
    B, N = case["B"], case["N"]
    for name, shape in (("exp_loss", (B,)), ("quality", (B, N))):
        X, Y = _dev(case["X"]).requires_grad_(), _dev(case["Y"]).requires_grad_()
        out = dfepe.ops.dsac(X, Y, _dev(case["K"]), _dev(case["idx"]), case["thresh"], case["beta"], case["alpha"], loss_kind=case["loss_kind"])
        assert out[name].grad_fn is not None and out["E_refit"].requires_grad and out["score"].requires_grad
        for key in ("soft", "sampson", "counts", "best", "top_loss"):
            assert not out[key].requires_grad, key
        out[name].sum().backward()
        torch.cuda.synchronize()
        _, got = run_abi(dfepe, case, totals=False, up={name: np.ones(shape, F32)})
        assert np.array_equal(X.grad.cpu().numpy(), got["g_X"]) and np.array_equal(Y.grad.cpu().numpy(), got["g_Y"]), name
        assert np.isfinite(got["g_X"]).all() and np.abs(got["g_X"]).max() > 0
    # only X requires grad: Y gets none, X's is unchanged; and with nothing requiring grad there is no graph and the same bits
    X = _dev(case["X"]).requires_grad_()
    out = dfepe.ops.dsac(X, _dev(case["Y"]), _dev(case["K"]), _dev(case["idx"]), case["thresh"], case["beta"], case["alpha"],
                         loss_kind=case["loss_kind"], want=())
    assert set(out) == {"E_sample", "score", "E_refit", "loss", "quality", "counts", "best"}
    out["quality"].sum().backward()
    assert np.array_equal(X.grad.cpu().numpy(), got["g_X"])
    plain = forward(dfepe, case)
    assert all(v.grad_fn is None for v in plain.values())
    for k, v in out.items():
        assert torch.equal(v.detach(), plain[k]), k


def _pin(ours, truth, yard, what):
    dist, bound = float(np.abs(ours - truth).max()), max(4 * yard, 1e-6 * float(np.abs(truth).max()))
    print(f"{what}: distance {dist:.3g}, reference's float32 {yard:.3g}, bound {bound:.3g}, ratio to the yardstick {dist / yard:.3g}")
    assert dist <= bound, (what, dist, bound)
    return dist / yard


def test_golden_pin_through_the_mirror(dfepe, golden):
    """compat.DSAC.expected_loss and compat.dsac_batch, seeded like the reference's run, against the reference's float64 gradients:
    within max(4 x the reference's own float32 distance, 1e-6 of the largest entry), the rule of the forward's pin.  On the case where
    the reference's gradient is not finite, ours is, and equals the restatement (check())."""
    g = golden("dsac_adjoint")
    n = int(g["n_cases"])
    worst = 0.0
    for k in range(n):
        X, Y, K, idx = g[f"{k}_X"], g[f"{k}_Y"], g[f"{k}_K"], g[f"{k}_idx"]
        thresh, beta, alpha, hyps = float(g[f"{k}_thresh"]), float(g[f"{k}_beta"]), float(g[f"{k}_alpha"]), int(g[f"{k}_hyps"])
        d = dfepe.compat.DSAC(hyps, thresh, beta, alpha, torch.from_numpy(K), dfepe.compat.H_loss.HLoss())
        Xt, Yt = _dev(X).requires_grad_(), _dev(Y).requires_grad_()
        random.seed(int(g[f"{k}_seed"]))
        exp_loss, top_loss = d.expected_loss(Xt, Yt)
        assert exp_loss.is_cuda and exp_loss.dim() == 0 and exp_loss.grad_fn is not None and not top_loss.requires_grad
        assert tuple(d.quality.shape) == (len(X), 1) and d.quality.is_cuda and d.quality.grad_fn is not None
        assert d.best_corres_idx == idx[d.best_H_idx].tolist()
        ge = torch.autograd.grad(exp_loss, (Xt, Yt), retain_graph=True)
        gq = torch.autograd.grad((_dev(g[f"{k}_c"]) * d.quality[:, 0]).sum(), (Xt, Yt))
        Xb, Yb = _dev(X[None]).requires_grad_(), _dev(Y[None]).requires_grad_()
        out = dfepe.compat.dsac_batch(Xb, Yb, _dev(K), hyps, thresh, beta, alpha, idx=_dev(idx[None]), loss_kind=1)
        gb = torch.autograd.grad(out["exp_loss"].sum(), (Xb, Yb))
        assert torch.equal(gb[0][0], ge[0]) and torch.equal(gb[1][0], ge[1])
        ours = {("exp_loss", "gX"): ge[0], ("exp_loss", "gY"): ge[1], ("quality", "gX"): gq[0], ("quality", "gY"): gq[1]}
        for (what, key), val in ours.items():
            val = val.cpu().numpy().astype(np.float64)
            assert np.isfinite(val).all(), (k, what, key)
            if bool(g[f"{k}_finite"]):
                worst = max(worst, _pin(val, g[f"{k}_{what}_{key}"], float(g[f"{k}_{what}_yard_{key}"]), f"golden case {k} {what} {key}"))
        if not bool(g[f"{k}_finite"]):
            case = ac.make("golden_nan", 1, len(X), hyps, seed=int(g[f"{k}_seed"]), beta=beta, decided=False, zeros=True, up=("exp_loss",))
            case.update(X=X[None], Y=Y[None], K=K[None], idx=idx[None], thresh=thresh, alpha=alpha)
            _, got = run_abi(dfepe, case, up={"exp_loss": np.ones(1, F32)})
            assert np.array_equal(got["g_X"][0], ge[0].cpu().numpy()) and np.array_equal(got["g_Y"][0], ge[1].cpu().numpy())
            fwd, got = run_abi(dfepe, case)          # the case's own seeded upstream: the one check() restates
            assert (fwd["soft"] == 0).any() and np.isfinite(got["g_X"]).all() and np.isfinite(got["g_Y"]).all()
            ac.check(case, fwd, got)
    print(f"largest distance / yardstick over the finite cases: {worst:.3g}")


def test_runs_are_bit_identical_and_totals_change_nothing(dfepe):
    case = CASES[6]   # B = 3, H = 16, kind 2, exact-zero weights
    fwd = forward(dfepe, case)
    (_, a), (_, b) = run_abi(dfepe, case, fwd=fwd), run_abi(dfepe, case, fwd=fwd)
    _, c = run_abi(dfepe, case, fwd=fwd, totals=False)
    _, dx = run_abi(dfepe, case, fwd=fwd, totals=False, want_y=False)
    _, dy = run_abi(dfepe, case, fwd=fwd, totals=False, want_x=False)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    for k in ("g_X", "g_Y", "gpn1", "gg2"):
        assert np.array_equal(a[k], c[k]), k
    assert np.array_equal(a["g_X"], dx["g_X"]) and np.array_equal(a["g_Y"], dy["g_Y"]) and dx["g_Y"] is None and dy["g_X"] is None
    # a pair alone equals the pair in the batch
    up = ac.upstreams(case)
    for p in range(case["B"]):
        one = dict(case, B=1, X=case["X"][p:p + 1], Y=case["Y"][p:p + 1], K=case["K"][p:p + 1], idx=case["idx"][p:p + 1])
        f1 = {k: fwd[k][p:p + 1].contiguous() for k in fwd}
        _, s = run_abi(dfepe, one, fwd=f1, up={k: v[p:p + 1] for k, v in up.items()})
        assert np.array_equal(s["g_X"][0], a["g_X"][p]) and np.array_equal(s["g_Y"][0], a["g_Y"][p]), p
        assert np.array_equal(s["t_w"][:, 0], a["t_w"][:, p]) and np.array_equal(s["t_E_sample"][0], a["t_E_sample"][p]), p


def test_a_nan_stays_in_its_pair(dfepe):
    case = ac.make("scene", 3, 70, 5, seed=51, beta=0.002)
    bad = dict(case, X=case["X"].copy())
    bad["X"][1, 7, 0] = np.nan
    (_, a), (_, b) = run_abi(dfepe, case), run_abi(dfepe, bad)
    for k in ("g_X", "g_Y", "t_score", "t_loss", "t_E_refit", "t_E_sample", "gpn1", "gg1"):
        assert np.array_equal(a[k][[0, 2]], b[k][[0, 2]]), k
    assert np.array_equal(a["t_w"][:, [0, 2]], b["t_w"][:, [0, 2]])
    assert np.isfinite(a["g_X"]).all() and np.isnan(b["g_X"][1]).any()


def test_one_graph_capture_of_forward_and_backward_replays_bit_identically(dfepe):
    case = CASES[8]   # N = 129: the refit crosses DFEPE_W8PT16_MAX_N
    X, Y, K, idx = (_dev(case[k]) for k in ("X", "Y", "K", "idx"))
    X.requires_grad_()
    Y.requires_grad_()
    gx, gy = torch.zeros_like(X), torch.zeros_like(Y)
    state = {}

    def step():
        out = dfepe.ops.dsac(X, Y, K, idx, case["thresh"], case["beta"], case["alpha"], loss_kind=case["loss_kind"])
        a, b = torch.autograd.grad(out["exp_loss"].sum() + out["quality"].sum(), (X, Y))
        gx.copy_(a)
        gy.copy_(b)
        state["out"] = {k: v.detach() for k, v in out.items()}

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
    fresh = ac.make("scene", case["B"], case["N"], case["H"], seed=71, beta=0.002, decided=False)
    with torch.no_grad():
        for t, key in ((X, "X"), (Y, "Y"), (K, "K"), (idx, "idx")):
            t.copy_(_dev(fresh[key]))
    replays = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        replays.append(({k: v.clone() for k, v in captured.items()}, gx.clone(), gy.clone()))
    step()
    torch.cuda.synchronize()
    for outs, rx, ry in replays:
        assert torch.equal(rx, gx) and torch.equal(ry, gy)
        for k, v in state["out"].items():
            assert torch.equal(outs[k], v), k
    assert torch.isfinite(gx).all() and gx.abs().max() > 0
