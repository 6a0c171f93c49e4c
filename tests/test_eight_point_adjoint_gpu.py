"""The adjoint of the textbook eight-point solvers on the GPU (csrc/eight_point_adjoint.hip through the C ABI, ops and compat): every
case of tests/eight_point_adjoint_cases.py through its check(), each output alone, bitwise reproducibility, batch independence,
locality of a non-finite point, capture in a hipGraph, several weight sets through ops, and the compat mirrors under requires_grad
against the reference's own float64 autograd (tests/golden/eight_point_adjoint.npz) within one yardstick."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eight_point_adjoint_cases as ec  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
F32 = np.float32
OUTPUTS = ("g_X", "g_Y", "g_w")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(REPO, "tests", "golden", "eight_point_adjoint.npz"))


def _dev(a, grad=False):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV).requires_grad_(grad)


def run_gpu(dfepe, case, want=OUTPUTS):
    """dfepe_eight_point_bwd on the case as it stands (its own F_out and g_F); only the outputs in `want` are asked for."""
    ops, L = dfepe.ops, dfepe._lib.lib()
    S, B, N = case["S"], case["B"], case["N"]
    X, Y, w, Fo, g = (_dev(case[k]) for k in ("X", "Y", "w", "F_out", "g_F"))
    out = {"g_X": torch.full((B, N, 2), float("nan"), device=DEV) if "g_X" in want else None,
           "g_Y": torch.full((B, N, 2), float("nan"), device=DEV) if "g_Y" in want else None,
           "g_w": torch.full((S, B, N), float("nan"), device=DEV) if "g_w" in want else None}
    n = L.dfepe_eight_point_bwd_workspace_bytes(B, N, S)
    ws = torch.empty(n // 8, dtype=torch.float64, device=DEV) if n else None
    rc = L.dfepe_eight_point_bwd(ops._stream(), ops._ptr(X), ops._ptr(Y), ops._ptr(w), B, N, S, ec.flags_of(case), ops._ptr(Fo), ops._ptr(g),
                                 ops._ptr(out["g_X"]), ops._ptr(out["g_Y"]), ops._ptr(out["g_w"]), ops._ptr(ws))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


def _slice(case, pairs):
    """The case restricted to some of its pairs (no cached reference)."""
    c = {k: v for k, v in case.items() if k != "_ref"}
    c["X"], c["Y"] = case["X"][pairs], case["Y"][pairs]
    c["w"] = None if case["w"] is None else np.ascontiguousarray(case["w"][:, pairs])
    c["F_out"], c["g_F"] = np.ascontiguousarray(case["F_out"][:, pairs]), np.ascontiguousarray(case["g_F"][:, pairs])
    c["B"] = len(pairs)
    return c


def _ops_grads(dfepe, X, Y, w, essential, normalize, G):
    F = dfepe.ops.eight_point(X, Y, w, essential=essential, normalize=normalize)
    return F, torch.autograd.grad(F, [t for t in (X, Y, w) if t is not None and t.requires_grad], G)


def test_fails_on_the_code_as_it_stood(dfepe):
    case = ec.scene_cases()[0]
    F = dfepe.ops.eight_point(_dev(case["X"], True), _dev(case["Y"]), None, essential=False)
    assert F.requires_grad and F.grad_fn is not None


def test_kernel_passes_the_check_at_every_case(dfepe):
    for case in ec.scene_cases() + ec.exact_cases() + (ec.nonfinite_case(),):
        ec.check(case, run_gpu(dfepe, case))


def test_each_output_alone_and_two_runs_give_equal_bits(dfepe):
    cases = ec.scene_cases()
    picked = [next(c for c in cases if c["S"] == 1 and c["B"] == 5), next(c for c in cases if c["S"] == 3 and c["B"] == 3),
              next(c for c in cases if c["S"] == 3 and c["B"] == 70)]
    for case in picked:
        full, again = run_gpu(dfepe, case), run_gpu(dfepe, case)
        for key in OUTPUTS:
            assert np.array_equal(full[key], again[key]), (ec.name_of(case), key)
            alone = run_gpu(dfepe, case, want=(key,))
            assert np.array_equal(alone[key], full[key]), (ec.name_of(case), key)
            assert all(alone[k] is None for k in OUTPUTS if k != key)
            ec.check(case, alone)


def test_a_pair_alone_and_inside_a_batch_gives_equal_bits(dfepe):
    cases = ec.scene_cases()
    for case in (next(c for c in cases if c["S"] == 3 and c["B"] == 70), next(c for c in cases if c["S"] == 1 and c["B"] == 70)):
        full = run_gpu(dfepe, case)
        for pairs in ([37], [0, 69], [5, 6, 7, 8, 9]):
            part = run_gpu(dfepe, _slice(case, pairs))
            assert np.array_equal(part["g_X"], full["g_X"][pairs]) and np.array_equal(part["g_Y"], full["g_Y"][pairs])
            assert np.array_equal(part["g_w"], full["g_w"][:, pairs])


def test_a_non_finite_point_leaves_its_neighbours_bits_unchanged(dfepe):
    case = ec.nonfinite_case()
    got = run_gpu(dfepe, case)
    assert np.isnan(got["g_X"][1]).all() and np.isnan(got["g_w"][:, 1]).all()
    clean = _slice(case, [0, 1, 2])
    clean["X"] = clean["X"].copy()
    clean["X"][1, case["N"] // 2, 0] = 0.0
    other = run_gpu(dfepe, clean)
    for key in ("g_X", "g_Y"):
        assert np.isfinite(other[key]).all() and np.array_equal(got[key][[0, 2]], other[key][[0, 2]])
    assert np.array_equal(got["g_w"][:, [0, 2]], other["g_w"][:, [0, 2]])


def test_ops_backward_is_the_kernel_on_the_forward_it_ran(dfepe):
    """ops.eight_point forward + backward on case inputs: the gradients pass check() with F_out = what the forward returned."""
    cases = ec.scene_cases()
    for case in (next(c for c in cases if c["S"] == 1 and c["w"] is None and c["B"] == 3),
                 next(c for c in cases if c["S"] == 1 and c["w"] is not None and c["B"] == 5),
                 next(c for c in cases if c["S"] == 3 and c["B"] == 3)):
        S, B, N = case["S"], case["B"], case["N"]
        X, Y = _dev(case["X"], True), _dev(case["Y"], True)
        w = None if case["w"] is None else _dev(case["w"] if S > 1 else case["w"][0], True)
        G = _dev(case["g_F"] if S > 1 else case["g_F"][0])
        F, grads = _ops_grads(dfepe, X, Y, w, case["essential"], case["normalize"], G)
        assert tuple(F.shape) == ((S, B, 3, 3) if S > 1 else (B, 3, 3))
        seen = _slice(case, list(range(B)))
        seen["F_out"] = F.detach().cpu().numpy().reshape(S, B, 3, 3)
        got = {"g_X": grads[0].cpu().numpy(), "g_Y": grads[1].cpu().numpy(),
               "g_w": None if w is None else grads[2].cpu().numpy().reshape(S, B, N)}
        ec.check(seen, got)
        with torch.no_grad():  # nothing requiring grad: the forward launch alone, the same bits
            assert torch.equal(dfepe.ops.eight_point(X, Y, w, essential=case["essential"], normalize=case["normalize"]), F)
        assert not dfepe.ops.eight_point(X.detach(), Y.detach(), None if w is None else w.detach(), essential=case["essential"],
                                         normalize=case["normalize"]).requires_grad


def test_points_that_start_at_an_odd_element_of_their_buffer(dfepe):
    """A contiguous [B,N,2] view at an odd float offset is not 8-byte aligned, which the C entry refuses; ops copies it."""
    case = next(c for c in ec.scene_cases() if c["S"] == 1 and c["B"] == 5)
    B, N = case["B"], case["N"]
    flat = torch.cat((torch.zeros(1, device=DEV), _dev(case["X"]).flatten())).requires_grad_(True)
    X = flat[1:].reshape(B, N, 2)
    assert X.is_contiguous() and X.data_ptr() % 8 == 4
    Y, G = _dev(case["Y"], True), _dev(case["g_F"][0])
    _, (g_flat, gY) = _ops_grads_of(dfepe, (flat, Y), X, Y, case, G)
    Xa = _dev(case["X"], True)
    _, (gXa, gYa) = _ops_grads_of(dfepe, (Xa, Y), Xa, Y, case, G)
    assert torch.equal(g_flat[1:].reshape(B, N, 2), gXa) and torch.equal(gY, gYa) and float(g_flat[0]) == 0.0


def _ops_grads_of(dfepe, leaves, X, Y, case, G):
    F = dfepe.ops.eight_point(X, Y, None, essential=case["essential"], normalize=case["normalize"])
    return F, torch.autograd.grad(F, leaves, G)


def test_weight_sets_equal_separate_calls_and_point_gradients_their_sum(dfepe):
    case = next(c for c in ec.scene_cases() if c["S"] == 3 and c["B"] == 5)
    S = case["S"]
    X, Y, w = _dev(case["X"], True), _dev(case["Y"], True), _dev(case["w"], True)
    G = _dev(case["g_F"])
    F, (gX, gY, gw) = _ops_grads(dfepe, X, Y, w, case["essential"], case["normalize"], G)
    sumX, sumY = torch.zeros_like(gX, dtype=torch.float64), torch.zeros_like(gY, dtype=torch.float64)
    for s in range(S):
        ws = w[s].detach().clone().requires_grad_(True)
        Fs, (gXs, gYs, gws) = _ops_grads(dfepe, X, Y, ws, case["essential"], case["normalize"], G[s])
        assert torch.equal(Fs, F[s]) and torch.equal(gws, gw[s])
        sumX += gXs.double()
        sumY += gYs.double()
    # each call rounds its point gradients to fp32 before they are added here; the joint call adds in fp64 and rounds once
    for joint, parts in ((gX, sumX), (gY, sumY)):
        tol = (S + 1) * 2.0 ** -24 * parts.abs().amax(dim=(1, 2), keepdim=True)
        assert ((joint.double() - parts).abs() <= tol).all()


def test_forward_and_backward_replay_from_a_graph(dfepe):
    cases = ec.scene_cases()
    first = next(c for c in cases if c["S"] == 3 and c["B"] == 3 and c["N"] >= 16)
    X, Y, w = _dev(first["X"], True), _dev(first["Y"], True), _dev(first["w"], True)
    G = _dev(first["g_F"])
    state = {}

    def step():
        state["F"], state["g"] = _ops_grads(dfepe, X, Y, w, first["essential"], first["normalize"], G)

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
    with torch.no_grad():  # other values in the captured buffers: the replay must recompute, not remember
        X.copy_(X.flip(0))
        Y.copy_(Y.flip(0))
        w.copy_(w.flip(1))
    graph.replay()
    torch.cuda.synchronize()
    replayed = [state["F"].clone()] + [g.clone() for g in state["g"]]
    step()
    torch.cuda.synchronize()
    for a, b in zip(replayed, [state["F"]] + list(state["g"])):
        assert torch.equal(a, b)
    assert torch.isfinite(replayed[1]).all() and not torch.equal(replayed[1], torch.zeros_like(replayed[1]))


def _held(name, ours, ref, yard):
    tol = max(float(yard), 2.0 ** -22 * np.abs(ref).max())
    err = np.abs(ours.astype(np.float64) - ref).max()
    print(f"{name}: {err / float(yard):.3f} yardsticks ({err / np.abs(ref).max():.2e} of max |g|)")
    assert err <= tol, (name, err, tol)


def test_compat_gradients_within_one_yardstick_of_the_reference(dfepe, golden):
    """_F_from_XY / _E_from_XY / _E_from_XY_batch under requires_grad on the golden cases: within one yardstick (max |the reference's
    float32 autograd - its float64 autograd|, floor 2^-22 max |g|) of the reference's float64 gradients.  The torch route this
    replaces differentiates the Hartley transforms and is hundreds of yardsticks off wherever `normalize` holds."""
    uF = dfepe.compat.utils_F
    cases = ec.golden_cases()
    for k, c in enumerate(cases):
        ref_out, g = golden[f"{k}_out"], _dev(c["g"])
        eye = torch.eye(3, device=DEV)
        forms = ["single"] + (["batch"] if c["essential"] else [])
        for form in forms:
            for wform in (("none",) if c["ws"] is None else ("diag", "vector")):
                X, Y = _dev(c["X"], True), _dev(c["Y"], True)
                ws = None if c["ws"] is None else _dev(c["ws"], wform == "vector")
                W = None if ws is None else (torch.diag(ws) if wform == "diag" else ws)
                if form == "batch":
                    Wb = None if W is None else (ws[None] if wform == "vector" else W[None])
                    out = uF._E_from_XY_batch(X[None], Y[None], eye[None], W=Wb, if_normzliedK=True, normalize=c["normalize"])[0]
                elif c["essential"]:
                    out = uF._E_from_XY(X, Y, eye, W=W, if_normzliedK=True, normalize=c["normalize"])
                else:
                    out = uF._F_from_XY(X, Y, W=W, normalize=c["normalize"])
                assert out.grad_fn is not None
                sgn = 1.0 if float((out.detach().cpu().double().numpy() * ref_out).sum()) >= 0 else -1.0
                (sgn * g * out).sum().backward()
                tag = f"case {k} {form} W={wform}"
                _held(tag + " gX", X.grad.cpu().numpy(), golden[f"{k}_gX"], golden[f"{k}_yard_gX"])
                _held(tag + " gY", Y.grad.cpu().numpy(), golden[f"{k}_gY"], golden[f"{k}_yard_gY"])
                if wform == "vector":
                    _held(tag + " gws", ws.grad.cpu().numpy(), golden[f"{k}_gws"], golden[f"{k}_yard_gws"])


def test_compat_routes(dfepe):
    """K keeps its gradient through the K^-1 step in front of the kernel; a 2-D W that requires grad stays on the torch route; the
    batch form refuses it."""
    uF = dfepe.compat.utils_F
    c = ec.golden_cases()[8]
    N = c["N"]
    K = torch.tensor(ec.K, dtype=torch.float32, device=DEV).requires_grad_(True)
    px = (torch.cat((_dev(c["X"]), torch.ones(N, 1, device=DEV)), 1) @ K.detach().t())[:, :2]
    py = (torch.cat((_dev(c["Y"]), torch.ones(N, 1, device=DEV)), 1) @ K.detach().t())[:, :2]
    E = uF._E_from_XY(px, py, K)
    E[0, 1].backward()
    assert K.grad is not None and torch.isfinite(K.grad).all() and float(K.grad.abs().max()) > 0
    W = torch.diag(torch.rand(N, device=DEV) + 0.5).requires_grad_(True)
    F = uF._F_from_XY(_dev(c["X"]), _dev(c["Y"]), W=W)
    F[0, 1].backward()
    assert W.grad is not None and float((W.grad - torch.diag(torch.diagonal(W.grad))).abs().max()) > 0   # off-diagonal gradient: torch route
    with pytest.raises(dfepe.DfepeError):
        uF._E_from_XY_batch(_dev(c["X"])[None], _dev(c["Y"])[None], torch.eye(3, device=DEV)[None], W=W[None], if_normzliedK=True)
