"""The adjoints of the epipolar distances on the GPU (csrc/epi_adjoint.hip through ops and compat): every kind and the residual at
every launch edge through the check() of tests/epi_adjoint_cases.py, bitwise reproducibility, the reduced loss form, the compat
mirrors under requires_grad against the restatement and the reference's own float64 autograd, locality of a non-finite point, and
capture in a hipGraph."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epi_adjoint_cases as ac  # noqa: E402
import epi_adjoint_ref as ar  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
F32 = np.float32


@pytest.fixture(scope="module")
def P(dfepe):
    return dfepe._lib.lib().dfepe_epi_adjoint_chunk()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(REPO, "tests", "golden", "epi_adjoint.npz"))


def _dev(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).requires_grad_(grad)


def run_gpu(dfepe, case, want=("g_F", "g_X", "g_Y")):
    """The gradients ops gives for the case's upstream g, only those in `want` requested."""
    F, X, Y = _dev(case["F"], "g_F" in want), _dev(case["X"], "g_X" in want), _dev(case["Y"], "g_Y" in want)
    if case["op"] == "residual":
        out = dfepe.ops.epi_residual(X, Y, F, case["clamp_at"])
    else:
        out = dfepe.ops.epi_metrics(case["kind"], F, X, Y, clamp_at=case["clamp_at"], eps=case["eps"])
    out.backward(_dev(case["g"]))
    got = {k: (None if t.grad is None else t.grad.cpu().numpy()) for k, t in (("g_F", F), ("g_X", X), ("g_Y", Y))}
    if case["op"] == "residual":
        got["g_F"] = None  # the adjoint to F is dfepe_epi_residual_bwd's, held by tests/test_epipolar_gpu.py
    return got


def _ladder_case(kind, B, N, homo, seed=0):
    return ac.make("scene", kind, B, N, homo, clamp=(kind == 0), eps=1e-10 if kind == 0 else 0.0, seed=seed)


def test_fails_on_the_code_as_it_stood(dfepe):
    case = _ladder_case(1, 1, 5, False)
    assert dfepe.ops.epi_metrics(1, _dev(case["F"], True), _dev(case["X"]), _dev(case["Y"])).requires_grad
    res = _ladder_case(3, 1, 5, True)
    got = run_gpu(dfepe, res, ("g_X", "g_Y"))
    assert got["g_X"] is not None and got["g_Y"] is not None


# N = m P + o: the edges of a wavefront's slab (64), of a pass of the workgroup (256) and of a chunk (P), one point and two chunks + 1
LADDER = [(0, 1), (0, 2), (0, 63), (0, 64), (0, 65), (0, 255), (0, 256), (0, 257), (1, -1), (1, 0), (1, 1), (2, 1)]


@pytest.mark.parametrize("m,o", LADDER, ids=[(f"{m}P{o:+d}" if m else str(o)) for m, o in LADDER])
def test_every_kind_at_every_launch_edge(dfepe, P, m, o):
    N = m * P + o
    for B in (1, 3):
        for kind in ac.KINDS:
            for homo in ((True,) if kind == 3 else (False, True)):
                case = _ladder_case(kind, B, N, homo, seed=kind)
                ac.check(case, run_gpu(dfepe, case))


def test_every_shared_family(dfepe):
    for case in ac.cpu_cases():
        ac.check(case, run_gpu(dfepe, case))


def test_each_gradient_alone_has_the_bits_it_has_with_the_others(dfepe, P):
    for kind, homo in ((0, False), (1, True), (2, False), (3, True)):
        case = _ladder_case(kind, 3, P + 1, homo)
        together = run_gpu(dfepe, case)
        for key in ("g_F", "g_X", "g_Y"):
            if together[key] is None:
                continue
            alone = run_gpu(dfepe, case, (key,))
            assert all(alone[k] is None for k in alone if k != key)
            assert alone[key].tobytes() == together[key].tobytes(), (kind, key)


def test_bitwise_reproducible_and_independent_of_the_batch(dfepe, P):
    for kind, homo, N in ((0, True, 2 * P + 1), (1, False, P + 1), (2, True, 257), (3, True, P + 1)):
        case = _ladder_case(kind, 3, N, homo)
        a, b = run_gpu(dfepe, case), run_gpu(dfepe, case)
        one = dict(case, B=1, F=case["F"][1:2], X=case["X"][1:2], Y=case["Y"][1:2], g=case["g"][:, 1:2] if kind == 2 else case["g"][1:2])
        c = run_gpu(dfepe, one)
        for key in ("g_F", "g_X", "g_Y"):
            if a[key] is None:
                continue
            assert a[key].tobytes() == b[key].tobytes(), (kind, key)
            assert a[key][1:2].tobytes() == c[key].tobytes(), (kind, key)


def test_a_non_finite_point_stays_local(dfepe, P):
    N = P + 70
    case = ac.make("nonfinite", 0, 3, N, False, clamp=True, eps=0.0, seed=5)
    clean = dict(case, X=case["X"].copy())
    clean["X"][1, N // 2, 0] = 1.0
    a, b = run_gpu(dfepe, case), run_gpu(dfepe, clean)
    keep = np.ones(N, bool)
    keep[N // 2] = False
    for key in ("g_X", "g_Y"):
        assert a[key][[0, 2]].tobytes() == b[key][[0, 2]].tobytes() and a[key][1][keep].tobytes() == b[key][1][keep].tobytes()
    assert a["g_F"][[0, 2]].tobytes() == b["g_F"][[0, 2]].tobytes()


def _loss_gpu(dfepe, case, w, gs):
    F, X, Y = _dev(case["F"], True), _dev(case["X"], True), _dev(case["Y"], True)
    wt = None if w is None else _dev(w, True)
    sums = dfepe.ops.epi_loss(case["kind"], F, X, Y, weights=wt, clamp_at=case["clamp_at"], eps=case["eps"], reduction="none")
    sums.backward(_dev(gs))
    return {"sums": sums.detach().cpu().numpy(), "g_F": F.grad.cpu().numpy(), "g_X": X.grad.cpu().numpy(), "g_Y": Y.grad.cpu().numpy(),
            "g_w": None if wt is None else wt.grad.cpu().numpy()}


def test_reduced_loss_form(dfepe, P):
    rng = np.random.default_rng(11)
    for kind, homo, N in ((0, False, 65), (0, True, P + 1), (1, True, 257), (1, False, 2 * P + 1), (2, False, P), (2, True, 63)):
        case = _ladder_case(kind, 3, N, homo, seed=20 + kind)
        gs = rng.standard_normal(3).astype(F32)
        for w in (None, rng.uniform(0, 1, (3, N)).astype(F32)):
            got = _loss_gpu(dfepe, case, w, gs)
            r = ac.check_loss(case, w, gs, got)
            # the same gradient through the per-point route, ops.epi_metrics(...).mul(w).sum().  Its upstream is the fp32 product
            # float32(g_sum w) that torch's backward forms (one rounding per point, 2^-24 T more between the two routes), so it is held
            # to the restatement at exactly that upstream, and the two routes to each other within the sum of their bounds
            F = _dev(case["F"], True)
            e = dfepe.ops.epi_metrics(kind, F, _dev(case["X"]), _dev(case["Y"]), clamp_at=case["clamp_at"], eps=case["eps"])
            e = e[0] if kind == 2 else e
            e = e if w is None else e.mul(_dev(w))
            (e.sum(1) * _dev(gs)).sum().backward()
            g32 = np.broadcast_to(gs[:, None], (3, N)).astype(F32) if w is None else gs[:, None] * w
            assert g32.dtype == F32
            g32 = np.stack((g32, np.zeros_like(g32), np.zeros_like(g32))) if kind == 2 else g32
            r2 = ac.reference(dict(case, g=g32))
            bnd, bnd2 = ar.bound_sum(r.gF, r.MF_pt, r.TF_pt, r.WF_pt), ar.bound_sum(r2.gF, r2.MF_pt, r2.TF_pt, r2.WF_pt)
            per_point = F.grad.cpu().numpy()
            assert ar.within(per_point, r2.gF, bnd2).all()
            assert (np.abs(per_point.astype(np.float64) - got["g_F"]) <= bnd + bnd2 + ar.U32 * r.TF).all()
    # the reductions of the wrapper
    case = _ladder_case(0, 2, 70, True)
    F, X, Y = _dev(case["F"]), _dev(case["X"]), _dev(case["Y"])
    none = dfepe.ops.epi_loss(0, F, X, Y, clamp_at=case["clamp_at"], eps=1e-10, reduction="none")
    assert none.shape == (2,) and not none.requires_grad
    assert torch.equal(dfepe.ops.epi_loss(0, F, X, Y, clamp_at=case["clamp_at"], eps=1e-10), none.sum())
    assert torch.equal(dfepe.ops.epi_loss(0, F, X, Y, clamp_at=case["clamp_at"], eps=1e-10, reduction="mean"), none.sum() / 140)


def test_compat_mirrors_under_requires_grad(dfepe, golden):
    """Values bit-equal to the no-grad kernel path; gradients within the bound of the restatement and, on top of it, within the
    measured distance of the restatement from the reference's own float64 autograd."""
    uF = dfepe.compat.utils_F
    for k, case in enumerate(ac.golden_cases()):
        kind, homo, cl = case["kind"], case["homo"], case["clamp_at"]
        forms = [("", slice(None))] if kind == 3 else [("", slice(None)), ("2", 0)]
        for suffix, sel in forms:
            F, X, Y = _dev(case["F"][sel], True), _dev(case["X"][sel], True), _dev(case["Y"][sel], True)
            fn = {0: lambda a, b, c: uF._sym_epi_dist(a, b, c, if_homo=homo, clamp_at=cl), 1: lambda a, b, c: uF._sampson_dist(a, b, c, if_homo=homo),
                  2: lambda a, b, c: torch.stack(uF._epi_distance(a, b, c, if_homo=homo)), 3: lambda a, b, c: uF.compute_epi_residual(b, c, a, cl)}[kind]
            out = fn(F, X, Y)
            assert out.requires_grad
            plain = fn(F.detach(), X.detach(), Y.detach())
            assert not plain.requires_grad and torch.equal(out.detach(), plain)
            g = (case["g"][:, sel] if kind == 2 else case["g"][sel])
            out.backward(_dev(g))
            sub = slice(None) if suffix == "" else slice(0, 1)
            g_ref = case["g"][:, sub] if kind == 2 else case["g"][sub]
            if kind == 3:
                r = ar.residual_adjoint(case["X"][sub], case["Y"][sub], case["F"][sub], cl, g_ref)
                parts = [(X.grad, r.g1, r.M1, r.W1, "gX"), (Y.grad, r.g2, r.M2, r.W2, "gY")]
            else:
                r = ar.metrics_adjoint(kind, case["F"][sub], case["X"][sub], case["Y"][sub], homo, g_ref, cl, case["eps"] if suffix == "" else 0.0)
                sd = 3 if homo else 2
                parts = [(X.grad, r.gX[..., :sd], r.MX[..., :sd], r.WX[..., :sd], "gX"), (Y.grad, r.gY[..., :sd], r.MY[..., :sd], r.WY[..., :sd], "gY")]
                bF = ar.bound_sum(r.gF, r.MF_pt, r.TF_pt, r.WF_pt)
                gotF = F.grad.cpu().numpy().reshape(r.gF.shape)
                assert ar.within(gotF, r.gF, bF).all()
                gold = golden[f"{k}_gF{suffix}"].reshape(r.gF.shape)
                assert (np.abs(gotF - gold) <= bF + ar.C_GOLDEN * ar.U64 * (r.MF + r.N * r.TF / ar.C_GOLDEN)).all()
            for grad, ref, M, W, name in parts:
                got = grad.cpu().numpy().reshape(ref.shape)
                bnd = ar.bound_point(ref, M, W)
                assert ar.within(got, ref, bnd).all(), (k, suffix, name)
                gold = golden[f"{k}_{name}{suffix}"].reshape(ref.shape)
                assert (np.abs(got - gold) <= bnd + ar.C_GOLDEN * ar.U64 * M).all(), (k, suffix, name)


def test_get_loss_softmax_and_hloss_against_the_golden(dfepe, golden):
    cases = ac.golden_cases()
    k = next(i for i, c in enumerate(cases) if c["kind"] == 0 and c["homo"] and c["clamp_at"] is not None)
    case = cases[k]
    B, N = case["B"], case["N"]
    F, X, Y = _dev(case["F"], True), _dev(case["X"], True), _dev(case["Y"], True)
    mean, losses = dfepe.compat.train_good_utils.get_loss_softmax(F, X, Y, case["clamp_at"])
    gold = golden[f"{k}_value"]
    r = ar.metrics_adjoint(0, case["F"], case["X"], case["Y"], True, np.full((B, N), F32(1.0 / (B * N))), case["clamp_at"], 1e-10)
    assert ar.within(losses.detach().cpu().numpy(), r.value, ar.bound(r.value, r.vmag)).all()
    assert (np.abs(losses.detach().cpu().numpy() - gold) <= ar.bound(r.value, r.vmag) + ar.C_GOLDEN * ar.U64 * r.vmag).all()
    # torch's fp32 mean of B N fp32 values: at most B N roundings of partial sums no larger than the sum of the values
    assert abs(mean.item() - gold.mean()) <= (B * N + 2) * ar.U32 * np.abs(gold).mean() + ar.bound(r.value, r.vmag).mean()
    mean.backward()
    ac.check(dict(case, g=np.full((B, N), F32(1.0 / (B * N)))), {"g_F": F.grad.cpu().numpy(), "g_X": X.grad.cpu().numpy(), "g_Y": Y.grad.cpu().numpy()})
    # HLoss: the mean Sampson distance of the 2-D form
    k = next(i for i, c in enumerate(cases) if c["kind"] == 1 and not c["homo"])
    case = cases[k]
    H, X, Y = _dev(case["F"][0], True), _dev(case["X"][0], True), _dev(case["Y"][0], True)
    loss = dfepe.compat.H_loss.HLoss()(H, X, Y)
    gold = golden[f"{k}_value2"]
    one = dict(case, B=1, F=case["F"][:1], X=case["X"][:1], Y=case["Y"][:1], g=np.full((1, N), F32(1.0 / N)))
    r = ac.reference(one)
    assert abs(loss.item() - gold.mean()) <= (N + 2) * ar.U32 * np.abs(gold).mean() + ar.bound(r.value, r.vmag).mean() + ar.C_GOLDEN * ar.U64 * r.vmag.mean()
    loss.backward()
    ac.check(one, {"g_F": H.grad.cpu().numpy()[None], "g_X": X.grad.cpu().numpy()[None], "g_Y": Y.grad.cpu().numpy()[None]}, ref=r)


def test_loss_forward_and_backward_replay_from_a_graph(dfepe, P):
    B, N = 4, P + 1
    first, fresh = _ladder_case(0, B, N, True, seed=31), _ladder_case(0, B, N, True, seed=32)
    cl = first["clamp_at"]
    F, X, Y = _dev(first["F"], True), _dev(first["X"], True), _dev(first["Y"], True)
    state = {}

    def step():
        loss = dfepe.ops.epi_loss(0, F, X, Y, clamp_at=cl, eps=1e-10, reduction="mean")
        state["loss"], state["g"] = loss, torch.autograd.grad(loss, (F, X, Y))

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
    with torch.no_grad():
        for t, a in ((F, fresh["F"]), (X, fresh["X"]), (Y, fresh["Y"])):
            t.copy_(_dev(a))
    graph.replay()
    torch.cuda.synchronize()
    replayed = [state["loss"].clone()] + [g.clone() for g in state["g"]]
    step()
    torch.cuda.synchronize()
    for a, b in zip(replayed, [state["loss"]] + list(state["g"])):
        assert torch.equal(a, b)
    assert not torch.equal(replayed[1], torch.zeros_like(replayed[1]))
