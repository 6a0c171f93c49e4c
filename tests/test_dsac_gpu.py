"""dfepe_dsac on the GPU: every shared case and edge of tests/dsac_cases.py through its check() against the fp64 restatement
(tests/dsac_ref.py), the reference's own float32 run (tests/golden/dsac.npz) through compat.DSAC, the batch against per-pair calls,
reproducibility, and one hipGraph capture.  GPU box only."""
import os
import random
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dsac_cases as dc  # noqa: E402
import dsac_ref as dr  # noqa: E402

DEV = "cuda:0"
F32 = np.float32
CASES = dc.all_cases()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(dfepe, case, **kw):
    out = dfepe.ops.dsac(_dev(case["X"]), _dev(case["Y"]), _dev(case["K"]), _dev(case["idx"]), case["thresh"], case["beta"], case["alpha"],
                         loss_kind=case["loss_kind"], **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _edge(name):
    return next(c for c in CASES if c["name"] == name)


def test_cases_are_built_around_the_kernels_constants(dfepe):
    L = dfepe._lib.lib()
    P, V, T = L.dfepe_dsac_hyps_per_block(), L.dfepe_dsac_vote_chunk(), L.dfepe_dsac_vote_tile()
    assert [dc.name_of(c) for c in dc.size_cases(P, V)] == [dc.name_of(c) for c in dc.size_cases()]
    Hs, Ns = {c["H"] for c in CASES}, {c["N"] for c in CASES}
    assert {P - 1, P, P + 1, T - 1, T, T + 1, 1, 2, 15, 16, 17, 65} <= Hs
    assert {V - 1, V, V + 1, 10, 11, 16, 17, 63, 64, 65, 129} <= Ns
    assert {c["S"] for c in CASES} == {8, 10, 16} and {c["B"] for c in CASES} == {1, 3}


@pytest.mark.parametrize("k", range(len(CASES)), ids=[dc.name_of(c) for c in CASES])
def test_case_passes_the_check(dfepe, k):
    case = CASES[k]
    got = run(dfepe, case)
    for key in dc.OUT_KEYS:
        assert key in got, key
    dc.check(case, got)


def test_beta_zero_is_exact(dfepe):
    case = _edge("beta0")
    dc.check_beta0(case, run(dfepe, case))


def test_unsampled_correspondences_and_the_ends(dfepe):
    case = _edge("unsampled")
    got = run(dfepe, case)
    never = np.ones(case["N"], bool)
    never[case["idx"][0].ravel()] = False
    assert never.sum() >= case["N"] - case["H"] * case["S"] > 0
    assert (got["counts"][0][never] == 0).all() and (got["quality"][0][never] == 0).all() and (got["counts"][0][~never] >= 1).all()
    case = _edge("ends")
    got = run(dfepe, case)
    assert (got["counts"][:, 0] >= 1).all() and (got["counts"][:, case["N"] - 1] >= 1).all()


def test_saturated_weights_stay_finite_and_no_score_is_above_zero(dfepe):
    case = _edge("saturated")
    got = run(dfepe, case)
    assert (got["score"] == 0).all() and (got["best"] == -1).all() and (got["top_loss"] == 0).all() and (got["soft"] == 0).all()
    for key in ("E_sample", "E_refit", "loss", "quality", "exp_loss"):
        assert np.isfinite(got[key]).all(), key
    _, term = dr.stage3(got["soft"], case["X"], case["Y"], case["K"])
    assert not np.vectorize(dr.decided)(term).any()


def test_equal_sets_tie_within_the_bound(dfepe):
    """N = S: every hypothesis is the same set in another order, so every E is the same matrix within the bound and the scores tie
    to rounding; `best` is whichever the kernel's own scores make first (check() holds it to that)."""
    case = _edge("n_equals_s")
    got = run(dfepe, case)
    xn, yn = dr.kinv_points(case["X"], case["K"]), dr.kinv_points(case["Y"], case["K"])
    E64, term = dr.fit(xn[0], yn[0])
    assert dr.decided(term)
    for h in range(case["H"]):
        assert dr.unit_diff(got["E_sample"][0, h], E64) <= dr.fit_bound(term)
    # the fits agree to ~1e-7, which moves an inlier's weight by less than its own fp32 rounding: the ten-term scores differ by ulps
    assert np.ptp(got["score"][0]) <= 1e-4


def test_a_nan_stays_in_its_pair(dfepe):
    case = dc.make("scene", 3, 70, 5, seed=51)
    bad = dict(case, X=case["X"].copy())
    bad["X"][1, 7, 0] = np.nan
    a, b = run(dfepe, case), run(dfepe, bad)
    for k in dc.OUT_KEYS:
        assert np.array_equal(a[k][[0, 2]], b[k][[0, 2]], equal_nan=True), k
    assert np.isnan(b["score"][1]).all() and (b["best"][1] == -1)


def test_two_runs_are_bit_identical_and_optional_outputs_change_nothing(dfepe):
    case = CASES[5]
    a, b, c = run(dfepe, case), run(dfepe, case), run(dfepe, case, want=())
    for k in dc.OUT_KEYS:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert set(c) == set(dc.OUT_KEYS) - {"soft", "sampson", "exp_loss", "top_loss"}
    for k in c:
        assert np.array_equal(a[k], c[k], equal_nan=True), k


def test_golden_pin_through_the_mirror(dfepe, golden):
    """compat.DSAC, seeded like the reference's run, against the float64 values: within max(4 x the reference's own float32 distance,
    1e-6 of the largest entry), the rule of tests/test_refcfg_gpu.py (two independent fp32 evaluations, a maximum over many entries);
    the drawn indices are the reference's exactly."""
    g = golden("dsac")
    for k, case in enumerate(dc.golden_cases()):
        d = dfepe.compat.DSAC(case["hyps"], case["thresh"], case["beta"], case["alpha"], torch.from_numpy(case["K"]), dfepe.compat.H_loss.HLoss())
        random.seed(case["seed"])
        q = d(torch.from_numpy(case["X"]), torch.from_numpy(case["Y"]), None)
        assert q.dtype == torch.float32 and q.device.type == "cpu" and tuple(q.shape) == (case["N"], 1)
        idx = g[f"{k}_idx"]
        assert d.best_corres_idx == idx[d.best_H_idx].tolist()
        ours = {"inlier_scores": d.inlier_scores.cpu().numpy(), "sampson_dists": d.sampson_dists.cpu().numpy(), "quality": q.numpy(),
                "max_score": np.float64(d.max_score)}
        for name, val in ours.items():
            truth, yard = g[f"{k}_f64_{name}"], float(g[f"{k}_yard_{name}"])
            dist, bound = float(np.abs(val - truth).max()), max(4 * yard, 1e-6 * float(np.abs(truth).max()))
            print(f"golden case {k} {name}: distance {dist:.3g}, reference's float32 {yard:.3g}, bound {bound:.3g}")
            assert dist <= bound, (k, name, dist, bound)
        top = np.sort(g[f"{k}_f64_hyp_scores"])[::-1]
        if top[0] - top[1] > 8 * float(g[f"{k}_yard_max_score"]) + 1e-4:
            assert d.best_H_idx == int(g[f"{k}_f64_best_H_idx"]) == int(g[f"{k}_best_H_idx"])
        assert d.hyp_losses.shape == (case["hyps"],) and torch.isfinite(d.hyp_losses).all()
        assert float(d.top_loss) == float(d.hyp_losses[d.best_H_idx])


def test_batch_equals_per_pair_mirror_calls(dfepe):
    B, N, H = 3, 50, 6
    X, Y, K = dc.scene(B, N, 61, 0.2)
    random.seed(9)
    singles = []
    for b in range(B):
        d = dfepe.compat.DSAC(H, dc.THRESH, dc.BETA, dc.ALPHA, torch.from_numpy(K[b]), dfepe.compat.H_loss.HLoss())
        q = d(torch.from_numpy(X[b]), torch.from_numpy(Y[b]), None)
        singles.append((q, d))
    random.seed(9)
    idx = torch.tensor([[random.sample(range(N), 10) for _ in range(H)] for _ in range(B)], dtype=torch.int32)
    out = dfepe.compat.dsac_batch(_dev(X), _dev(Y), _dev(K), H, dc.THRESH, dc.BETA, dc.ALPHA, idx=idx.to(DEV), loss_kind=1)
    for b, (q, d) in enumerate(singles):   # N <= 128: the same fit kernels whatever the batch, so the same bits
        assert torch.equal(out["quality"][b].cpu(), q[:, 0]) and torch.equal(out["soft"][b], d.inlier_scores)
        assert torch.equal(out["score"][b], d.hyp_scores) and torch.equal(out["loss"][b], d.hyp_losses)
        assert int(out["best"][b]) == d.best_H_idx and torch.equal(out["E_refit"][b, d.best_H_idx], d.best_H)
    drawn = dfepe.compat.dsac_batch(_dev(X), _dev(Y), _dev(K), H, dc.THRESH, dc.BETA, seed=9)
    rng = random.Random(9)
    assert drawn["idx"].cpu().tolist() == [[rng.sample(range(N), 10) for _ in range(H)] for _ in range(B)]
    assert torch.equal(drawn["quality"], out["quality"])


def test_one_graph_capture_replays_bit_identically(dfepe):
    case = CASES[7]   # N = 129: the refit crosses DFEPE_W8PT16_MAX_N
    X, Y, K, idx = (_dev(case[k]) for k in ("X", "Y", "K", "idx"))
    state = {}

    def step():
        state["out"] = dfepe.ops.dsac(X, Y, K, idx, case["thresh"], case["beta"], case["alpha"], loss_kind=case["loss_kind"])

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
    fresh = dc.make("scene", case["B"], case["N"], case["H"], seed=71, decided=False)   # not one of the chosen seeds: no cap on it
    for t, key in ((X, "X"), (Y, "Y"), (K, "K"), (idx, "idx")):
        t.copy_(_dev(fresh[key]))
    replays = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        replays.append({k: v.clone() for k, v in captured.items()})
    step()
    torch.cuda.synchronize()
    for k, v in state["out"].items():
        assert torch.equal(replays[0][k], v) and torch.equal(replays[1][k], v), k
    dc.check(fresh, {k: v.cpu().numpy() for k, v in state["out"].items()})
