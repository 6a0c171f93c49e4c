"""The DSAC hypothesis loop without a GPU: the fp64 restatement (tests/dsac_ref.py) against the reference's own float32 run
(tests/golden/dsac.npz) and against plain loops, the host build of csrc/dsac_math.h (tests/emu/emu_dsac.cpp, chained with the host
build of the fit kernels, tests/emu/emu_w8pt16.cpp, the way dfepe_dsac chains its six launches) through the same check() as the GPU,
and the C ABI's refusals, which are made before any HIP call."""
import ctypes
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dsac_cases as dc  # noqa: E402
import dsac_ref as dr  # noqa: E402

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EMU_DIR = os.path.join(REPO, "tests", "emu")
CSRC = os.path.join(REPO, "pytorch-deepfepe_amd", "csrc")
F32 = np.float32
INVALID, UNSUPPORTED = -1, -3
FIT_FLAGS = 4 | 8 | 16  # DFEPE_W8PT_SQRT2 | NO_ROWNORM | FORCE_110


def _build(lib, srcs, extra):
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", *extra, srcs[0], "-o", lib], check=True)
    return ctypes.CDLL(lib)


@pytest.fixture(scope="module")
def emu():
    out = os.path.join(EMU_DIR, "_build")
    os.makedirs(out, exist_ok=True)
    L = _build(os.path.join(out, "libemu_dsac.so"),
               [os.path.join(EMU_DIR, "emu_dsac.cpp"), os.path.join(CSRC, "dsac_math.h"), os.path.join(CSRC, "epi_adjoint_math.h")],
               ["-ffp-contract=off", f"-I{CSRC}"])
    fit = _build(os.path.join(out, "libemu_w8pt16.so"),
                 [os.path.join(EMU_DIR, "emu_w8pt16.cpp"), os.path.join(EMU_DIR, "rowgroup.h")] +
                 [os.path.join(CSRC, f) for f in ("w8pt16_body.h", "w8pt16_bwd_body.h", "loss_tail_body.h", "pose_math.h", "dfepe_math.h",
                                                  "fit_plan.h")] + [os.path.join(REPO, "include", "dfepe.h")],
                 [f"-I{EMU_DIR}", f"-I{CSRC}", f"-I{REPO}/include"])
    i, p, fl, u = ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_uint
    L.emu_dsac_prep.argtypes = [p, p, p, p, i, i, i, i, p, p, p, p, p]
    L.emu_dsac_prep.restype = None
    L.emu_dsac_hyp.argtypes = [i, p, p, p, p, i, i, i, fl, fl, i, p, p, p, p, p, p]
    L.emu_dsac_hyp.restype = None
    L.emu_dsac_vote.argtypes = [p, p, p, fl, i, i, i, i, p, p, p, p, p]
    L.emu_dsac_vote.restype = None
    fit.emu_w8pt16_fwd.restype = i
    fit.emu_w8pt16_fwd.argtypes = [p, p, p, i, i, i, u, fl, fl, fl, p, p, p, p, p]
    L.fit = fit
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def run_emu(L, case):
    """The six steps of dfepe_dsac on the host."""
    B, N, H, S = case["B"], case["N"], case["H"], case["S"]
    X, Y, K, idx = (np.ascontiguousarray(case[k]) for k in ("X", "Y", "K", "idx"))
    pn1, pn2 = np.zeros((B, N, 3), F32), np.zeros((B, N, 3), F32)
    g1, g2, ones = np.zeros((B * H, S, 3), F32), np.zeros((B * H, S, 3), F32), np.zeros((B * H, S), F32)
    L.emu_dsac_prep(_p(X), _p(Y), _p(K), _p(idx), B, N, H, S, _p(pn1), _p(pn2), _p(g1), _p(g2), _p(ones))
    got = {"E_sample": np.zeros((B, H, 3, 3), F32), "soft": np.zeros((B, H, N), F32), "sampson": np.zeros((B, H, N), F32),
           "score": np.zeros((B, H), F32), "E_refit": np.zeros((B, H, 3, 3), F32), "loss": np.zeros((B, H), F32),
           "quality": np.zeros((B, N), F32), "counts": np.zeros((B, N), F32), "best": np.zeros(B, np.int32),
           "exp_loss": np.zeros(B, F32), "top_loss": np.zeros(B, F32)}
    res_s, res_r = np.zeros((B * H, S), F32), np.zeros((H, B, N), F32)
    assert L.fit.emu_w8pt16_fwd(_p(g1), _p(g2), _p(ones), B * H, S, 1, FIT_FLAGS, 0.0, 0.0, 0.5, _p(got["E_sample"]), _p(res_s), None, None,
                                None) == 0
    wts, E_hb = np.zeros((H, B, N), F32), np.zeros((H, B, 3, 3), F32)
    L.emu_dsac_hyp(0, _p(X), _p(Y), _p(K), _p(got["E_sample"]), B, N, H, case["thresh"], case["beta"], case["loss_kind"], _p(got["soft"]),
                   _p(got["sampson"]), _p(got["score"]), _p(wts), None, None)
    assert L.fit.emu_w8pt16_fwd(_p(pn1), _p(pn2), _p(wts), B, N, H, FIT_FLAGS, 0.0, 0.0, 0.5, _p(E_hb), _p(res_r), None, None, None) == 0
    L.emu_dsac_hyp(1, _p(X), _p(Y), _p(K), _p(E_hb), B, N, H, case["thresh"], case["beta"], case["loss_kind"], None, None, None, None,
                   _p(got["E_refit"]), _p(got["loss"]))
    L.emu_dsac_vote(_p(idx), _p(got["score"]), _p(got["loss"]), case["alpha"], B, N, H, S, _p(got["quality"]), _p(got["counts"]),
                    _p(got["best"]), _p(got["exp_loss"]), _p(got["top_loss"]))
    return got


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def _loop_dsac(X, Y, K, idx, thresh, beta):
    """dsac.py:138-176 as plain float64 loops with formulas of their own (eigh of the normal matrix, per-point Sampson)."""
    N, Ki = len(X), np.linalg.inv(K)

    def kn(P):
        out = np.zeros((len(P), 2))
        for i, p in enumerate(P):
            h = Ki @ np.array([p[0], p[1], 1.0])
            out[i] = np.float32(h[:2] / (h[2] + 1e-10))
        return out

    def e_from(x, y, w):
        def hart(P):
            m = P.mean(0)
            s = math.sqrt(2) / np.mean([math.hypot(*(p - m)) for p in P])
            return np.array([[s, 0, -s * m[0]], [0, s, -s * m[1]], [0, 0, 1]])

        T1, T2 = hart(x), hart(y)
        A = np.zeros((9, 9))
        for p, q, wi in zip(x, y, w):
            a, b = T1 @ [p[0], p[1], 1], T2 @ [q[0], q[1], 1]
            r = wi * np.kron(b, a)
            A += np.outer(r, r)
        f = np.linalg.eigh(A)[1][:, max(0, 9 - len(x))].reshape(3, 3)   # V[:, -1] of the reduced SVD: 9 - n null directions are passed over
        U, _, Vt = np.linalg.svd(f)
        return T2.T @ U @ np.diag([1, 1, 0.0]) @ Vt @ T1

    xn, yn = kn(X), kn(Y)
    Es, softs, dists, Er = [], [], [], []
    for h in range(len(idx)):
        E = e_from(xn[idx[h]], yn[idx[h]], np.ones(len(idx[h])))
        F = Ki.T @ np.float32(E).astype(np.float64) @ Ki
        d = np.zeros(N)
        for n in range(N):
            x, y = np.array([*X[n], 1.0]), np.array([*Y[n], 1.0])
            a, b = F @ x, F.T @ y
            d[n] = (y @ F @ x) ** 2 / (a[0] ** 2 + a[1] ** 2 + b[0] ** 2 + b[1] ** 2)
        with np.errstate(over="ignore"):
            soft = 1 - 1 / (1 + np.exp(-beta * (d - thresh)))
        Es.append(E), dists.append(d), softs.append(soft)
        Er.append(e_from(xn, yn, np.sqrt(np.float32(soft).astype(np.float64)).astype(F32).astype(np.float64)))
    return np.array(Es), np.array(dists), np.array(softs), np.array(Er)


def test_stages_against_plain_loops():
    for case in (dc.make("scene", 1, 24, 3, seed=41, outliers=0.1), dc.make("scene", 1, 17, 2, S=8, seed=42, outliers=0.0)):
        X, Y, K, idx = (case[k].astype(np.float64) if k != "idx" else case[k] for k in ("X", "Y", "K", "idx"))
        Es, d, soft, Er = _loop_dsac(X[0], Y[0], K[0], idx[0], case["thresh"], case["beta"])
        E1, t1 = dr.stage1(case["X"], case["Y"], case["K"], idx)
        for h in range(case["H"]):
            assert dr.unit_diff(E1[0, h], Es[h]) <= 1e-13 * t1[0, h]
        s2 = dr.stage2(E1.astype(F32), case["X"], case["Y"], case["K"], case["thresh"], case["beta"])
        np.testing.assert_allclose(s2["sampson"][0], d, rtol=1e-10)
        np.testing.assert_allclose(s2["soft"][0], soft, rtol=0, atol=1e-12)   # 1 - sigmoid and the single quotient are one function
        np.testing.assert_allclose(s2["score"][0], soft.sum(1), rtol=1e-12)
        E3, t3 = dr.stage3(soft[None].astype(F32), case["X"], case["Y"], case["K"])
        for h in range(case["H"]):
            assert dr.unit_diff(E3[0, h], Er[h]) <= 1e-13 * t3[0, h]
        loss, _ = dr.stage4(E3.astype(F32), case["X"], case["Y"], case["K"], 1)
        assert loss.shape == (1, case["H"]) and (loss > 0).all()
        # the vote: the sequential float32 += of dsac.py:163-165, and the first strict maximum above 0
        sc = s2["score"].astype(F32)
        s5 = dr.stage5(sc, idx, case["N"], loss, 0.1)
        ns, nc = np.zeros((case["N"], 1), F32), np.zeros((case["N"], 1), F32)
        for h in range(case["H"]):
            ns[idx[0, h]] += sc[0, h]
            nc[idx[0, h]] += 1.0
        assert np.array_equal(s5["quality"][0], (ns / (nc + F32(1e-10)))[:, 0]) and s5["best"][0] == int(np.argmax(sc[0]))
        p = np.exp(0.1 * (sc[0].astype(np.float64) - sc[0].max()))
        assert abs(s5["exp_loss"][0] - (p / p.sum() * loss[0]).sum()) <= 1e-12 * abs(s5["exp_loss"][0])
    assert dr.first_best(np.array([0.0, -1.0, np.nan])) == -1 and dr.first_best(np.array([1.0, 3.0, 3.0, 2.0])) == 1


def test_restatement_against_the_reference_golden(golden):
    """The reference's own float32 run (make_golden_dsac.py) against the float64 restatement.  The fixture's yardsticks ARE these
    distances, so what is asserted is (a) that the restatement still gives the stored float64 values, (b) that the distances are
    those of a float32 evaluation and not of another function: a float32 fit leaves its float64 value by about u32 term, term up to
    ~1e3 at these sizes, which moves a Sampson distance by up to ~1e-4 of itself and a weight by beta/4 of that (d up to ~1e2
    where the weight still moves): 1e-3 absolute on the weights, 1e-4 relative on the quality, and (c) the best hypothesis agrees
    wherever the float64 top two scores differ by more than 1e-3."""
    g = golden("dsac")
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    import make_golden_dsac as mk

    for k, case in enumerate(dc.golden_cases()):
        for key in ("X", "Y", "K"):
            assert np.array_equal(g[f"{k}_{key}"], case[key]) and g[f"{k}_{key}"].dtype == F32
        random.seed(case["seed"])
        idx = np.array([random.sample(range(case["N"]), 10) for _ in range(case["hyps"])], np.int32)
        assert np.array_equal(idx, g[f"{k}_idx"])
        f64 = mk.float64_run(case, idx)
        for name in ("inlier_scores", "sampson_dists", "quality", "max_score"):
            np.testing.assert_allclose(f64[name], g[f"{k}_f64_{name}"], rtol=1e-9, atol=1e-12)
        assert float(g[f"{k}_yard_inlier_scores"]) <= 1e-3
        assert float(g[f"{k}_yard_quality"]) <= 1e-4 * float(np.abs(f64["quality"]).max())
        top = np.sort(f64["hyp_scores"])[::-1]
        if top[0] - top[1] > 1e-3:
            assert int(g[f"{k}_best_H_idx"]) == int(f64["best_H_idx"])
        print(f"golden case {k}: yardsticks soft {float(g[f'{k}_yard_inlier_scores']):.3g}, sampson {float(g[f'{k}_yard_sampson_dists']):.3g}, "
              f"quality {float(g[f'{k}_yard_quality']):.3g}, max_score {float(g[f'{k}_yard_max_score']):.3g}")


def test_cap_holds_for_the_restatement_alone():
    """The seeds of the shared cases: at most a quarter of a decided case's hypotheses are undecided, for either fit."""
    for case in dc.all_cases():
        E1, t1 = dr.stage1(case["X"], case["Y"], case["K"], case["idx"])
        s2 = dr.stage2(E1.astype(F32), case["X"], case["Y"], case["K"], case["thresh"], case["beta"])
        _, t3 = dr.stage3(s2["soft"].astype(F32), case["X"], case["Y"], case["K"])
        u1, u3 = int((~np.vectorize(dr.decided)(t1)).sum()), int((~np.vectorize(dr.decided)(t3)).sum())
        print(f"{dc.name_of(case)}: undecided {u1} + {u3} of {t1.size}, largest decided terms {t1[np.vectorize(dr.decided)(t1)].max(initial=0):.3g} "
              f"{t3[np.vectorize(dr.decided)(t3)].max(initial=0):.3g}")
        if case["decided"]:
            assert 4 * u1 <= t1.size and 4 * u3 <= t3.size, dc.name_of(case)
        else:
            assert u3 == t3.size, dc.name_of(case)       # saturated weights: every refit is degenerate


def test_host_build_passes_the_check(emu):
    assert emu.emu_dsac_hyps_per_block() == 4 and emu.emu_dsac_vote_chunk() == 256
    for case in dc.cpu_cases():
        dc.check(case, run_emu(emu, case))


def test_host_build_exact_edges(emu):
    case = next(c for c in dc.edge_cases() if c["name"] == "beta0")
    got = run_emu(emu, case)
    dc.check_beta0(case, got)
    case = next(c for c in dc.edge_cases() if c["name"] == "unsampled")
    got = run_emu(emu, case)
    never = np.ones(case["N"], bool)
    never[case["idx"][0].ravel()] = False
    assert never.sum() >= case["N"] - case["H"] * case["S"] > 0
    assert (got["counts"][0][never] == 0).all() and (got["quality"][0][never] == 0).all() and (got["counts"][0][~never] >= 1).all()
    case = next(c for c in dc.edge_cases() if c["name"] == "saturated")
    got = run_emu(emu, case)
    assert (got["score"] == 0).all() and (got["best"] == -1).all() and (got["top_loss"] == 0).all()   # all scores 0
    assert all(np.isfinite(got[k]).all() for k in ("E_sample", "E_refit", "loss", "quality", "exp_loss"))


def test_a_nan_stays_in_its_pair(emu):
    case = dc.make("scene", 3, 20, 3, seed=51)
    bad = dict(case, X=case["X"].copy())
    bad["X"][1, 7, 0] = np.nan
    a, b = run_emu(emu, case), run_emu(emu, bad)
    for k in dc.OUT_KEYS:
        assert np.array_equal(a[k][[0, 2]], b[k][[0, 2]], equal_nan=True), k


# ---- the C ABI: refusals before any HIP call, the workspace and the getters ------------------------------------------------------------
def _addr(align=0):
    buf = ctypes.create_string_buffer(64)  # host memory: only looked at, never dereferenced before the refusals
    _addr.keep.append(buf)
    return (ctypes.addressof(buf) + 15) // 16 * 16 + align


_addr.keep = []


def test_symbols_version_and_getters(dfepe, emu):
    L = dfepe._lib.lib()
    raw = ctypes.CDLL(dfepe.LIB_PATH)
    for name in ("dfepe_dsac", "dfepe_dsac_workspace_bytes", "dfepe_dsac_hyps_per_block", "dfepe_dsac_vote_chunk", "dfepe_dsac_vote_tile"):
        assert hasattr(raw, name) and name in dfepe.EXPORTED_SYMBOLS
    assert L.dfepe_version() == 154
    assert L.dfepe_dsac_hyps_per_block() == emu.emu_dsac_hyps_per_block() and L.dfepe_dsac_vote_chunk() == emu.emu_dsac_vote_chunk()
    T = L.dfepe_dsac_vote_tile()
    assert T == emu.emu_dsac_vote_tile() and {T - 1, T, T + 1} <= {c["H"] for c in dc.all_cases()}   # 15, 16, 17 hypotheses


def test_workspace_bytes(dfepe):
    L = dfepe._lib.lib()
    r4 = lambda n: (n + 3) // 4 * 4  # noqa: E731
    for B, N, H, S in ((1, 10, 1, 10), (3, 129, 5, 8), (2, 1000, 64, 16), (7, 33, 3, 9)):
        want = 4 * (2 * r4(B * N * 3) + 2 * r4(B * H * S * 3) + 2 * r4(B * H * S) + 2 * r4(B * H * N) + r4(B * H * 9))
        assert L.dfepe_dsac_workspace_bytes(B, N, H, S) == want, (B, N, H, S)
    for bad in ((0, 10, 1, 10), (1, 0, 1, 10), (1, 10, 0, 10), (1, 10, 1, 7), (1, 20, 1, 17), (-1, 10, 1, 10)):
        assert L.dfepe_dsac_workspace_bytes(*bad) == 0


def test_refusals_without_a_launch(dfepe):
    L = dfepe._lib.lib()
    a = _addr()
    names = ("X", "Y", "K", "idx", "E_sample", "soft", "sampson", "score", "E_refit", "loss", "quality", "counts", "best", "exp_loss",
             "top_loss", "ws")

    def call(B=2, N=20, H=3, S=10, kind=1, **ptr):
        q = {n: ptr.get(n, a) for n in names}
        return L.dfepe_dsac(None, q["X"], q["Y"], q["K"], q["idx"], B, N, H, S, 100.0, 0.02, 0.1, kind, q["E_sample"], q["soft"],
                            q["sampson"], q["score"], q["E_refit"], q["loss"], q["quality"], q["counts"], q["best"], q["exp_loss"],
                            q["top_loss"], q["ws"])

    assert call(B=-1) == INVALID and call(N=-1) == INVALID and call(H=0) == INVALID and call(H=-2) == INVALID
    assert call(S=7) == INVALID and call(S=17, N=40) == INVALID and call(N=9) == INVALID and call(N=15, S=16) == INVALID
    assert call(kind=-1) == INVALID and call(kind=3) == INVALID
    assert call(B=0) == 0 and call(B=0, X=None, ws=None) == 0                    # nothing to do: before the pointer checks
    assert call(B=0, S=7) == INVALID and call(B=0, kind=5) == INVALID and call(B=0, N=5) == INVALID   # the documented order
    for n in names:
        want = 0 if n in ("soft", "sampson", "exp_loss", "top_loss") else INVALID
        if want == INVALID:
            assert call(**{n: None}) == INVALID, n
    assert call(X=_addr(4)) == INVALID and call(Y=_addr(4)) == INVALID and call(ws=_addr(8)) == INVALID
    assert call(B=4, N=2 ** 29, H=2) == UNSUPPORTED and call(B=1, N=2 ** 20, H=2 ** 12) == UNSUPPORTED


def test_python_layer_refuses_cpu_tensors_and_bad_arguments(dfepe):
    import torch

    X, K, idx = torch.zeros(2, 20, 2), torch.eye(3).expand(2, 3, 3), torch.zeros(2, 3, 10, dtype=torch.int32)
    with pytest.raises(dfepe.DfepeError):
        dfepe.ops.dsac(X, X, K, idx, 100.0, 0.02)
    with pytest.raises(dfepe.DfepeError):
        dfepe.compat.dsac_batch(X, X, K, 3, 100.0, 0.02, seed=1)
    d = dfepe.compat.DSAC(4, 100.0, 0.02, 0.1, torch.eye(3), dfepe.compat.H_loss.HLoss())
    with pytest.raises(ValueError):
        d(torch.zeros(9, 2), torch.zeros(9, 2), None)                     # random.sample(range(9), 10)
    with pytest.raises(NotImplementedError):
        d(torch.zeros(20, 2, requires_grad=True), torch.zeros(20, 2), None)
    with pytest.raises(NotImplementedError):
        d(torch.zeros(20, 2), torch.zeros(20, 2, requires_grad=True), None)
    assert dfepe.compat.DSAC is dfepe.compat.dsac.DSAC and dfepe.compat.dsac_batch is dfepe.compat.dsac.dsac_batch


def test_seeded_draw_is_the_references(dfepe, golden):
    """A seeded compat.DSAC samples what the reference sampled: the index lists of the fixture, replayed through the mirror's draw."""
    g = golden("dsac")
    for k, case in enumerate(dc.golden_cases()):
        random.seed(case["seed"])
        assert dfepe.compat.dsac._draw(case["N"], case["hyps"], dfepe.compat.dsac.SAMPLE) == g[f"{k}_idx"].tolist()
