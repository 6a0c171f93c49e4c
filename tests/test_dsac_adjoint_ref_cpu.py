"""The adjoint of the DSAC loop without a GPU: the `pure` float64 restatement (tests/dsac_adjoint_ref.py) against the reference's own
float64 autograd (tests/golden/dsac_adjoint.npz) and against central differences; the host build of csrc/dsac_adjoint_math.h
(tests/emu/emu_dsac_adjoint.cpp, chained with the host build of the fit adjoint the way dfepe_dsac_bwd chains its launches) through the
same check() as the GPU; and the C ABI's workspace formula and refusals, which are made before any HIP call."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dsac_adjoint_cases as ac  # noqa: E402
import dsac_adjoint_ref as ar  # noqa: E402
import dsac_cases as dc  # noqa: E402
import test_dsac_ref_cpu as fwd_cpu  # noqa: E402  (run_emu: the host build of the forward)

REPO = fwd_cpu.REPO
EMU_DIR, CSRC = fwd_cpu.EMU_DIR, fwd_cpu.CSRC
F32 = np.float32
INVALID, UNSUPPORTED = -1, -3
FIT_FLAGS = 4 | 8 | 16
_p = fwd_cpu._p


def _forward_emu():
    out = os.path.join(EMU_DIR, "_build")
    os.makedirs(out, exist_ok=True)
    L = fwd_cpu._build(os.path.join(out, "libemu_dsac.so"),
                       [os.path.join(EMU_DIR, "emu_dsac.cpp"), os.path.join(CSRC, "dsac_math.h"), os.path.join(CSRC, "epi_adjoint_math.h")],
                       ["-ffp-contract=off", f"-I{CSRC}"])
    fit = fwd_cpu._build(os.path.join(out, "libemu_w8pt16.so"),
                         [os.path.join(EMU_DIR, "emu_w8pt16.cpp"), os.path.join(EMU_DIR, "rowgroup.h")] +
                         [os.path.join(CSRC, f) for f in ("w8pt16_body.h", "w8pt16_bwd_body.h", "loss_tail_body.h", "pose_math.h", "dfepe_math.h",
                                                          "fit_plan.h")] + [os.path.join(REPO, "include", "dfepe.h")],
                         [f"-I{EMU_DIR}", f"-I{CSRC}", f"-I{REPO}/include"])
    i, p, fl, u = ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_uint
    L.emu_dsac_prep.argtypes = [p, p, p, p, i, i, i, i, p, p, p, p, p]
    L.emu_dsac_hyp.argtypes = [i, p, p, p, p, i, i, i, fl, fl, i, p, p, p, p, p, p]
    L.emu_dsac_vote.argtypes = [p, p, p, fl, i, i, i, i, p, p, p, p, p]
    L.emu_dsac_prep.restype = L.emu_dsac_hyp.restype = L.emu_dsac_vote.restype = None
    fit.emu_w8pt16_fwd.restype = i
    fit.emu_w8pt16_fwd.argtypes = [p, p, p, i, i, i, u, fl, fl, fl, p, p, p, p, p]
    L.fit = fit
    return L


@pytest.fixture(scope="module")
def emu():
    out = os.path.join(EMU_DIR, "_build")
    os.makedirs(out, exist_ok=True)
    A = fwd_cpu._build(os.path.join(out, "libemu_dsac_adjoint.so"),
                       [os.path.join(EMU_DIR, "emu_dsac_adjoint.cpp")] +
                       [os.path.join(CSRC, f) for f in ("dsac_adjoint_math.h", "dsac_math.h", "epi_adjoint_math.h")],
                       ["-ffp-contract=off", f"-I{CSRC}"])
    E = fwd_cpu._build(os.path.join(out, "libemu_eight_point_adjoint.so"),
                       [os.path.join(EMU_DIR, "emu_eight_point_adjoint.cpp"), os.path.join(CSRC, "eight_point_adjoint_math.h")],
                       ["-ffp-contract=off", f"-I{CSRC}"])
    i, p, fl, u = ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_uint
    A.emu_dsac_bwd_prep.argtypes = [p] * 7 + [i] * 5 + [p] * 8
    A.emu_dsac_bwd_head.argtypes = [p] * 8 + [fl, i, i, i, i, p, p]
    A.emu_dsac_bwd_hyp.argtypes = [i] + [p] * 9 + [fl, i, i, i, i, p, p]
    A.emu_dsac_bwd_points.argtypes = [p] * 15 + [fl, i, i, i, i, i, p, p]
    A.emu_dsac_bwd_prep.restype = A.emu_dsac_bwd_head.restype = A.emu_dsac_bwd_hyp.restype = A.emu_dsac_bwd_points.restype = None
    E.emu_eight_point_bwd.restype = i
    E.emu_eight_point_bwd.argtypes = [p, p, p, i, i, i, u, p, p, p, p, p]
    A.e8 = E
    A.fwd = _forward_emu()
    return A


FWD_KEYS = ("E_sample", "soft", "score", "E_refit", "loss", "counts")


def run_emu(A, case, fwd=None, want_x=True, want_y=True):
    """The launches of dfepe_dsac_bwd on the host, on the host build's own forward.  Returns (fwd, got) as check() takes them."""
    B, N, H, S = case["B"], case["N"], case["H"], case["S"]
    X, Y, K, idx = (np.ascontiguousarray(case[k]) for k in ("X", "Y", "K", "idx"))
    if fwd is None:
        fwd = fwd_cpu.run_emu(A.fwd, case)
    fwd = {k: np.ascontiguousarray(fwd[k]) for k in FWD_KEYS}
    up = {k: np.ascontiguousarray(v) for k, v in ac.upstreams(case).items()}
    z = lambda *s: np.zeros(s, F32)  # noqa: E731
    pn1, pn2, g1, g2, wts, E_hb = z(B, N, 2), z(B, N, 2), z(B * H, S, 2), z(B * H, S, 2), z(H, B, N), z(H, B, 9)
    Fd, Md = np.zeros((B, H, 9)), np.zeros((B, H, 9))
    A.emu_dsac_bwd_prep(_p(X), _p(Y), _p(K), _p(idx), _p(fwd["soft"]), _p(fwd["E_sample"]), _p(fwd["E_refit"]), B, N, H, S, case["loss_kind"],
                        _p(pn1), _p(pn2), _p(g1), _p(g2), _p(wts), _p(E_hb), _p(Fd), _p(Md))
    got = {"t_score": z(B, H), "t_loss": z(B, H), "t_E_refit": z(B, H, 3, 3), "t_w": z(H, B, N), "t_E_sample": z(B, H, 3, 3),
           "gpn1": z(B, N, 2), "gpn2": z(B, N, 2), "gg1": z(B, H, S, 2), "gg2": z(B, H, S, 2), "g_X": z(B, N, 2) if want_x else None,
           "g_Y": z(B, N, 2) if want_y else None}
    A.emu_dsac_bwd_head(_p(idx), _p(fwd["score"]), _p(fwd["loss"]), _p(fwd["counts"]), _p(up.get("score")), _p(up.get("loss")),
                        _p(up.get("quality")), _p(up.get("exp_loss")), case["alpha"], B, N, H, S, _p(got["t_score"]), _p(got["t_loss"]))
    tE_hb = z(H, B, 9)
    A.emu_dsac_bwd_hyp(1, _p(X), _p(Y), _p(K), _p(up.get("E_refit")), _p(Md), _p(got["t_loss"]), None, None, None, case["beta"],
                       case["loss_kind"], B, N, H, _p(got["t_E_refit"]), _p(tE_hb))
    assert A.e8.emu_eight_point_bwd(_p(pn1), _p(pn2), _p(wts), B, N, H, FIT_FLAGS, _p(E_hb), _p(tE_hb), _p(got["gpn1"]), _p(got["gpn2"]),
                                    _p(got["t_w"])) == 0
    A.emu_dsac_bwd_hyp(0, _p(X), _p(Y), _p(K), _p(up.get("E_sample")), _p(Fd), _p(got["t_score"]), _p(fwd["soft"]), _p(wts), _p(got["t_w"]),
                       case["beta"], case["loss_kind"], B, N, H, _p(got["t_E_sample"]), None)
    assert A.e8.emu_eight_point_bwd(_p(g1), _p(g2), None, B * H, S, 1, FIT_FLAGS, _p(fwd["E_sample"]), _p(got["t_E_sample"]), _p(got["gg1"]),
                                    _p(got["gg2"]), None) == 0
    A.emu_dsac_bwd_points(_p(X), _p(Y), _p(K), _p(idx), _p(fwd["soft"]), _p(wts), _p(got["t_w"]), _p(got["t_score"]), _p(got["t_loss"]),
                          _p(Fd), _p(Md), _p(got["gpn1"]), _p(got["gpn2"]), _p(got["gg1"]), _p(got["gg2"]), case["beta"], case["loss_kind"],
                          B, N, H, S, _p(got["g_X"]), _p(got["g_Y"]))
    return fwd, got


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def test_settings_hold_for_the_restatement_alone():
    """The seeds, beta and outlier shares of the size cases: every hypothesis decided, and exact-zero float32 weights where promised."""
    with_zeros = 0
    for case in ac.size_cases():
        fwd = ac.restated_forward(case)
        gs, gr = ac.gaps(case, fwd)
        zeros = int((fwd["soft"] == 0).sum())
        print(f"{ac.name_of(case)}: smallest gaps {gs.min():.3g} (sample) {gr.min():.3g} (refit), exact-zero weights {zeros} of {fwd['soft'].size}")
        assert gs.min() >= ac.MIN_GAP and gr.min() >= ac.MIN_GAP, ac.name_of(case)
        assert (zeros > 0) or not case["zeros"], ac.name_of(case)
        with_zeros += zeros > 0
    assert with_zeros >= 3
    sizes = {(c["B"], c["N"], c["H"], c["S"], c["loss_kind"]) for c in ac.size_cases()}
    assert sizes == {(1, 8, 2, 8, 1), (1, 10, 3, 8, 1), (3, 11, 1, 10, 1), (1, 16, 2, 16, 1), (3, 17, 4, 16, 1), (1, 63, 15, 10, 1),
                     (3, 64, 16, 10, 2), (1, 65, 17, 10, 1), (3, 129, 5, 10, 1), (1, 64, 65, 10, 2), (1, 255, 2, 10, 1), (3, 256, 3, 8, 1),
                     (1, 257, 5, 10, 1)}
    ups = [c["up"] for c in ac.size_cases()]
    assert ("exp_loss",) in ups and ("quality",) in ups and ac.ALL_UP in ups


def _objective(case, up, X, Y, frozen):
    f = ar.pure_forward(X, Y, case["K"], case["idx"], case["thresh"], case["beta"], case["alpha"], case["loss_kind"], frozen)
    # the fits' sign is a gauge: only sign-invariant outputs enter the objective
    return sum(float((np.asarray(up[k], np.float64) * f[k]).sum()) for k in up)


@pytest.mark.parametrize("name", ["plain", "zero_weights"])
def test_pure_gradient_against_central_differences(name):
    """The `pure` gradient of sum(upstream . outputs) over score, loss, quality and exp_loss against central differences of the `pure`
    forward with every fit's Hartley transforms held at their values (they are constants of the adjoint, as of the reference's autograd).
    `zero_weights` runs at the reference's beta = 0.02 with gross outliers, where the float64 weights are tiny but positive
    and the reference's own autograd returns NaN: this holds the limit rule d sqrt(s)/dd = -(beta/2) sqrt(s)(1 - s) there.
    The step is 1e-4 px; the differences of a function with second derivatives of order 1 are then accurate to about 1e-8 + 1e-16 /
    1e-4 relative, and 1e-5 of the largest entry leaves three digits for the conditioning of the fits."""
    case = (ac.make("scene", 1, 12, 3, seed=43, outliers=0.0, beta=0.002) if name == "plain"
            else ac.make("zero_weights", 1, 14, 3, seed=44, outliers=0.2, beta=0.02))
    up = {k: v for k, v in ac.upstreams(dict(case, up=ac.ALL_UP)).items() if k in ("score", "loss", "quality", "exp_loss")}
    X, Y = case["X"].astype(np.float64), case["Y"].astype(np.float64)
    gX, gY, f = ar.pure_gradient(X, Y, case["K"], case["idx"], case["thresh"], case["beta"], case["alpha"], case["loss_kind"], up)
    assert np.isfinite(gX).all() and np.isfinite(gY).all()
    if name == "zero_weights":
        assert (f["soft"] > 0).all() and f["soft"].min() < 1e-17, f["soft"].min()   # below where 1 - sigmoid cancels to 0 in float64
    h = 1e-4
    for P, g, which in ((X, gX, "X"), (Y, gY, "Y")):
        num = np.zeros_like(g)
        for n in range(case["N"]):
            for k in range(2):
                Pp, Pm = P.copy(), P.copy()
                Pp[0, n, k] += h
                Pm[0, n, k] -= h
                a = _objective(case, up, *((Pp, Y) if which == "X" else (X, Pp)), f["T"])
                b = _objective(case, up, *((Pm, Y) if which == "X" else (X, Pm)), f["T"])
                num[0, n, k] = (a - b) / (2 * h)
        err, top = np.abs(num - g).max(), np.abs(num).max()
        print(f"{name}: g_{which} against central differences: {err / top:.3g} of the largest entry {top:.3g}")
        assert err <= 1e-5 * top, (name, which, err, top)


def test_pure_restatement_against_the_reference_golden(golden):
    """tests/golden/dsac_adjoint.npz: the reference's DSAC + HLoss, float64 and float32 autograd of exp_loss and of sum c_n quality_n.
    The pure restatement must be at least 1000 times closer to the reference's float64 gradient than the reference's own float32
    gradient is: both are float64 evaluations of one function, and the factor leaves six of float64's nine extra digits to
    conditioning.  The last case stores only the fact that the reference's gradient is not finite at its own settings; there the
    restatement is finite."""
    g = golden("dsac_adjoint")
    n = int(g["n_cases"])
    for k in range(n):
        X, Y, K, idx = g[f"{k}_X"][None], g[f"{k}_Y"][None], g[f"{k}_K"][None], g[f"{k}_idx"][None]
        thresh, beta, alpha = float(g[f"{k}_thresh"]), float(g[f"{k}_beta"]), float(g[f"{k}_alpha"])
        for what, up in (("exp_loss", {"exp_loss": np.ones(1)}), ("quality", {"quality": g[f"{k}_c"][None].astype(np.float64)})):
            gX, gY, _ = ar.pure_gradient(X.astype(np.float64), Y.astype(np.float64), K, idx, thresh, beta, alpha, 1, up)
            assert np.isfinite(gX).all() and np.isfinite(gY).all()
            if not bool(g[f"{k}_finite"]):
                continue
            for ours, key in ((gX[0], "gX"), (gY[0], "gY")):
                truth, yard = g[f"{k}_{what}_{key}"], float(g[f"{k}_{what}_yard_{key}"])
                dist = float(np.abs(ours - truth).max())
                print(f"golden case {k} {what} {key}: pure - reference float64 {dist:.3g}, reference float32 - float64 {yard:.3g}")
                assert 1000 * dist <= yard, (k, what, key, dist, yard)
    assert not bool(g[f"{n - 1}_finite"]) and float(g[f"{n - 1}_beta"]) == 0.02


# ---- the host build ----------------------------------------------------------------------------------------------------------------------
CPU_CASES = ac.cpu_cases()


@pytest.mark.parametrize("k", range(len(CPU_CASES)), ids=[ac.name_of(c) for c in CPU_CASES])
def test_host_build_passes_the_check(emu, k):
    case = CPU_CASES[k]
    fwd, got = run_emu(emu, case)
    ac.check(case, fwd, got)


def test_host_build_constants_and_null_outputs(emu):
    assert emu.emu_dsac_bwd_point_lanes() == 64 and emu.emu_dsac_bwd_point_waves() == 4
    assert {c["H"] for c in ac.all_cases()} >= {1, 2, 3, 4, 5, 15, 16, 17, 65}      # around a quarter split and a workgroup's share
    case = CPU_CASES[4]
    fwd, a = run_emu(emu, case)
    _, b = run_emu(emu, case, fwd=fwd, want_y=False)
    _, c = run_emu(emu, case, fwd=fwd, want_x=False)
    assert np.array_equal(a["g_X"], b["g_X"]) and np.array_equal(a["g_Y"], c["g_Y"])


def test_a_nan_stays_in_its_pair(emu):
    case = ac.make("scene", 3, 20, 3, seed=51, beta=0.002)
    bad = dict(case, X=case["X"].copy())
    bad["X"][1, 7, 0] = np.nan
    (_, a), (_, b) = run_emu(emu, case), run_emu(emu, bad)
    for k in ("g_X", "g_Y", "t_score", "t_loss", "t_E_refit", "t_E_sample"):
        assert np.array_equal(a[k][[0, 2]], b[k][[0, 2]]), k
    assert np.array_equal(a["t_w"][:, [0, 2]], b["t_w"][:, [0, 2]])


# ---- the C ABI: the workspace and the refusals before any HIP call -----------------------------------------------------------------------
workspace_floats = ac.workspace_floats


def test_workspace_bytes(dfepe):
    L = dfepe._lib.lib()
    for B, N, H, S in ((1, 10, 1, 10), (3, 129, 5, 8), (2, 1000, 64, 16), (7, 33, 3, 9)):
        assert L.dfepe_dsac_bwd_workspace_bytes(B, N, H, S) == 4 * workspace_floats(B, N, H, S)[0], (B, N, H, S)
        assert L.dfepe_eight_point_bwd_workspace_bytes(B, N, H) == (32 * B * H * N if H > 1 else 0)
    for bad in ((0, 10, 1, 10), (1, 0, 1, 10), (1, 10, 0, 10), (1, 10, 1, 7), (1, 20, 1, 17), (-1, 10, 1, 10)):
        assert L.dfepe_dsac_bwd_workspace_bytes(*bad) == 0


def test_symbols_and_version(dfepe):
    raw = ctypes.CDLL(dfepe.LIB_PATH)
    for name in ("dfepe_dsac_bwd", "dfepe_dsac_bwd_workspace_bytes"):
        assert hasattr(raw, name) and name in dfepe.EXPORTED_SYMBOLS
    assert dfepe._lib.lib().dfepe_version() == 154


def test_refusals_without_a_launch(dfepe):
    L = dfepe._lib.lib()
    a = fwd_cpu._addr()
    fwd_names = ("X", "Y", "K", "idx", "E_sample", "soft", "score", "E_refit", "loss", "counts")
    ups = ("g_E_sample", "g_score", "g_E_refit", "g_loss", "g_quality", "g_exp_loss")
    totals = ("t_score", "t_loss", "t_E_refit", "t_w", "t_E_sample")
    names = fwd_names + ups + ("g_X", "g_Y") + totals + ("ws",)

    def call(B=2, N=20, H=3, S=10, kind=1, **ptr):
        q = {n: ptr.get(n, a) for n in names}
        return L.dfepe_dsac_bwd(None, q["X"], q["Y"], q["K"], q["idx"], B, N, H, S, 100.0, 0.02, 0.1, kind,
                                *(q[n] for n in fwd_names[4:]), *(q[n] for n in ups), q["g_X"], q["g_Y"], *(q[n] for n in totals), q["ws"])

    none_up = {n: None for n in ups}
    assert call(B=-1) == INVALID and call(N=-1) == INVALID and call(H=0) == INVALID and call(H=-2) == INVALID
    assert call(S=7) == INVALID and call(S=17, N=40) == INVALID and call(N=9) == INVALID and call(N=15, S=16) == INVALID
    assert call(kind=-1) == INVALID and call(kind=3) == INVALID
    assert call(B=0) == 0 and call(B=0, X=None, ws=None, g_X=None, g_Y=None, **none_up) == 0   # nothing to do: before the pointer checks
    assert call(B=0, S=7) == INVALID and call(B=0, kind=5) == INVALID and call(B=0, N=5) == INVALID   # the documented order
    for n in fwd_names + ("ws",):
        assert call(**{n: None}) == INVALID, n
    assert call(**none_up) == INVALID
    assert call(g_X=None, g_Y=None) == INVALID
    big = dict(B=4, N=2 ** 29, H=2)                                                   # UNSUPPORTED comes last:
    assert call(**big) == UNSUPPORTED and call(B=1, N=2 ** 20, H=2 ** 12) == UNSUPPORTED
    assert call(X=None, **big) == INVALID and call(**none_up, **big) == INVALID and call(g_X=None, g_Y=None, **big) == INVALID
    for n in ("X", "Y", "g_X", "g_Y"):
        assert call(**{n: fwd_cpu._addr(4)}) == INVALID and call(**{n: fwd_cpu._addr(4)}, **big) == INVALID, n
    assert call(ws=fwd_cpu._addr(8)) == INVALID
    # what may be NULL: each upstream alone, either output, every total -- refused by nothing above, so the size check is reached
    for n in ups:
        assert call(**{m: None for m in ups if m != n}, **big) == UNSUPPORTED, n
    assert call(g_X=None, **big) == UNSUPPORTED and call(g_Y=None, **big) == UNSUPPORTED
    assert call(**{n: None for n in totals}, **big) == UNSUPPORTED


def test_python_layer_refusals(dfepe):
    import torch

    X, K, idx = torch.zeros(2, 20, 2), torch.eye(3).expand(2, 3, 3).contiguous(), torch.zeros(2, 3, 10, dtype=torch.int32)
    with pytest.raises(dfepe.DfepeError):
        dfepe.ops.dsac(X.clone().requires_grad_(), X, K, idx, 100.0, 0.02)
    with pytest.raises(dfepe.DfepeError):
        dfepe.compat.dsac_batch(X.clone().requires_grad_(), X, K, 3, 100.0, 0.02, seed=1)
    with pytest.raises(NotImplementedError, match="gradient to K"):
        dfepe.ops.dsac(X, X, K.clone().requires_grad_(), idx, 100.0, 0.02)
    d = dfepe.compat.DSAC(4, 100.0, 0.02, 0.1, torch.eye(3), lambda E, X, Y: 0.0)
    with pytest.raises(NotImplementedError, match="HLoss"):
        d.expected_loss(torch.zeros(20, 2), torch.zeros(20, 2))
    d = dfepe.compat.DSAC(4, 100.0, 0.02, 0.1, torch.eye(3), None)
    with pytest.raises(NotImplementedError):
        d.expected_loss(torch.zeros(20, 2), torch.zeros(20, 2))
    d = dfepe.compat.DSAC(4, 100.0, 0.02, 0.1, torch.eye(3), dfepe.compat.H_loss.HLoss())
    with pytest.raises(ValueError):
        d.expected_loss(torch.zeros(9, 2), torch.zeros(9, 2))                     # random.sample(range(9), 10)
