"""The adjoints of the epipolar distances without a GPU: the fp64 restatement (tests/epi_adjoint_ref.py) against the reference's own
float64 autograd (tests/golden/epi_adjoint.npz), against its 50-digit twin, and the host build of csrc/epi_adjoint_math.h
(tests/emu/emu_epi_adjoint.cpp, compiled with g++) through the same check() as the GPU; the constant of the bound is measured here.
The C ABI's refusals are made before any HIP call, so they are tested here too."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epi_adjoint_cases as ac  # noqa: E402
import epi_adjoint_ref as ar  # noqa: E402

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EMU_DIR = os.path.join(REPO, "tests", "emu")
CSRC = os.path.join(REPO, "pytorch-deepfepe_amd", "csrc")
F32 = np.float32
INVALID, UNSUPPORTED = -1, -3
HOMO = 8


@pytest.fixture(scope="module")
def cases():
    return ac.cpu_cases()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(REPO, "tests", "golden", "epi_adjoint.npz"))


@pytest.fixture(scope="module")
def emu():
    out = os.path.join(EMU_DIR, "_build")
    os.makedirs(out, exist_ok=True)
    lib = os.path.join(out, "libemu_epi_adjoint.so")
    srcs = [os.path.join(EMU_DIR, "emu_epi_adjoint.cpp"), os.path.join(CSRC, "epi_adjoint_math.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", f"-I{CSRC}", srcs[0], "-o", lib], check=True)
    L = ctypes.CDLL(lib)
    fl = ctypes.c_float
    i, p = ctypes.c_int, ctypes.c_void_p
    L.emu_epi_metrics_bwd.argtypes = [i, p, p, p, i, i, fl, fl, p, p, p, p]
    L.emu_epi_loss_fwd.argtypes = [i, p, p, p, p, i, i, fl, fl, p]
    L.emu_epi_loss_bwd.argtypes = [i, p, p, p, p, i, i, fl, fl, p, p, p, p, p]
    L.emu_epi_residual_bwd_pts.argtypes = [p, p, p, i, i, fl, p, p, p]
    L.emu_epi_point_terms.argtypes = [i, p, p, p, i, i, fl, fl, p, p, p, p, p]
    L.emu_epi_residual_point_terms.argtypes = [p, p, p, i, i, fl, p, p, p]
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _cl(case):
    return -1.0 if case["clamp_at"] is None else case["clamp_at"]


def _kind(case):
    return case["kind"] | (HOMO if case["homo"] else 0)


def run_emu(L, case, want=("g_F", "g_X", "g_Y")):
    B, N = case["B"], case["N"]
    got = {"g_F": np.full((B, 3, 3), -7, F32) if "g_F" in want else None,
           "g_X": np.full(case["X"].shape, -7, F32) if "g_X" in want else None,
           "g_Y": np.full(case["Y"].shape, -7, F32) if "g_Y" in want else None}
    if case["op"] == "residual":
        rc = L.emu_epi_residual_bwd_pts(_p(case["X"]), _p(case["Y"]), _p(case["F"]), B, N, case["clamp_at"], _p(case["g"]), _p(got["g_X"]),
                                        _p(got["g_Y"]))
        got["g_F"] = None
    else:
        rc = L.emu_epi_metrics_bwd(_kind(case), _p(case["F"]), _p(case["X"]), _p(case["Y"]), B, N, _cl(case), case["eps"], _p(case["g"]),
                                   _p(got["g_F"]), _p(got["g_X"]), _p(got["g_Y"]))
    assert rc == 0
    return got


def host_fp64(L, case):
    """The host build's per-point values before they are rounded to fp32."""
    B, N = case["B"], case["N"]
    if case["op"] == "residual":
        g1, g2 = np.zeros((B, N, 3)), np.zeros((B, N, 3))
        L.emu_epi_residual_point_terms(_p(case["X"]), _p(case["Y"]), _p(case["F"]), B, N, case["clamp_at"], _p(case["g"]), _p(g1), _p(g2))
        return {"g1": g1, "g2": g2}
    value = np.zeros((3 if case["kind"] == 2 else 1, B, N))
    gF, gX, gY = np.zeros((B, N, 9)), np.zeros((B, N, 3)), np.zeros((B, N, 3))
    L.emu_epi_point_terms(_kind(case), _p(case["F"]), _p(case["X"]), _p(case["Y"]), B, N, _cl(case), case["eps"], _p(case["g"]), _p(value),
                          _p(gF), _p(gX), _p(gY))
    return {"value": value, "gF_pt": gF, "gX": gX, "gY": gY}


def _exact(case):
    if case["op"] == "residual":
        return ar.mp_residual(case["X"], case["Y"], case["F"], case["clamp_at"], case["g"])
    return ar.mp_metrics(case["kind"], case["F"], case["X"], case["Y"], case["homo"], case["g"], case["clamp_at"], case["eps"])


def _pairs(case, r, vals):
    """(values, M) per output name, shaped like the twin's flat lists."""
    if case["op"] == "residual":
        return {"g1": (vals["g1"], r.M1), "g2": (vals["g2"], r.M2)}
    return {"value": (vals["value"], r.vmag), "gF_pt": (vals["gF_pt"], r.MF_pt), "gX": (vals["gX"], r.MX), "gY": (vals["gY"], r.MY)}


@pytest.fixture(scope="module")
def twins(cases):
    return [_exact(c) for c in cases]


def test_host_arithmetic_within_the_measured_constant(emu, cases, twins):
    """Measures c: the smallest value with |host fp64 - exact| <= c 2^-53 M over every output of every shared case."""
    import mpmath as mp

    worst = 0.0
    for case, exact in zip(cases, twins):
        r, host = ac.reference(case), host_fp64(emu, case)
        for name, (vals, M) in _pairs(case, r, host).items():
            w = ar.worst_ratio(vals, exact[name], M, mp)
            assert w <= ar.C_MEASURED, (ac.name_of(case), name, w)
            worst = max(worst, w)
    print(f"host build against the 50-digit twin: largest |host - exact| / (2^-53 M) = {worst:.3f} (C_MEASURED = {ar.C_MEASURED})")


def test_restatement_within_the_bound_of_its_twin(cases, twins):
    import mpmath as mp

    worst = 0.0
    for case, exact in zip(cases, twins):
        r = ac.reference(case)
        if case["op"] == "residual":
            vals = {"g1": r.g1, "g2": r.g2}
        else:
            vals = {"value": r.value, "gF_pt": r.gF_pt, "gX": r.gX, "gY": r.gY}
        for name, (v, M) in _pairs(case, r, vals).items():
            w = ar.worst_ratio(v, exact[name], M, mp)
            assert w <= ar.C, (ac.name_of(case), name, w)
            worst = max(worst, w)
    print(f"restatement against the 50-digit twin: largest ratio {worst:.3f}")


def test_restatement_reproduces_the_reference(golden):
    """Values and the reference's own float64 autograd, batched and 2-D, within C_GOLDEN 2^-53 M (2^-53 N sum T more for g_F)."""
    worst = 0.0
    for k, case in enumerate(ac.golden_cases()):
        for key in ("F", "X", "Y", "g"):
            assert np.array_equal(golden[f"{k}_{key}"], case[key]) and golden[f"{k}_{key}"].dtype == F32
        forms = [("", slice(None))] if case["kind"] == 3 else [("", slice(None)), ("2", slice(0, 1))]
        for suffix, sel in forms:
            g = case["g"][:, sel] if case["kind"] == 2 else case["g"][sel]
            if case["op"] == "residual":
                r = ar.residual_adjoint(case["X"][sel], case["Y"][sel], case["F"][sel], case["clamp_at"], g)
                parts = [(r.g1, r.M1, golden[f"{k}_gX"]), (r.g2, r.M2, golden[f"{k}_gY"])]
                assert not r.flagged.any()
            else:
                eps = case["eps"] if suffix == "" else 0.0
                r = ar.metrics_adjoint(case["kind"], case["F"][sel], case["X"][sel], case["Y"][sel], case["homo"], g, case["clamp_at"], eps,
                                       eps32=False)
                assert not r.flagged.any()
                sd = 3 if case["homo"] else 2
                shp = (lambda a: a) if suffix == "" else (lambda a: a[None])
                gold_v = golden[f"{k}_value{suffix}"]
                gold_v = gold_v if suffix == "" else (gold_v[:, None] if case["kind"] == 2 else gold_v[None])
                parts = [(r.value, r.vmag, gold_v), (r.gX[..., :sd], r.MX[..., :sd], shp(golden[f"{k}_gX{suffix}"])),
                         (r.gY[..., :sd], r.MY[..., :sd], shp(golden[f"{k}_gY{suffix}"])),
                         (r.gF, r.MF + r.N * r.TF / ar.C_GOLDEN, shp(golden[f"{k}_gF{suffix}"]))]
            for ours, M, gold in parts:
                assert ours.shape == gold.shape, (k, ours.shape, gold.shape)
                err, unit = np.abs(ours - gold), ar.U64 * M
                assert (err <= ar.C_GOLDEN * unit).all(), (ac.name_of(case), suffix, float((err / unit).max()))
                worst = max(worst, float(np.nanmax(np.where(unit > 0, err / np.where(unit > 0, unit, 1.0), 0.0))))
    assert worst <= ar.C_GOLDEN_MEASURED
    print(f"restatement against the reference's float64 autograd: largest ratio {worst:.3f} (C_GOLDEN_MEASURED = {ar.C_GOLDEN_MEASURED})")


def test_values_are_those_of_the_forward_restatement(cases):
    """The values next to the derivatives are tests/epipolar_ref.py's forward metrics (the yardstick of the forward kernels)."""
    import epipolar_ref as er

    for case in cases:
        if case["op"] != "metrics":
            continue
        F, X, Y, homo = case["F"], case["X"], case["Y"], case["homo"]
        want = {0: lambda: er.sym_epi(F, X, Y, homo, case["clamp_at"], case["eps"]), 1: lambda: er.sampson(F, X, Y, homo),
                2: lambda: er.epi_distance(F, X, Y, homo)}[case["kind"]]()
        np.testing.assert_allclose(ac.reference(case).value, want, rtol=4 * ar.U64, atol=0.0, equal_nan=True)


def test_host_build_passes_the_check(emu, cases):
    for case in cases:
        ac.check(case, run_emu(emu, case))


def test_flagged_set_is_the_listed_one(cases):
    """No point of any shared case is flagged (the fp64 bands are ~1e-12 relative); the exact families are decided exactly."""
    for case in cases:
        r = ac.reference(case)
        assert int(r.flagged.sum()) == 0, ac.name_of(case)
        if case["family"] == "integers":
            assert (r.t.s == 0).mean() >= 0.25                      # sign(0) = 0 is exercised
            if case["clamp_at"] is not None and case["op"] == "metrics" and case["eps"] == 0.0:
                assert (r.value == case["clamp_at"]).any() and r.gate[r.value == case["clamp_at"]].any()   # a point exactly ON the clamp passes
        if case["family"] == "epipole":
            assert (r.t.A[:, 0] == 0).all()


def test_a_non_finite_point_stays_local(emu):
    case = ac.make("nonfinite", 0, 3, 70, False, clamp=True, eps=1e-10, seed=5)
    clean = dict(case, X=case["X"].copy())
    clean["X"][1, 35, 0] = 1.0
    a, b = run_emu(emu, case), run_emu(emu, clean)
    keep = np.ones(70, bool)
    keep[35] = False
    for key in ("g_X", "g_Y"):
        assert np.array_equal(a[key][[0, 2]], b[key][[0, 2]]) and np.array_equal(a[key][1][keep], b[key][1][keep])
    assert np.array_equal(a["g_F"][[0, 2]], b["g_F"][[0, 2]])


def test_host_loss_form_passes_the_check(emu):
    P = emu.emu_epi_adjoint_chunk()
    for kind, homo, N in ((0, False, 70), (1, True, 70), (2, False, P + 3)):
        case = ac.make("scene", kind, 2, N, homo, clamp=(kind == 0), eps=1e-10 if kind == 0 else 0.0, seed=9)
        rng = np.random.default_rng(4)
        for w in (None, rng.uniform(0, 1, (2, N)).astype(F32)):
            gs = rng.standard_normal(2).astype(F32)
            got = {"sums": np.zeros(2, F32), "g_F": np.zeros((2, 3, 3), F32), "g_X": np.zeros_like(case["X"]), "g_Y": np.zeros_like(case["Y"]),
                   "g_w": np.zeros((2, N), F32)}
            args = (_kind(case), _p(case["F"]), _p(case["X"]), _p(case["Y"]), _p(w), 2, N, _cl(case), case["eps"])
            assert emu.emu_epi_loss_fwd(*args, _p(got["sums"])) == 0
            assert emu.emu_epi_loss_bwd(*args, _p(gs), _p(got["g_F"]), _p(got["g_X"]), _p(got["g_Y"]), _p(got["g_w"])) == 0
            ac.check_loss(case, w, gs, got)


# ---- the C ABI: refusals before any HIP call, the workspace and the chunk ----------------------------------------------------------
def _addr(align=0):
    buf = ctypes.create_string_buffer(64)  # host memory: only looked at, never dereferenced before the refusals
    _addr.keep.append(buf)
    return (ctypes.addressof(buf) + 15) // 16 * 16 + align


_addr.keep = []


def test_symbols_and_version(dfepe):
    L = dfepe._lib.lib()
    raw = ctypes.CDLL(dfepe.LIB_PATH)
    for name in ("dfepe_epi_adjoint_chunk", "dfepe_epi_adjoint_workspace_bytes", "dfepe_epi_metrics_bwd", "dfepe_epi_residual_bwd_pts",
                 "dfepe_epi_loss_fwd", "dfepe_epi_loss_bwd"):
        assert hasattr(raw, name) and name in dfepe.EXPORTED_SYMBOLS
    assert L.dfepe_version() == 154


def test_workspace_and_chunk_are_consistent(dfepe, emu):
    L = dfepe._lib.lib()
    P = L.dfepe_epi_adjoint_chunk()
    assert P == emu.emu_epi_adjoint_chunk() and P >= 256 and P % 256 == 0
    for B, N in ((1, 1), (3, P), (3, P + 1), (2, 2 * P), (2, 2 * P + 1), (0, 5 * P), (4, 0), (-1, 3 * P)):
        chunks = -(-N // P)
        want = B * chunks * 9 * 8 if (B > 0 and chunks > 1) else 0
        assert L.dfepe_epi_adjoint_workspace_bytes(B, N) == want, (B, N)


def test_refusals_without_a_launch(dfepe):
    L = dfepe._lib.lib()
    P = L.dfepe_epi_adjoint_chunk()
    a = _addr()

    def mb(kind=0, B=2, N=10, clamp=-1.0, F=a, X=a, Y=a, g=a, gF=a, gX=a, gY=a, ws=None):
        return L.dfepe_epi_metrics_bwd(None, kind, F, X, Y, B, N, clamp, 0.0, g, gF, gX, gY, ws)

    def lf(kind=0, B=2, N=10, clamp=-1.0, F=a, X=a, Y=a, w=None, out=a, ws=None):
        return L.dfepe_epi_loss_fwd(None, kind, F, X, Y, w, B, N, clamp, 0.0, out, ws)

    def lb(kind=0, B=2, N=10, clamp=-1.0, F=a, X=a, Y=a, w=None, gs=a, gF=a, gX=a, gY=a, gw=a, ws=None):
        return L.dfepe_epi_loss_bwd(None, kind, F, X, Y, w, B, N, clamp, 0.0, gs, gF, gX, gY, gw, ws)

    def rp(B=2, N=10, p1=a, p2=a, F=a, g=a, g1=a, g2=a):
        return L.dfepe_epi_residual_bwd_pts(None, p1, p2, F, B, N, 0.5, g, g1, g2)

    for f in (mb, lf, lb):
        assert f(B=-1) == INVALID and f(N=-1) == INVALID
        for bad in (-1, 3, 4, 7, 16, HOMO | 3):
            assert f(kind=bad) == INVALID
        assert f(kind=1, clamp=0.5) == INVALID and f(kind=2 | HOMO, clamp=0.0) == INVALID
        assert f(B=0) == 0 and f(N=0) == 0 and f(B=0, F=None, X=None, Y=None) == 0      # nothing to do: before the pointer checks
        assert f(B=0, kind=5) == INVALID and f(N=0, kind=1, clamp=1.0) == INVALID          # the documented order
        assert f(F=None) == INVALID and f(X=None) == INVALID and f(Y=None) == INVALID
        assert f(X=_addr(4)) == INVALID and f(Y=_addr(4)) == INVALID                       # [B,N,2] rows are read as 8-byte pairs
        assert f(N=P + 1) == INVALID and f(N=P + 1, ws=_addr(4)) == INVALID                # several chunks need the workspace
        assert f(B=3, N=2 ** 30) in (INVALID, UNSUPPORTED)
        assert f(B=3, N=2 ** 30, ws=a) == UNSUPPORTED
    assert mb(g=None) == INVALID and mb(gF=None, gX=None, gY=None) == INVALID
    assert mb(gX=_addr(4)) == INVALID and mb(gY=_addr(4)) == INVALID
    assert lf(out=None) == INVALID
    assert lb(gs=None) == INVALID and lb(gF=None, gX=None, gY=None, gw=None) == INVALID
    assert rp(B=-1) == INVALID and rp(N=-1) == INVALID and rp(B=0) == 0 and rp(N=0) == 0
    for k in ("p1", "p2", "F", "g"):
        assert rp(**{k: None}) == INVALID
    assert rp(g1=None, g2=None) == INVALID and rp(B=3, N=2 ** 30) == UNSUPPORTED


def test_python_layer_refuses_cpu_tensors_and_bad_arguments(dfepe):
    import torch

    F, X = torch.eye(3).expand(2, 3, 3), torch.zeros(2, 5, 2)
    with pytest.raises(dfepe.DfepeError):
        dfepe.ops.epi_loss(0, F, X, X)
    with pytest.raises(ValueError):
        dfepe.ops.epi_loss(0, F, X, X, reduction="max")
    with pytest.raises(dfepe.DfepeError):
        dfepe.compat.train_good_utils.get_loss_softmax(F, torch.zeros(2, 5, 3), torch.zeros(2, 5, 3), 0.5)
    with pytest.raises(dfepe.DfepeError):
        dfepe.compat.H_loss.HLoss()(F[0], X[0], X[0])
