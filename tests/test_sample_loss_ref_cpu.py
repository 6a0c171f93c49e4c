"""The sample-loss branch without a GPU: the host build of csrc/sample_loss_math.h (tests/emu/emu_sample_loss.cpp) through the same
check() of every stage as the GPU (tests/sample_loss_cases.py) -- the draw and the top-K bit for bit against the integer restatement
(tests/sample_loss_ref.py), the floating-point stages inside their derived bounds -- one chi-square check of the restatement's law
with a fixed seed, and the stand-alone program over the host build under -fsanitize=address,undefined."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_loss_cases as sc  # noqa: E402
import sample_loss_ref as slr  # noqa: E402
import sampler_ref as sr  # noqa: E402

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EMU_DIR = os.path.join(REPO, "tests", "emu")
CSRC = os.path.join(REPO, "pytorch-deepfepe_amd", "csrc")
SRCS = [os.path.join(EMU_DIR, "emu_sample_loss.cpp")] + [os.path.join(CSRC, h) for h in ("sample_loss_math.h", "sampler_math.h", "epi_adjoint_math.h")]


def _stale(out):
    return not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in SRCS)


@pytest.fixture(scope="module")
def emu():
    out = os.path.join(EMU_DIR, "_build")
    os.makedirs(out, exist_ok=True)
    lib = os.path.join(out, "libemu_sample_loss.so")
    if _stale(lib):
        subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", f"-I{CSRC}", SRCS[0], "-o", lib], check=True)
    L = ctypes.CDLL(lib)
    i, p, u, u64, f = ctypes.c_int, ctypes.c_void_p, ctypes.c_uint, ctypes.c_ulonglong, ctypes.c_float
    L.emu_sample_multisets.argtypes, L.emu_sample_multisets.restype = [i, i, i, i, u64, u, p, p, p, p, p], None
    L.emu_topk_select.argtypes, L.emu_topk_select.restype = [p, p, i, i, i, p], None
    L.emu_sample_gather.argtypes, L.emu_sample_gather.restype = [p, p, p, p, i, i, i, i, p, p, p, p], None
    L.emu_sample_floss.argtypes, L.emu_sample_floss.restype = [p, i, i, p, p, i, p, p, i, f, p, p, p], None
    L.emu_sample_scatter_bwd.argtypes, L.emu_sample_scatter_bwd.restype = [p, p, p, p, p, i, i, i, i, p], None
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _c(a, dtype=np.float32):
    return np.ascontiguousarray(a, dtype)


def test_host_draw_is_the_restatement(emu):
    for case in sc.draw_cases():
        B, H, K = case["B"], case["H"], case["K"]
        idx, fb = np.full((B, H, K), -1, np.int32), np.full(B, -1, np.int32)
        ctr = None if case["counter"] is None else np.array([case["counter"]], np.uint32)
        emu.emu_sample_multisets(B, case["N"], H, K, case["seed"], case["offset"], _p(ctr), _p(case["weights"]), _p(case["n_valid"]), _p(idx), _p(fb))
        sc.check_draw(idx, fb, case)


def test_a_set_does_not_depend_on_the_batch():
    """(seed, off, b, h, n, K) and the pair's weights alone: pair 2, set 64 of a 3 x 65 draw is the same in a 4 x 100 draw."""
    w = sc._weights(4, 70, 5)
    a, _, _ = slr.sample_multisets(3, 70, 65, 20, 9, weights=w[:3], pairs=[2], sets=[64])
    b, _, _ = slr.sample_multisets(4, 70, 100, 20, 9, weights=w, pairs=[2], sets=[64])
    assert (a[2, 64] == b[2, 64]).all() and (a[2, 64] >= 0).all()


def test_host_topk_is_the_rule(emu):
    for case in sc.topk_cases():
        B, N = case["x"].shape
        idx = np.full((B, case["K"]), -1, np.int32)
        emu.emu_topk_select(_p(case["x"]), _p(case["n_valid"]), B, N, case["K"], _p(idx))
        sc.check_topk(idx, case)


def test_topk_rule_against_torch():
    """Where torch.topk is deterministic (distinct finite values and NaNs apart) the rule gives torch's indices."""
    import torch

    x = np.random.RandomState(1).randn(3, 90).astype(np.float32)
    assert (slr.topk(x, 20) == torch.topk(torch.from_numpy(x), 20, dim=1)[1].numpy()).all()
    x[0, 5] = np.nan
    assert slr.topk(x, 20)[0, 0] == 5 and torch.topk(torch.from_numpy(x), 20, dim=1)[1][0, 0] == 5


def _gather(emu, case):
    B, N = case["weights"].shape
    _, H, K = case["idx"].shape
    p1, p2, w = np.zeros((B * H, K, 3), np.float32), np.zeros((B * H, K, 3), np.float32), np.zeros((B * H, K), np.float32)
    accu = np.zeros((B, H), np.float32)
    zero = np.zeros((B, N, 3), np.float32)
    emu.emu_sample_gather(_p(_c(case.get("pts1", zero))), _p(_c(case.get("pts2", zero))), _p(_c(case["weights"])), _p(_c(case["idx"], np.int32)),
                          B, N, H, K, _p(p1), _p(p2), _p(w), _p(accu))
    return p1, p2, w, accu


def test_host_gather_and_accu(emu):
    for tag, case in sc.gather_cases():
        sc.check_gather(*_gather(emu, case), case, tag)


def test_host_loss_and_adjoint(emu):
    for case in sc.loss_cases():
        B, H = case["F_sel"].shape[:2]
        M = case["virt1"].shape[1]
        T1, T2 = _c(case["T1"]), _c(case["T2"])
        st = 9 if T1.ndim == 3 else 0
        loss, gF = np.zeros((B, H), np.float32), np.zeros((B, H, 3, 3), np.float32)
        args = (_p(_c(case["F_sel"])), B, H, _p(T1), _p(T2), st, _p(_c(case["virt1"])), _p(_c(case["virt2"])), M, case["clamp"])
        emu.emu_sample_floss(*args, _p(loss), None, None)
        emu.emu_sample_floss(*args, None, _p(_c(case["g"])), _p(gF))
        sc.check_loss(loss, gF, case)


def test_host_scatter(emu):
    for case in sc.scatter_cases():
        B, N = case["weights"].shape
        _, H, K = case["idx"].shape
        accu = _gather(emu, case)[3]
        for with_accu in (True, False):
            g_w = np.full((B, N), 7.0, np.float32)
            emu.emu_sample_scatter_bwd(_p(case["g_w_sel"]), _p(case["g_accu"]) if with_accu else None, _p(case["weights"]), _p(accu), _p(case["idx"]),
                                       B, N, H, K, _p(g_w))
            sc.check_scatter(g_w, case, accu, with_accu)


CHI2_999 = {35: 66.62}  # the 99.9 % quantile of chi-square, as tests/test_sampler_ref_cpu.py states it


def test_first_draw_marginal():
    """The first draw of 20000 sets (seed 9, offset 1, b = 0) against q / sum q: 36 drawable weights, 35 degrees of freedom.  Every
    draw of a multiset has this law (with replacement), the first one stands for them."""
    rng = random.Random(3)
    w = [rng.random() ** 4 for _ in range(40)]
    w[5:9] = [0.0, float("nan"), -1.0, 1e-12]
    q = sr.quantise(w)
    P = sr.prefix(q)
    assert [q[i] for i in range(5, 9)] == [0, 0, 0, 0]
    c = np.zeros(40)
    sets = 20000
    for h in range(sets):
        c[slr.multiset(sr.r64_draws(9, 1, 0, h, 1), q, P, 40, 1)[0]] += 1
    qa = np.array(q, float)
    pos = qa > 0
    e = sets * qa[pos] / qa.sum()
    stat = ((c[pos] - e) ** 2 / e).sum()
    dof = int(pos.sum()) - 1
    print(f"multiset first draw: chi2 = {stat:.2f} at {dof} dof (bound {CHI2_999[dof]})")
    assert c[~pos].sum() == 0 and stat < CHI2_999[dof]


def test_standalone_program_under_sanitizers():
    """The stand-alone program (its own main) over the host build with -fsanitize=address,undefined at the shapes of the GPU tests."""
    out = os.path.join(EMU_DIR, "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "emu_sample_loss_san")
    if _stale(exe):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-DEMU_SAMPLE_LOSS_MAIN", f"-I{CSRC}", SRCS[0], "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "every index in range" in r.stdout


def test_restatement_against_the_reference_golden(golden):
    """tests/golden/sample_loss.npz (the reference's own Fit.forward and loss lines, float64 run) against the float64 restatement on the
    recorded sets: the top-K rule picks what torch.topk picked, the fits, accu, the loss and d loss / d weights agree to float64
    round-off of two LAPACK routes (1e-9 of the largest entry, 1e-6 for the gradient; F up to its sign)."""
    import torch

    oracle = __import__("oracle.deepf_oracle", fromlist=["x"])
    g = golden("sample_loss")
    B, N = g["logits"].shape
    w = torch.softmax(torch.from_numpy(g["logits"]).double(), 1).requires_grad_(True)
    p1, p2, _ = oracle.normalize_hw(torch.from_numpy(g["matches"]).double(), sc.IMAGE_SIZE)
    T = torch.from_numpy(sc.T_HW.astype(np.float64))
    # the top-K fit: the rule's indices, then the reference's own arithmetic on them
    top = slr.topk(w.detach().float().numpy(), 20, g["nums"])
    F_top, _ = slr.fit_selected(p1, p2, w.detach(), top[:, None, :])
    assert slr.fit_error(F_top.reshape(B, 3, 3).numpy(), g["f64_out_topK"]).max() < 1e-9
    F_sel, accu = slr.fit_selected(p1, p2, w, g["idx"])
    assert slr.fit_error(F_sel.detach().reshape(-1, 3, 3).numpy(), g["f64_out_sample_selected_batch"].reshape(-1, 3, 3)).max() < 1e-9
    np.testing.assert_allclose(accu.detach().numpy(), g["f64_weights_sample_selected_accu_batch"], rtol=1e-9, atol=1e-300)
    loss, layers = slr.loss_selected([F_sel], T, T, torch.from_numpy(g["virt1"]), torch.from_numpy(g["virt2"]))
    assert abs(loss.item() - float(g["f64_loss_selected_F"])) < 1e-9 * float(g["f64_loss_selected_F"])
    loss.backward()
    # the adjoint of an SVD divides by the gaps of the singular values: the round-off of the two routes is amplified by them
    assert np.abs(w.grad.numpy() - g["f64_g_weights"]).max() < 1e-6 * np.abs(g["f64_g_weights"]).max()
    # accu of the float64 restatement of the device's formula is the same number
    a, _ = slr.accu(w.detach().numpy(), g["idx"])
    np.testing.assert_allclose(a[..., None], g["f64_weights_sample_selected_accu_batch"], rtol=1e-9)


def test_compat_host_draw_reproduces_the_recorded_sets(golden, dfepe):
    """compat.DeepFNetSampleLoss.Fit without a sampler, under the golden's NumPy seed, draws the sets the reference drew."""
    import torch

    g = golden("sample_loss")
    w = torch.softmax(torch.from_numpy(g["logits"]).unsqueeze(1), dim=2)
    np.random.seed(int(g["seed"]))
    idx = dfepe.compat.DeepFNetSampleLoss.Fit().draw_host(w, torch.from_numpy(g["nums"]))
    assert (idx.numpy() == g["idx"]).all()
