"""The tridiagonalising basis in the fit's `save` record: the forward stores the explicit orthogonal Q = diag(1, Q') with
M / trace M = Q T Q^T (not its seven Householder reflectors) and z, the eigenvector of T; the backward recomputes f = Q z and applies
Q^T and Q as independent sums.  Checked here on the record the emulated bodies write (tests/emu/, no GPU): Q is orthogonal, it
tridiagonalises the oracle's fp64 design matrix into the stored T, Q z reproduces the returned F, both layout marks are there and
the backward refuses a record without the second one -- at every rung of the N ladder and on the degenerate rows.

Bounds: the 64 entries of Q' and the 9 of z are rounded to fp32 (relative 2^-24 each); an entry of Q^T Q or Q^T (M / tr M) Q sums
up to 8 such products twice over, |entries| <= 1, ||M / tr M|| <= 1: 2 * 8 * 2^-24 = 9.5e-7, and the bound leaves a factor of two."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_emu_cpu import IMAGE_SIZE, LOGITS, RAW, emu, emu_bwd, emu_fwd, relerr, unit_align  # noqa: E402,F401  (emu: the fixture)

# ---- mirror of the record layout in pytorch-deepfepe_amd/csrc/w8pt16_body.h (S16_*), floats ----
S16_Q = 8        # 64: Q'[i][j], i, j = 1..8, at 8 i + (j - 1)
S16_TD = 72      # 9 doubles
S16_TE = 90      # 8 doubles
S16_Z = 108      # 9
S16_MARK, MARK_VALUE = 126, 64.0
S16_TAG, TAG_VALUE = 127, 17.0

BOUND = 2e-6
LADDER = (8, 9, 16, 17, 100, 112, 113, 128, 129, 300)


def read_record(save):
    """(Q [B,9,9], td [B,9], te [B,8], z [B,9]) of a record, in fp64."""
    s = save.contiguous().numpy()
    B = s.shape[0]
    Q = np.zeros((B, 9, 9))
    Q[:, 0, 0] = 1.0
    Q[:, 1:, 1:] = s[:, S16_Q:S16_Q + 64].reshape(B, 8, 8).astype(np.float64)
    td = np.ascontiguousarray(s[:, S16_TD:S16_TD + 18]).view(np.float64)
    te = np.ascontiguousarray(s[:, S16_TE:S16_TE + 16]).view(np.float64)
    z = s[:, S16_Z:S16_Z + 9].astype(np.float64)
    return Q, td, te, z


def tridiag(td, te):
    T = np.zeros((td.shape[0], 9, 9))
    i = np.arange(9)
    T[:, i, i] = td
    T[:, i[:-1], i[1:]] = te
    T[:, i[1:], i[:-1]] = te
    return T


def record_figures(oracle, m, wout, F, save):
    """The three record figures: max |Q^T Q - I|, max |Q^T (M / tr M) Q - T|, max over the pairs of |unit F(Q z) - unit F returned|."""
    Q, td, te, z = read_record(save)
    Qt = np.transpose(Q, (0, 2, 1))
    orth = np.abs(Qt @ Q - np.eye(9)).max()
    p1, p2, _ = oracle.normalize_hw(m.double(), IMAGE_SIZE)
    _, X, T1, T2 = oracle.fit_rows(p1, p2, wout.double().unsqueeze(1))
    M = (X.transpose(1, 2) @ X).numpy()
    Mn = M / np.trace(M, axis1=1, axis2=2)[:, None, None]
    tri = np.abs(Qt @ Mn @ Q - tridiag(td, te)).max()
    f = torch.from_numpy(np.einsum("bij,bj->bi", Q, z))
    out = T2.transpose(1, 2) @ oracle._rank2(f.reshape(-1, 3, 3), "batched") @ T1
    a, r, _ = unit_align(out, F)
    dF = (a - r).norm(dim=1).max().item()
    return orth, tri, dF


@pytest.mark.parametrize("N", LADDER)
def test_record_basis_is_orthogonal_tridiagonalises_and_reproduces_F(emu, dfepe, oracle, N):
    B = 5
    sc = dfepe.synth.make_scene(B, N, seed=300 + N, outlier_ratio=0.2, noise_px=0.5)
    m = sc["matches_xy_ori"].contiguous()
    logits = sc["logits_layers"][0].contiguous()
    F, res, epi, save, wout = emu_fwd(emu, m, None, logits, RAW | LOGITS)
    orth, tri, dF = record_figures(oracle, m, wout, F, save)
    tolF = 2 * (1e-5 if N < 12 else 1e-6)  # the bound of test_forward_body_matches_fp64_oracle for F
    print(f"N={N}: |QtQ-I| {orth:.2e} (<= {BOUND}), |QtMQ-T| {tri:.2e} (<= {BOUND}), |F(Qz)-F| {dF:.2e} (< {tolF})")
    assert orth <= BOUND
    assert tri <= BOUND
    assert dF < tolF
    # both layout marks; a record with the second one cleared is refused (NaN), not misread
    assert (save[:, S16_TAG] == TAG_VALUE).all() and (save[:, S16_MARK] == MARK_VALUE).all()
    GF = torch.randn(B, 3, 3, generator=torch.Generator().manual_seed(2))
    gL, _, _ = emu_bwd(emu, m, None, wout, RAW | LOGITS, save, F, GF, None, None)
    assert torch.isfinite(gL).all()
    bad = save.clone()
    bad[:, S16_MARK] = 0.0
    gB, _, _ = emu_bwd(emu, m, None, wout, RAW | LOGITS, bad, F, GF, None, None)
    assert torch.isnan(gB).all()
    bad = save.clone()
    bad[:, S16_TAG] = 16.0
    gB, _, _ = emu_bwd(emu, m, None, wout, RAW | LOGITS, bad, F, GF, None, None)
    assert torch.isnan(gB).all()


def _oracle_grad(oracle, m, logits, F, GF):
    lo_in = logits.double().requires_grad_(True)
    p1, p2, _ = oracle.normalize_hw(m.double(), IMAGE_SIZE)
    o_out, _, _ = oracle.fit_forward(p1, p2, torch.softmax(lo_in, 1).unsqueeze(1))
    s = torch.sign((o_out.detach() * F.double()).flatten(1).sum(1))
    (s[:, None, None] * o_out * GF.double()).sum().backward()
    return lo_in.grad


def _orth(save):
    Q = read_record(save)[0]
    return Q, np.abs(np.transpose(Q, (0, 2, 1)) @ Q - np.eye(9)).max()


def test_rank_one_row_keeps_basis_orthogonal(emu, dfepe, oracle):
    """All correspondences of pair 1 identical: M has rank 1, every reflector after the first is the identity.  The eigenvector and
    its adjoint are ill-defined there (an eightfold zero eigenvalue): the gradient of that pair may be anything but infinite; the
    other pairs are held to the oracle."""
    B, N = 5, 100
    sc = dfepe.synth.make_scene(B, N, seed=41, outlier_ratio=0.2, noise_px=0.5)
    m = sc["matches_xy_ori"].clone().contiguous()
    m[1] = m[1, 0]
    logits = sc["logits_layers"][0].contiguous()
    F, res, epi, save, wout = emu_fwd(emu, m, None, logits, RAW | LOGITS)
    Q, orth = _orth(save)
    print(f"rank one: |QtQ-I| {orth:.2e}")
    assert np.isfinite(Q).all() and orth <= BOUND
    GF = torch.randn(B, 3, 3, generator=torch.Generator().manual_seed(4))
    gL, _, _ = emu_bwd(emu, m, None, wout, RAW | LOGITS, save, F, GF, None, None)
    assert not torch.isinf(gL).any()
    keep = [0, 2, 3, 4]
    assert torch.isfinite(gL[keep]).all()
    assert relerr(gL[keep].numpy(), _oracle_grad(oracle, m[keep], logits[keep], F[keep], GF[keep]).numpy()) < 2e-4


def test_non_finite_correspondence_keeps_basis_and_gradient_finite(emu, dfepe, oracle):
    """One non-finite correspondence in pair 2: dropped from X by the forward and the backward alike.  The oracle has no gradient for
    that pair (NaN input); it is finite here, and the other pairs are held to the oracle."""
    B, N = 5, 100
    sc = dfepe.synth.make_scene(B, N, seed=43, outlier_ratio=0.2, noise_px=0.5)
    m = sc["matches_xy_ori"].clone().contiguous()
    m[2, 17, 1] = float("nan")
    logits = sc["logits_layers"][0].contiguous()
    F, res, epi, save, wout = emu_fwd(emu, m, None, logits, RAW | LOGITS)
    Q, orth = _orth(save)
    print(f"non-finite correspondence: |QtQ-I| {orth:.2e}")
    assert np.isfinite(Q).all() and orth <= BOUND
    GF = torch.randn(B, 3, 3, generator=torch.Generator().manual_seed(5))
    gL, _, _ = emu_bwd(emu, m, None, wout, RAW | LOGITS, save, F, GF, None, None)
    assert torch.isfinite(gL).all()
    keep = [0, 1, 3, 4]
    assert relerr(gL[keep].numpy(), _oracle_grad(oracle, m[keep], logits[keep], F[keep], GF[keep]).numpy()) < 2e-4


def test_minimal_system_takes_the_kth_branch(emu, dfepe, oracle):
    """N = 8: M has rank 8 and the fit passes over one eigenvalue (kth = 1).  Basis orthogonal, gradient finite and the oracle's
    (bound of test_backward_body_vs_oracle_autograd for N < 20)."""
    B, N = 5, 8
    sc = dfepe.synth.make_scene(B, N, seed=15, outlier_ratio=0.2)
    m = sc["matches_xy_ori"].contiguous()
    logits = sc["logits_layers"][0].contiguous()
    F, res, epi, save, wout = emu_fwd(emu, m, None, logits, RAW | LOGITS)
    Q, orth = _orth(save)
    print(f"N = 8: |QtQ-I| {orth:.2e}")
    assert np.isfinite(Q).all() and orth <= BOUND
    GF = torch.randn(B, 3, 3, generator=torch.Generator().manual_seed(6))
    gL, _, _ = emu_bwd(emu, m, None, wout, RAW | LOGITS, save, F, GF, None, None)
    assert torch.isfinite(gL).all()
    assert relerr(gL.numpy(), _oracle_grad(oracle, m, logits, F, GF).numpy()) < 2e-3
