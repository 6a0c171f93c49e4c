"""tests/cheirality_ref.py (the fp64 restatement the GPU cheirality tests compare with) against oracle.cheirality_select and the
golden vectors the unmodified reference wrote."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cheirality_ref as cref  # noqa: E402


def _oracle_counts(oracle, E, K, m, thr):
    E64 = torch.from_numpy(np.asarray(E, np.float32).astype(np.float64))
    m64 = np.asarray(m, np.float32).astype(np.float64)
    return oracle.cheirality_select(E64, np.asarray(K, np.float32).astype(np.float64), m64[:, :2], m64[:, 2:], float(np.float32(thr)))


def _hold(r, counts, winner, Rt_cam):
    """counts / winner / Rt_cam of a same-gauge (LAPACK) run of the reference's algorithm against the restatement r."""
    counts = np.asarray(counts)
    assert ((r["lo"] <= counts) & (counts <= r["hi"])).all(), (counts, r["lo"], r["hi"])
    if not r["undecided"].any():
        assert (counts == r["in_front"].sum(1)).all()
        w = cref.select(counts)
        assert w == winner
        if w >= 0:
            np.testing.assert_allclose(cref.inverse_pose(*r["cands"][w]), Rt_cam, atol=1e-9)
        return True
    return False


@pytest.mark.parametrize("case", ["mixed", "dense1000", "garbage"])
def test_restatement_reproduces_the_golden_of_the_unmodified_reference(golden, oracle, case):
    g = golden("cheirality")
    E, K, m = (g[f"{case}_{k}"] for k in ("E", "K", "matches"))
    thr = float(g[f"{case}_depth_thres"])
    exact = 0
    for b in range(E.shape[0]):
        r = cref.reference(E[b], K[b], m[b], thr)
        gw = int(g[f"{case}_winner"][b])
        exact += _hold(r, g[f"{case}_counts"][b], gw, g[f"{case}_Rt_cam"][b] if gw >= 0 else None)
        _, win, counts = _oracle_counts(oracle, E[b], K[b], m[b], thr)
        _hold(r, counts, win if counts[win] > 0 else -1, g[f"{case}_Rt_cam"][b] if gw >= 0 else None)
    assert exact >= 0.95 * E.shape[0]


@pytest.mark.parametrize("N,outliers,planar,thr,which", [(300, 0.2, False, 50.0, "gt"), (257, 0.6, False, 5.0, "gt"),
                                                         (300, 0.2, True, 20.0, "gt"), (200, 0.2, False, 50.0, "random")])
def test_restatement_agrees_with_the_oracle_on_scenes(dfepe, oracle, N, outliers, planar, thr, which):
    B = 4
    sc = dfepe.synth.make_scene(B, N, seed=N, outlier_ratio=outliers, planar=planar)
    E = sc["E_gt"] / sc["E_gt"].flatten(1).norm(dim=1)[:, None, None]
    if which == "random":
        E = torch.randn(B, 3, 3, generator=torch.Generator().manual_seed(N))
    E, K, m = E.float().numpy(), sc["Ks"].float().numpy(), sc["matches_xy_ori"].float().numpy()
    exact = 0
    for b in range(B):
        r = cref.reference(E[b], K[b], m[b], thr)
        Rt, win, counts = _oracle_counts(oracle, E[b], K[b], m[b], thr)
        exact += _hold(r, counts, win if counts[win] > 0 else -1, None if Rt is None else Rt.numpy())
    assert exact == B


def test_non_finite_rows_count_nowhere(dfepe):
    sc = dfepe.synth.make_scene(1, 130, seed=2, outlier_ratio=0.1)
    E, K, m = sc["E_gt"][0].float().numpy(), sc["Ks"][0].float().numpy(), sc["matches_xy_ori"][0].float().numpy()
    full = cref.reference(E, K, m, 50.0)
    assert full["in_front"].any()
    bad = m.copy()
    bad[0] = np.nan
    bad[64:128, 2] = np.nan   # one coordinate only
    bad[129, 1] = np.inf
    r = cref.reference(E, K, bad, 50.0)
    dead = ~np.isfinite(bad).all(1)
    assert not r["in_front"][:, dead].any() and not r["undecided"][:, dead].any()
    assert (r["in_front"][:, ~dead] == full["in_front"][:, ~dead]).all()
    bad[:] = np.nan
    r = cref.reference(E, K, bad, 50.0)
    assert (r["lo"] == 0).all() and (r["hi"] == 0).all() and cref.select(r["hi"]) == -1


def test_pre_forms_the_congruence_in_fp64():
    g = np.random.default_rng(0)
    F, pre = g.standard_normal((3, 3)).astype(np.float32), g.standard_normal((3, 3)).astype(np.float32)
    np.testing.assert_allclose(cref.essential(F, pre), pre.astype(np.float64).T @ F.astype(np.float64) @ pre.astype(np.float64), rtol=0, atol=0)
