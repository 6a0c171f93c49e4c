"""The accuracy contract of the two-view structure entry points, checked without a GPU: the fp64 restatement
(tests/triangulate_ref.py) is pinned against 50 digits, goes through check() itself (the cap on unheld points holds by itself),
and the host build of csrc/triangulate_math.h -- the code the kernels run per lane -- goes through the same check() on every
family, all three functions.  The printed distances are fractions of the bounds (DESIGN.md §3.12 records them)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import triangulate_cases as C  # noqa: E402
import triangulate_ref as ref  # noqa: E402

ALL = C.REGULAR + C.DEGENERATE


def test_restatement_sits_within_a_sixteenth_of_the_band_of_50_digits():
    pytest.importorskip("mpmath")
    worst = {}
    for name in ALL:
        f = C.family(name)
        if "K" in f:
            P1, P2, _, _ = ref.cameras(f["Rt"], f["K"], False)
            Xr, eta = ref.null_vectors(P1, P2, ref.f64(f["m"]))
        else:
            P1, P2 = ref.f64(f["P1"]), ref.f64(f["P2"])
            Xr, eta = C.ref_triangulate(name)
        m = ref.f64(f["m"])
        w = 0.0
        for i in range(0, len(m), 16):
            if not np.isfinite(eta[i]):  # no null vector, or no gap: nothing to pin
                continue
            Xm = ref.mp_null_vector(P1, P2, m[i])
            d = np.abs(Xr[i] - Xm).max()
            if abs(Xm[3]) <= eta[i]:
                d = min(d, np.abs(Xr[i] + Xm).max())
            w = max(w, d / (eta[i] / 16))
        worst[name] = w
        assert w <= 1.0, f"{name}: the restatement is {w:.3g} x eta / 16 from 50 digits"
    print("restatement vs 50 digits, fractions of eta / 16:", {k: f"{v:.2g}" for k, v in worst.items()})


def test_restatement_passes_its_own_check_and_holds_the_cap():
    for name in ALL:
        Xr, eta = C.ref_triangulate(name)
        C.check("Xh", Xr, (Xr, eta), name, "restatement")
        if name == "general_P":
            continue
        r = C.ref_structure(name)
        C.check("structure", {k: r[k] for k in ("X", "z1", "z2")}, r, name, "restatement")
        if C.family(name)["regular"]:
            share = (~C.held(r)).mean()
            print(f"{name}: unheld {share:.4f}, eta median {np.nanmedian(r['eta']):.2g} max {np.nanmax(r['eta'][np.isfinite(r['eta'])]):.2g}")
    for name in ("near_epipole[0]", "near_epipole[1e-3]", "near_epipole[0.1]"):
        print(f"{name}: held share {C.held(C.ref_structure(name)).mean():.2f}")


@pytest.mark.parametrize("name", ALL)
def test_host_build_of_the_header_passes_check_on_every_family(name):
    f = C.family(name)
    fr = {"Xh": C.check("Xh", C.header_triangulate(f["P1"], f["P2"], f["m"]), C.ref_triangulate(name), name, "header")}
    if name != "general_P":
        fr["structure"] = C.check("structure", C.header_structure(f["Rt"], f["K"], f["m"]), C.ref_structure(name), name, "header")
        fr["structure_cam"] = C.check("structure", C.header_structure(f["Rt_cam"], f["K"], f["m"], camera_motion=True),
                                      C.ref_structure(name, True), name, "header_cam")
        sc = C.header_structure(f["Rt"], f["K"], f["m"], scale=7.25, clamp=150.0)
        C.check("structure", sc, C.ref_structure(name), name, "header_scaled", scale=7.25, clamp=150.0)
        C.check("structure", {"X": sc["X"]}, C.ref_structure(name), name, "header_scaled", scale=7.25)
        for view in (1, 2):
            Rt = C.IDENTITY_RT if view == 1 else f["Rt"]
            fr[f"reproject{view}"] = C.check("reproject", C.header_reproject(f["Xw"], Rt, f["K"]), C.ref_reproject(name, view), name, "header")
        fr["reproject_cam"] = C.check("reproject", C.header_reproject(f["Xw"], f["Rt_cam"], f["K"], camera_motion=True),
                                      C.ref_reproject(name, 2, True), name, "header_cam")
        no_pose = C.header_structure(f["Rt"], f["K"], f["m"], winner=-1)
        assert all(np.isnan(v).all() for v in no_pose.values())
    print(f"host header, {name}: " + ", ".join(f"{k} {v:.2g}" for k, v in fr.items()))


@pytest.mark.parametrize("name", ("short_baseline", "outliers"))
def test_regression_guard_values_need_more_than_one_refinement(name):
    """The families on which the cheirality route (an fp32 start and one fp64 Rayleigh-quotient iteration) misses the band by
    orders of magnitude: the header's worst fraction of the bound, Xh and values."""
    f = C.family(name)
    a = C.check("Xh", C.header_triangulate(f["P1"], f["P2"], f["m"]), C.ref_triangulate(name), name, "guard")
    b = C.check("structure", C.header_structure(f["Rt"], f["K"], f["m"]), C.ref_structure(name), name, "guard")
    print(f"regression guard, {name}: Xh at {a:.3g}, X / z1 / z2 at {b:.3g} of the bound")
    assert a <= 1.0 and b <= 1.0


def test_round_trip_of_the_header_stays_within_the_propagated_bounds():
    for name in ("forward", "sideways"):
        f = C.family(name)
        X = C.header_structure(f["Rt"], f["K"], f["m"])["X"]
        h = C.held(C.ref_structure(name))
        for view in (1, 2):
            x = C.header_reproject(X, C.IDENTITY_RT if view == 1 else f["Rt"], f["K"])["x"].astype(np.float64)
            d = np.abs(x - f["m"][:, 2 * view - 2:2 * view].astype(np.float64))
            b = C.round_trip_bound(name, view)
            print(f"round trip, {name} view {view}: max {d[h].max():.3g} px, {(d / b)[h].max():.3g} of the bound")
            assert (d <= b)[h].all()
