"""The C ABI of the correspondence evaluation without a GPU: the two symbols are exported, the version did not move, every refusal
include/dfepe.h lists is made on the host before anything is launched; the Python layers refuse CPU tensors; and the host-side
contract of compat.eval_tools.Result_processor and of PointTracker's two-frame state holds."""
import ctypes
import logging

import numpy as np
import pytest

INVALID = -1
NAMES = ("dfepe_inlier_table", "dfepe_inlier_table_mean")
PTRS = ("m", "F", "d", "sc", "nv", "it", "mt", "cnt", "num", "ratio", "do")


def _addr(align=0):
    buf = ctypes.create_string_buffer(64)  # host memory: only looked at, never dereferenced before the refusals
    _addr.keep.append(buf)
    return (ctypes.addressof(buf) + 15) // 16 * 16 + align


_addr.keep = []


def _tab(L, B=2, N=10, Ti=2, Tm=2, **ptr):
    a = _addr()
    p = {name: a for name in PTRS}
    p["d"] = None  # matches + F by default
    p.update(ptr)
    return L.dfepe_inlier_table(p["m"], p["F"], p["d"], p["sc"], p["nv"], B, N, p["it"], Ti, p["mt"], Tm, p["cnt"], p["num"], p["ratio"],
                                p["do"], None)


def test_symbols_and_version(dfepe):
    L = dfepe._lib.lib()
    raw = ctypes.CDLL(dfepe.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name) and name in dfepe.EXPORTED_SYMBOLS
    assert L.dfepe_version() == 154  # pinned by the existing tests; nothing that existed changed
    assert dfepe._lib.INLIER_TABLE_MAX_THDS == 16


def test_inlier_table_refusals_without_a_launch(dfepe):
    L = dfepe._lib.lib()
    none = {name: None for name in PTRS}
    assert _tab(L, B=0, Tm=1, **none) == 0 and _tab(L, B=0) == 0                     # empty batch: nothing to do
    assert _tab(L, B=-1) == INVALID and _tab(L, N=-1) == INVALID
    for bad in (0, -1, 17):
        assert _tab(L, Ti=bad) == INVALID and _tab(L, Tm=bad) == INVALID
    assert _tab(L, d=_addr()) == INVALID                                        # matches and dist: exactly one
    assert _tab(L, sc=None, Tm=2) == INVALID                                    # no scores: nothing to sweep
    # the documented order: these are refused on an empty batch too
    assert _tab(L, B=0, Ti=0, **none) == INVALID and _tab(L, B=0, d=_addr()) == INVALID and _tab(L, B=0, sc=None, Tm=2) == INVALID
    assert _tab(L, m=None) == INVALID                                           # N > 0 and neither input
    assert _tab(L, F=None) == INVALID and _tab(L, m=_addr(8)) == INVALID        # matches without F, or misaligned
    assert _tab(L, it=None) == INVALID and _tab(L, mt=None) == INVALID
    assert _tab(L, cnt=None, num=None, ratio=None, do=None) == INVALID          # nothing asked for
    assert _tab(L, N=0, m=None, F=None, it=None) == INVALID                     # N == 0 needs no input, but its thresholds


def test_inlier_table_mean_refusals_without_a_launch(dfepe):
    L = dfepe._lib.lib()
    a = _addr()
    mean = lambda B=3, Tm=2, Ti=2, r=a, n=a, m=a, t=a: L.dfepe_inlier_table_mean(r, n, B, Tm, Ti, m, t, None)  # noqa: E731
    assert mean(B=-1) == INVALID
    for bad in (0, -1, 17):
        assert mean(Ti=bad) == INVALID and mean(Tm=bad) == INVALID
    assert mean(m=None, t=None) == INVALID
    assert mean(r=None) == INVALID and mean(n=None) == INVALID
    assert mean(B=0, r=None, n=None, m=None, t=None) == INVALID


def test_python_layer_refuses_cpu_tensors_and_bad_arguments(dfepe):
    import torch

    m, F, sc = torch.zeros(2, 5, 4), torch.eye(3).expand(2, 3, 3), torch.zeros(2, 5)
    with pytest.raises(dfepe.DfepeError):
        dfepe.ops.inlier_table(matches=m, F=F, scores=sc, inlier_thds=[1.0], mask_thds=[1.0])
    with pytest.raises(dfepe.DfepeError):
        dfepe.ops.inlier_table(dist=sc, inlier_thds=[1.0])
    with pytest.raises(dfepe.DfepeError):
        dfepe.ops.inlier_table_mean(torch.zeros(2, 1, 1, dtype=torch.float64), torch.zeros(2, 1, dtype=torch.int32))
    with pytest.raises(ValueError):
        dfepe.ops.inlier_table(matches=m, F=F, dist=sc)                         # exactly one of the two
    with pytest.raises(ValueError):
        dfepe.ops.inlier_table(inlier_thds=[1.0])
    with pytest.raises(ValueError):
        dfepe.ops.inlier_table(dist=sc, want=("mean",))
    with pytest.raises(dfepe.DfepeError):
        dfepe.compat.correspondence_eval_batch((m[..., :2], m[..., :2]), (torch.zeros(2, 5, 32), torch.zeros(2, 5, 32)), F, 0.7, [1.0])
    with pytest.raises(dfepe.DfepeError):
        dfepe.compat.evaluation_epiDist.epi_dist_from_matches(np.zeros((1, 5, 4)), {"F": F}, "cpu")
    img = dfepe.compat.evaluation_epiDist.process_grey2tensor(torch.full((2, 4, 6), 255, dtype=torch.uint8))
    assert img.shape == (2, 1, 4, 6) and img.dtype == torch.float32 and float(img.max()) == 1.0


def test_result_processor_host_contract(dfepe, caplog, tmp_path):
    RP = dfepe.compat.eval_tools.Result_processor
    rp = RP(["epi_dist_mean_gt", "mscores", "num_matches"])
    assert rp.result_dict_all == {"epi_dist_mean_gt": [], "mscores": [], "num_matches": []} and rp.result_processed == {}
    with caplog.at_level(logging.WARNING):
        rp.load_result({"epi_dist_mean_gt": np.array([0.5, 2.0]), "mscores": np.array([0.1, 0.9]), "other": 1})
    assert "num_matches not in the result dictionary" in caplog.text
    rp.load_result({"epi_dist_mean_gt": np.array([1.5]), "mscores": np.array([0.3]), "num_matches": 1})
    got = rp.get_entry_from_result("epi_dist_mean_gt")
    assert len(got) == 2 and got[1][0] == 1.5 and rp.get_entry_from_result("num_matches") == [1]
    with caplog.at_level(logging.ERROR):
        assert rp.get_entry_from_result("absent") is None
    assert "absent is not in the dictionary." in caplog.text
    assert RP.get_mask([0.2, 1.0, np.nan, 0.99], 1.0).tolist() == [True, False, False, True]   # strict, NaN not kept
    assert RP.get_mask(np.array([0.5]), 1).dtype == bool
    rp.save_result(tmp_path / "r.npz", "something else")                        # only result_dict_all is ever saved
    assert not (tmp_path / "r.npz").exists()
    one = RP(["epi_dist_mean_gt"])
    one.load_result({"epi_dist_mean_gt": np.array([0.5, 2.0])})
    one.save_result(tmp_path / "r.npz", "result_dict_all")
    assert np.load(tmp_path / "r.npz")["epi_dist_mean_gt"].tolist() == [[0.5, 2.0]]
    # the reference's assert on a mask of another length, made on the host before anything is shipped
    with pytest.raises(AssertionError, match="mask size not equal to estimated arr"):
        rp.inlier_ratio([np.zeros(3), np.zeros(2)], [1.0], mask_list=[np.zeros(3), np.zeros(5)])
    # nothing to evaluate needs no device
    r = rp.inlier_ratio([], [0.5, 1.0])
    assert r["inlier_ratio"].shape == (2,) and np.isnan(r["inlier_ratio"]).all() and r["num_corrs"].shape == (0,)
    assert "unpinned" in RP.ap_inlier_thd.__doc__.lower()


def test_point_tracker_two_frame_state(dfepe):
    PT = dfepe.compat.model_wrap.PointTracker
    with pytest.raises(ValueError):
        PT(max_length=3, nn_thresh=0.7).update(np.zeros((3, 4)), np.zeros((32, 4)))
    with pytest.raises(ValueError):
        PT(max_length=1)
    t = PT(max_length=2, nn_thresh=0.7)
    assert t.get_matches().shape == (4, 0) and t.get_mscores().shape == (0,)
    t.update(None, None)                                                        # the published tracker warns and returns
    assert t.get_matches().shape == (4, 0)
    t.clear_desc()
    assert t.last_desc is None
    with pytest.raises(AssertionError):
        t.update(np.zeros((3, 4)), np.zeros((32, 5)))
    assert "unpinned" in open(dfepe.compat.model_wrap.__file__).read()
