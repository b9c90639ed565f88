"""CPU: the contribution-statistics entry of the C ABI (fdgs_contribution: exported, struct sizes, argument errors -- nothing is
launched) and the host side of fdgs.importance (scores, the keep-fraction selection)."""
import ctypes as C

import pytest
import torch


def test_symbol_is_exported_and_struct_sizes_match():
    from fdgs import _capi
    assert "fdgs_contribution" in _capi.EXPORTED and hasattr(_capi.lib, "fdgs_contribution")
    cin, cout = _capi.FdgsContributionIn(), _capi.FdgsContributionOut()
    # include/fdgs.h on a 64-bit target: 4 x 4 bytes, three pointers, an int32 (+ padding), a pointer / a uint32 (+ padding), five pointers
    assert cin.struct_size == C.sizeof(_capi.FdgsContributionIn) == 56 and cout.struct_size == C.sizeof(_capi.FdgsContributionOut) == 48
    assert [f[0] for f in _capi.FdgsContributionIn._fields_] == ["struct_size", "P", "W", "H", "geom_buffer", "binning_buffer", "image_buffer",
                                                                "num_rendered", "pix_weight"]
    assert [f[0] for f in _capi.FdgsContributionOut._fields_] == ["struct_size", "weight_sum", "weight_max", "hits", "dominant", "dominant_id"]
    # the library agrees with both sizes: with them it gets as far as the argument checks behind the size checks
    cin.P, cin.W, cin.H = 5, 16, 16
    assert _capi.lib.fdgs_contribution(C.byref(cin), C.byref(cout), None) == 1
    assert "struct_size" not in _capi.last_error() and "every output is NULL" in _capi.last_error()
    assert _capi.lib.fdgs_version() == 502


def test_argument_errors_are_reported():
    from fdgs import _capi
    fn = _capi.lib.fdgs_contribution
    cin, cout = _capi.FdgsContributionIn(), _capi.FdgsContributionOut()
    cin.P, cin.W, cin.H = 5, 16, 16
    dummy = (C.c_float * 4)()
    cout.weight_sum = C.addressof(dummy)
    assert fn(None, C.byref(cout), None) == 1 and fn(C.byref(cin), None, None) == 1
    cin.struct_size -= 8
    assert fn(C.byref(cin), C.byref(cout), None) == 1 and "fdgs_contribution_in" in _capi.last_error() and "struct_size" in _capi.last_error()
    cin.struct_size += 8
    cout.struct_size += 8
    assert fn(C.byref(cin), C.byref(cout), None) == 1 and "fdgs_contribution_out" in _capi.last_error()
    cout.struct_size -= 8
    for P, W, H in ((-1, 16, 16), (5, 0, 16), (5, 16, -3), (1 << 26, 16, 16)):
        cin.P, cin.W, cin.H = P, W, H
        assert fn(C.byref(cin), C.byref(cout), None) == 1 and "bad sizes" in _capi.last_error(), (P, W, H)
    cin.P, cin.W, cin.H = 5, 16, 16
    for R in (7, -1, 0):   # P > 0 but no buffers: refused whatever num_rendered says
        cin.num_rendered = R
        assert fn(C.byref(cin), C.byref(cout), None) == 1 and "must not be NULL" in _capi.last_error(), R
    cout.weight_sum = None
    assert fn(C.byref(cin), C.byref(cout), None) == 1 and "every output is NULL" in _capi.last_error()


def test_python_entry_points_refuse_cpu_tensors():
    from fdgs import importance
    e = torch.empty(0, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        importance.contribution_pass(4, 8, 8, e, e, e, 0, weight_sum=torch.zeros(4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        importance.contribution_pass(4, 8, 8, e, e, e, 0, dominant_id=torch.zeros((8, 8), dtype=torch.int32))


def _stats(ws, wm=None, hits=None, dom=None):
    from fdgs.importance import ContributionStats
    s = ContributionStats(len(ws), "cpu")
    s.weight_sum = torch.tensor(ws, dtype=torch.float32)
    s.weight_max = torch.tensor(wm if wm is not None else ws, dtype=torch.float32).clamp(max=0.99)
    s.hits = torch.tensor(hits if hits is not None else [int(w > 0) for w in ws], dtype=torch.int32)
    s.dominant = torch.tensor(dom if dom is not None else [0] * len(ws), dtype=torch.int32)
    return s


def test_score_kinds_and_volume_power():
    s = _stats([1.0, 4.0, 0.0, 2.0], wm=[0.5, 0.75, 0.0, 0.25], dom=[3, 0, 0, 7])
    assert s.score().tolist() == [1.0, 4.0, 0.0, 2.0] and s.score("sum").tolist() == s.score().tolist()
    assert s.score("max").tolist() == [0.5, 0.75, 0.0, 0.25] and s.score("dominant").tolist() == [3.0, 0.0, 0.0, 7.0]
    assert s.score("dominant").dtype == torch.float32
    with pytest.raises(ValueError):
        s.score("mean")
    with pytest.raises(ValueError, match="scales"):
        s.score("sum", volume_power=0.5)
    s.scales = torch.tensor([[1.0, 2.0, 2.0], [1.0, 1.0, 1.0], [3.0, 3.0, 3.0], [0.5, 0.5, 4.0]])
    torch.testing.assert_close(s.score("sum", volume_power=0.5), torch.tensor([2.0, 4.0, 0.0, 2.0]))
    torch.testing.assert_close(s.score("sum", volume_power=-1.0), torch.tensor([0.25, 4.0, 0.0, 2.0]))
    assert s.score("sum", volume_power=0.0).tolist() == [1.0, 4.0, 0.0, 2.0]
    s.score("sum")[0] = 99.0   # a copy: the statistics are not aliased
    assert s.weight_sum[0] == 1.0
    s.views = 3
    assert s.zero_() is s and s.views == 0 and float(s.weight_sum.abs().sum() + s.weight_max.abs().sum()) == 0.0 and int(s.hits.sum()) == 0


def test_keep_fraction_keeps_ties_order_and_one_survivor():
    s = _stats([5.0, 1.0, 3.0, 3.0, 0.0, 3.0, 7.0, 2.0])
    assert s.keep_mask(keep_fraction=1.0).all()
    assert s.keep_mask(keep_fraction=0.25).tolist() == [True, False, False, False, False, False, True, False]       # top 2
    # top 3 of 8 = 0.375: the third place is a three-way tie at 3.0 -- all of it is kept
    assert s.keep_mask(keep_fraction=0.375).tolist() == [True, False, True, True, False, True, True, False]
    assert s.keep_mask(keep_fraction=0.5).tolist() == [True, False, True, True, False, True, True, False]           # top 4: inside the tie
    assert s.keep_mask(keep_fraction=0.01).tolist() == [False] * 6 + [True, False]                                  # at least one
    # surviving rows keep their order: the selection is a mask over the rows, nothing is sorted
    idx = torch.nonzero(s.keep_mask(keep_fraction=0.5)).flatten()
    assert idx.tolist() == sorted(idx.tolist()) == [0, 2, 3, 5, 6]
    for bad in (0.0, -0.5, 1.5):
        with pytest.raises(ValueError):
            s.keep_mask(keep_fraction=bad)
    # everything zero: every Gaussian ties at the cut, all are kept
    assert _stats([0.0] * 5).keep_mask(keep_fraction=0.2).all()


def test_thresholds_combine_and_never_empty_the_model():
    s = _stats([5.0, 1.0, 3.0, 0.0], wm=[0.9, 0.002, 0.5, 0.0], hits=[40, 1, 9, 0], dom=[6, 0, 1, 0])
    assert s.keep_mask(min_hits=1).tolist() == [True, True, True, False]
    assert s.keep_mask(min_weight_max=0.01).tolist() == [True, False, True, False]
    assert s.keep_mask(min_dominant=1).tolist() == [True, False, True, False]
    assert s.keep_mask(min_hits=1, min_dominant=2).tolist() == [True, False, False, False]
    assert s.keep_mask(keep_fraction=0.75, min_hits=10).tolist() == [True, False, False, False]
    assert s.keep_mask(min_hits=1000).tolist() == [True, False, False, False]       # nothing passes: the best by summed weight stays
    assert s.keep_mask().all()
    s.select_(torch.tensor([0, 2]))
    assert s.P == 2 and s.weight_sum.tolist() == [5.0, 3.0] and s.hits.tolist() == [40, 9] and s.dominant.tolist() == [6, 1]
