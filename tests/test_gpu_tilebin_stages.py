"""GPU: the tile binning stages (csrc/tilebin.hip) through fdgs_debug_tile_bin against tests/tilebin_oracle.py, at the sizes where the
code changes path.  Everything is an integer with one right answer: every comparison is array equality.

What is held to the oracle per case: the counters after the count pass and after the scan, ctl = (R, longest list), every tile's slice of the
scattered pairs as a sorted multiset (the arrival order is free), point_list, ranges, and the tile order (a permutation of the tiles that
obeys the class rule of tile_order_block).  Every output buffer, and the scratch, lies between two guard bands of a known pattern that
must come back untouched, and so must the part of pairs / point_list behind num_rendered.

Boundaries (cases: tests/tilebin_cases.py, their planted properties: tests/test_tilebin_oracle_host.py):
  tile_sort       n = 1, 2; TS_DIRECT 96 | 97; TS_ENDS 1024 | 1025; the instance caps 1024 / 2048 / 4096 / 8192 / 16384 and one more; a pile
                  of exactly rank_max | rank_max + 1 equal depths; 64 equal samples; the LDS size in 64-key steps (63, 64, 65)
  walk_rect_tiles BIN_BIG 48 | 49; wide, tall and whole-grid rectangles; the largest quotient of the wide path (300 x 300 tiles);
                  widths whose float-reciprocal quotient needs the correction step
  tile_bin_*      P around a wave and a workgroup; bin_rounds (T 8192 | 8193); LDS histogram | direct atomics (T 36864 | 36865); the flush
                  stride (T 4095, 4096, 4097)
  tile_scan       T % 4 != 0, T = 1, per_thread 4 | 8, the longest list in the last tile
  tile_order      gmax = 0, one hot tile, all tiles equal
  sparse lists    a tile at the cap, one over, far over;  the ctl[0] > capacity guard of a run-ahead launch
"""
import numpy as np
import pytest
import torch

import tilebin_cases as tc
import tilebin_oracle as to

pytestmark = pytest.mark.gpu

GUARD = 64                       # words on either side of every buffer (256 bytes: the buffers keep their alignment)
PAT = 0xA5A5A5A5


class _Binner:
    """fdgs_debug_tile_bin on numpy inputs; every buffer the library writes sits between guard bands."""

    def __init__(self, dev):
        from fdgs import _capi
        self.capi, self.dev = _capi, dev

    def _buf(self, words):
        return torch.full((GUARD + max(words, 1) + GUARD,), PAT - (1 << 32), dtype=torch.int32, device=self.dev)

    def call(self, case, sparse_cap=0, capacity=None, max_count=0, rect=None, grid_x=None, T=None):
        """Returns (rc, dict of the outputs as uint32 arrays); asserts the guard bands."""
        lib = self.capi.lib
        rect = case["rect"] if rect is None else rect
        grid_x = case["grid_x"] if grid_x is None else grid_x
        T = case["T"] if T is None else T
        P = int(rect.shape[0])
        if capacity is None:
            tile, _ = to.instances(case["rect"], case["grid_x"])
            capacity = max(T, 1) * sparse_cap if sparse_cap else max(int(tile.size), 1)
        Tw = max(T, 1)
        sizes = dict(counts=Tw, starts=Tw, ctl=2, pairs=2 * capacity, point_list=capacity, ranges=2 * Tw, order=Tw,
                     scratch=int(lib.fdgs_debug_tile_bin_scratch_bytes(Tw, capacity)) // 4)
        bufs = {k: self._buf(n) for k, n in sizes.items()}
        d_rect = torch.from_numpy(np.ascontiguousarray(rect).view(np.int16).copy()).to(self.dev)
        d_dep = torch.from_numpy(np.ascontiguousarray(case["depths"][:P]).copy()).to(self.dev)
        ptr = {k: b.data_ptr() + 4 * GUARD for k, b in bufs.items()}
        with torch.cuda.device(self.dev):
            rc = lib.fdgs_debug_tile_bin(P, d_rect.data_ptr(), d_dep.data_ptr(), grid_x, T, sparse_cap, capacity, max_count, ptr["counts"],
                                         ptr["starts"], ptr["ctl"], ptr["pairs"], ptr["point_list"], ptr["ranges"], ptr["order"],
                                         ptr["scratch"], self.capi.current_stream_handle(self.dev))
        torch.cuda.synchronize(self.dev)
        out = {}
        for k, b in bufs.items():
            a = b.cpu().numpy().view(np.uint32)
            assert (a[:GUARD] == PAT).all(), "%s: something wrote in front of `%s`" % (case["name"], k)
            assert (a[GUARD + max(sizes[k], 1):] == PAT).all(), "%s: something wrote behind `%s`" % (case["name"], k)
            out[k] = a[GUARD:GUARD + sizes[k]]
        out["capacity"] = capacity
        return rc, out

    def run(self, case, **kw):
        rc, out = self.call(case, **kw)
        assert rc == 0, self.capi.last_error()
        return out


@pytest.fixture(scope="module")
def binner(gpu_device):
    return _Binner(gpu_device)


_ORACLES = {}


def _oracle(case):
    """Computed once per case and shared (treated as read-only)."""
    if case["name"] not in _ORACLES:
        _ORACLES[case["name"]] = to.bin_compact(case["rect"], np.ascontiguousarray(case["depths"]).view(np.uint32), case["grid_x"], case["T"])
    return _ORACLES[case["name"]]


def _check_order(out, counts, gmax, name):
    np.testing.assert_array_equal(np.sort(out["order"]), np.arange(counts.size, dtype=np.uint32), err_msg=name + ": the tile order is no permutation")
    excess = to.order_breaks_class_rule(out["order"], counts, gmax)
    print("%s: tile order, largest (later - earlier) count minus the class width: %g" % (name, excess))
    assert excess <= 0, "%s: a longer list comes behind a shorter one of another class (by %g)" % (name, excess)


def _check_compact(case, out):
    o = _oracle(case)
    name, T, R = case["name"], case["T"], o["R"]
    np.testing.assert_array_equal(out["counts"], o["counts"], err_msg=name + ": counters after the count pass")
    np.testing.assert_array_equal(out["starts"], o["starts"], err_msg=name + ": counters after the scan")
    assert out["ctl"].tolist() == [R, o["longest"]], name + ": ctl"
    pairs = out["pairs"].reshape(-1, 2)
    # a tile's slice of the scattered pairs, sorted by (bits, id), is the oracle's list; the oracle's `tile` is the slice every slot belongs to
    srt = np.lexsort((pairs[:R, 1], pairs[:R, 0], o["tile"]))
    np.testing.assert_array_equal(pairs[:R, 1][srt], o["gid"], err_msg=name + ": ids of the scattered pairs, per tile")
    np.testing.assert_array_equal(pairs[:R, 0][srt], o["key"], err_msg=name + ": depth bits of the scattered pairs, per tile")
    assert (pairs[R:] == PAT).all() and (out["point_list"][R:] == PAT).all(), name + ": a write behind num_rendered"
    np.testing.assert_array_equal(out["point_list"][:R], o["point_list"], err_msg=name + ": point_list")
    np.testing.assert_array_equal(out["ranges"].reshape(T, 2), o["ranges"], err_msg=name + ": ranges")
    _check_order(out, o["counts"], o["longest"], name)
    return o


# ----------------------------------------------------------------------------------------------------------------
# list lengths x depth kinds
# ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", tc.DEPTH_KINDS)
@pytest.mark.parametrize("n", tc.LIST_LENGTHS)
def test_list_lengths(n, kind, binner):
    case = tc.list_case(n, kind)
    o = _check_compact(case, binner.run(case))
    assert o["longest"] == n or n < 40


@pytest.mark.parametrize("rank_max", [96, 8])
@pytest.mark.parametrize("n", [300, 3000])
def test_crowded_bucket_either_side_of_rank_max(n, rank_max, binner):
    """A pile of exactly rank_max equal depths stays on the ranking path, one more sends the tile to the LDS bitonic sort; both orders
    must be the oracle's (inside the pile: by id)."""
    try:
        binner.capi.lib.fdgs_debug_tile_sort_limits(0, 0 if rank_max == 96 else rank_max)
        for pile in (rank_max, rank_max + 1):
            case = tc.crowded_case(n, pile)
            _check_compact(case, binner.run(case))
    finally:
        binner.capi.lib.fdgs_debug_tile_sort_limits(0, 0)


@pytest.mark.parametrize("n", [1024, 2048])
def test_all_64_samples_equal(n, binner):
    """All splitters are one value: two buckets (n <= 1024) or the two end intervals only (longer lists).  Whether the samples really were
    equal is read off the scattered pairs (arrival order) and printed; tests/tilebin_cases.equal_samples_case says why they are."""
    case = tc.equal_samples_case(n)
    out = binner.run(case)
    o = _check_compact(case, out)
    s = int(o["starts"][case["hot"]])
    samples = out["pairs"].reshape(-1, 2)[s + ((np.arange(64) * n) >> 6), 0]
    print("%s: distinct depths among the 64 samples: %d" % (case["name"], len(np.unique(samples))))
    assert (samples == case["sample_depth"].view(np.uint32)).all()


@pytest.mark.parametrize("limits", [(64, 0), (0, 1), (2, 0)], ids=["global-scratch", "lds-bitonic", "all-global"])
@pytest.mark.parametrize("n", [97, 1025, 4097])
def test_debug_limits(n, limits, binner):
    try:
        binner.capi.lib.fdgs_debug_tile_sort_limits(*limits)
        for kind in ("uniform", "two_values"):
            case = tc.list_case(n, kind)
            _check_compact(case, binner.run(case))
    finally:
        binner.capi.lib.fdgs_debug_tile_sort_limits(0, 0)


# ----------------------------------------------------------------------------------------------------------------
# rectangles, P and T
# ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", list(tc.RECT_SHAPES))
def test_single_rectangles(shape, binner):
    case = tc.rect_single_case(shape)
    _check_compact(case, binner.run(case))


@pytest.mark.parametrize("seed", [0, 1])
def test_rectangle_mix(seed, binner):
    case = tc.rect_mix_case(seed=seed)
    _check_compact(case, binner.run(case))


def test_largest_quotient_of_the_wide_path(binner):
    case = tc.big_grid_case()
    o = _check_compact(case, binner.run(case))
    assert o["R"] == 90000 + 299 + 299 and o["longest"] == 3 and o["counts"][-1] == 3      # the last tile lies in all three


@pytest.mark.parametrize("which", ["lds", "direct"])
def test_wide_path_widths_that_need_the_correction_step(which, binner):
    """Widths at which the float-reciprocal quotient is one short (41, 47, 55, 61, ...): without the correction step the second row of
    such a rectangle starts one row too high and a width to the right."""
    case = tc.wide_correction_case() if which == "lds" else tc.big_grid_widths_case()
    _check_compact(case, binner.run(case))


@pytest.mark.parametrize("P", tc.P_EDGES)
def test_p_edges(P, binner):
    case = tc.p_edge_case(P)
    _check_compact(case, binner.run(case))


@pytest.mark.parametrize("T", tc.T_EDGES)
def test_t_edges(T, binner):
    case = tc.t_edge_case(T)
    o = _check_compact(case, binner.run(case))
    assert o["counts"][-1] == o["longest"] >= 1


@pytest.mark.parametrize("kind", ["all_empty", "one_hot", "all_equal"])
def test_tile_order_corner_cases(kind, binner):
    case = tc.order_case(kind)
    out = binner.run(case)
    o = _check_compact(case, out)
    if kind == "all_empty":
        assert out["ctl"].tolist() == [0, 0] and not out["ranges"].any()
    if kind == "one_hot":
        assert out["order"][0] == 40 and o["longest"] == 500


# ----------------------------------------------------------------------------------------------------------------
# the capacity guard, sparse lists, reproducibility, refused arguments
# ----------------------------------------------------------------------------------------------------------------

def test_capacity_guard_of_a_run_ahead_launch(binner):
    """num_rendered = capacity + 1: scatter and sort leave pairs and point_list alone and every tile is reported empty; count, scan and
    ctl are what they always are.  num_rendered = capacity: an ordinary result."""
    case = tc.rect_mix_case(seed=0)
    o = _oracle(case)
    out = binner.run(case, capacity=o["R"] - 1)
    np.testing.assert_array_equal(out["counts"], o["counts"])
    np.testing.assert_array_equal(out["starts"], o["starts"])
    assert out["ctl"].tolist() == [o["R"], o["longest"]]
    assert (out["pairs"] == PAT).all() and (out["point_list"] == PAT).all(), "the guard let a pass write into buffers that are too small"
    assert not out["ranges"].any()
    _check_compact(case, binner.run(case, capacity=o["R"]))


@pytest.mark.parametrize("cap", tc.SPARSE_CAPS)
def test_sparse_lists(cap, binner):
    case = tc.sparse_case(cap)
    T = case["T"]
    o = to.bin_sparse(case["rect"], np.ascontiguousarray(case["depths"]).view(np.uint32), case["grid_x"], T, cap)
    out = binner.run(case, sparse_cap=cap)
    name = case["name"]
    c = o["compact"]
    np.testing.assert_array_equal(out["counts"], o["counts"], err_msg=name + ": the tiles' counts (true counts, over the cap too)")
    assert out["ctl"].tolist() == [o["R"], o["longest"]] and out["ctl"][1] > cap      # the overflow is reported through the longest list
    np.testing.assert_array_equal(out["ranges"].reshape(T, 2), o["ranges"], err_msg=name + ": ranges")
    assert (out["starts"] == PAT).all()
    pairs, pl = out["pairs"].reshape(T, cap, 2), out["point_list"].reshape(T, cap)
    weak = 0
    for t in range(T):
        n, s = int(o["counts"][t]), int(c["starts"][t])
        want_k, want_g = c["key"][s:s + n], c["gid"][s:s + n]
        st = int(o["stored"][t])
        assert (pairs[t, st:] == PAT).all() and (pl[t, st:] == PAT).all(), "%s: tile %d wrote beyond its %d entries" % (name, t, st)
        got = pairs[t, :st]
        srt = np.lexsort((got[:, 1], got[:, 0]))
        if not o["over"][t]:
            np.testing.assert_array_equal(got[srt, 1], want_g, err_msg="%s: tile %d pairs" % (name, t))
            np.testing.assert_array_equal(got[srt, 0], want_k, err_msg="%s: tile %d pairs" % (name, t))
            np.testing.assert_array_equal(pl[t, :st], want_g, err_msg="%s: tile %d point_list" % (name, t))
        else:
            # which cap of its instances arrived first is free: distinct members of the oracle's set, in (bits, id) order
            weak += 1
            bits_of = dict(zip(want_g.tolist(), want_k.tolist()))
            ids = got[:, 1].tolist()
            assert st == cap and len(set(ids)) == cap and all(g in bits_of and bits_of[g] == k for k, g in got.tolist()), (name, t)
            np.testing.assert_array_equal(pl[t], got[srt, 1], err_msg="%s: tile %d (over the cap) is not in (bits, id) order" % (name, t))
    assert weak == 2
    _check_order(out, o["counts"], o["longest"], name)


def test_same_case_twice_with_another_in_between(binner):
    a = tc.list_case(4097, "sliver_plus_outliers")
    b = tc.rect_mix_case(seed=0)
    first = {}
    for case in (a, b, a, b):
        out = binner.run(case)
        _check_compact(case, out)
        if case["name"] in first:
            np.testing.assert_array_equal(out["point_list"], first[case["name"]]["point_list"])
            np.testing.assert_array_equal(out["ranges"], first[case["name"]]["ranges"])
        first.setdefault(case["name"], out)


def test_refused_arguments_launch_nothing(binner):
    case = tc.rect_mix_case(seed=0)
    o = _oracle(case)

    def refused(what, **kw):
        kw.setdefault("capacity", o["R"])
        rc, out = binner.call(case, **kw)
        assert rc == 1 and "fdgs_debug_tile_bin" in binner.capi.last_error() and what in binner.capi.last_error(), binner.capi.last_error()
        for k in ("counts", "starts", "ctl", "pairs", "point_list", "ranges", "order", "scratch"):
            assert (out[k] == PAT).all(), k
    refused("T = 0", T=0)
    refused("T = -3", T=-3)
    refused("grid_x = 0", grid_x=0)
    bad = case["rect"].copy()
    bad[11] = [38, 2, 41, 3]          # x1 > grid_x
    refused("rectangle 11", rect=bad)
    bad = case["rect"].copy()
    bad[64] = [0, 29, 1, 31]          # y1 * grid_x > T
    refused("rectangle 64", rect=bad)
    bad = case["rect"].copy()
    bad[0] = [5, 5, 4, 6]             # x0 > x1: a width of 65535 after the unsigned subtraction
    refused("rectangle 0", rect=bad)
    refused("rectangle", T=case["T"] - 1)                         # a grid one tile short of what the rectangles reach
    refused("capacity", sparse_cap=64, capacity=64 * case["T"] - 1)
    lib = binner.capi.lib
    small = torch.zeros(4096, dtype=torch.int32, device=binner.dev).data_ptr()       # (T >= 2^24 is refused before anything is sized by it)
    assert lib.fdgs_debug_tile_bin(1, small, small, 4096, 1 << 24, 0, 10, 0, small, small, small, small, small, small, small, small, None) == 1
    assert "T = 16777216" in binner.capi.last_error()
    assert lib.fdgs_debug_tile_bin(65, None, None, 40, 1200, 0, 10, 0, None, None, None, None, None, None, None, None, None) == 1
    assert "NULL" in binner.capi.last_error()
    b = [lib.fdgs_debug_tile_bin_scratch_bytes(T, R) for T, R in ((1, 1), (1200, 5000), (90000, 90598))]
    assert all(x % 256 == 0 for x in b) and b[0] < b[1] < b[2] and b[2] >= 90000 * 4 * 4 + 90598 * 8
