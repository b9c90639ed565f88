"""CPU: tests/tilebin_oracle.py against a per-instance loop, and every planned case of tests/tilebin_cases.py against the property it was
built for (the GPU tests of tests/test_gpu_tilebin_stages.py rely on both)."""
import numpy as np
import pytest

import tilebin_cases as tc
import tilebin_oracle as to


def _brute(rect, bits, grid_x, T):
    """Instance by instance: per-tile lists of (bits, gid), sorted; counts; starts; point_list; ranges."""
    lists = [[] for _ in range(T)]
    for g, (x0, y0, x1, y1) in enumerate(np.asarray(rect).tolist()):
        for y in range(y0, y1):
            for x in range(x0, x1):
                lists[y * grid_x + x].append((int(bits[g]), g))
    counts = [len(l) for l in lists]
    starts, run = [], 0
    for c in counts:
        starts.append(run)
        run += c
    pl = [g for l in lists for _, g in sorted(l)]
    ranges = [(s, s + c) if c else (0, 0) for s, c in zip(starts, counts)]
    return lists, counts, starts, pl, ranges


def _bits(case):
    return np.ascontiguousarray(case["depths"]).view(np.uint32)


def _counts(case):
    tile, _ = to.instances(case["rect"], case["grid_x"])
    assert tile.size == 0 or (tile.min() >= 0 and tile.max() < case["T"])
    return np.bincount(tile, minlength=case["T"])


def _depths_ok(case):
    d = case["depths"]
    assert d.dtype == np.float32 and d.shape == (case["rect"].shape[0],) and case["rect"].dtype == np.uint16
    assert np.isfinite(d).all() and (d >= np.float32(0.2)).all(), case["name"]


SMALL = [tc.list_case(1, "uniform"), tc.list_case(65, "two_values"), tc.list_case(97, "all_equal"), tc.rect_mix_case(), tc.rect_mix_case(seed=1),
         tc.rect_single_case("7x7"), tc.rect_single_case("40x30"), tc.p_edge_case(65), tc.t_edge_case(5), tc.t_edge_case(1023),
         tc.wide_correction_case(), tc.order_case("all_empty"), tc.order_case("all_equal"), tc.sparse_case(64)]


@pytest.mark.parametrize("case", SMALL, ids=[c["name"] for c in SMALL])
def test_oracle_matches_a_per_instance_loop(case):
    bits = _bits(case)
    lists, counts, starts, pl, ranges = _brute(case["rect"], bits, case["grid_x"], case["T"])
    o = to.bin_compact(case["rect"], bits, case["grid_x"], case["T"])
    assert o["counts"].tolist() == counts and o["starts"].tolist() == starts
    assert o["R"] == sum(counts) and o["longest"] == max(counts)
    assert o["point_list"].tolist() == pl and o["ranges"].tolist() == [list(r) for r in ranges]
    for t in range(case["T"]):
        s, c = starts[t], counts[t]
        assert list(zip(o["key"][s:s + c].tolist(), o["gid"][s:s + c].tolist())) == sorted(lists[t])
        assert (o["tile"][s:s + c] == t).all()


def test_sparse_oracle_matches_a_per_instance_loop():
    case = tc.sparse_case(64)
    cap, T = 64, case["T"]
    bits = _bits(case)
    lists, counts, _, _, _ = _brute(case["rect"], bits, case["grid_x"], T)
    o = to.bin_sparse(case["rect"], bits, case["grid_x"], T, cap)
    assert o["counts"].tolist() == counts and o["R"] == sum(counts) and o["longest"] == max(counts) == 4 * cap
    for t in range(T):
        c = counts[t]
        assert bool(o["over"][t]) == (c > cap) and o["stored"][t] == min(c, cap)
        assert o["ranges"][t].tolist() == ([t * cap, t * cap + min(c, cap)] if c else [0, 0])
        want = [g for _, g in sorted(lists[t])] + [-1] * (cap - c) if c <= cap else [-1] * cap
        assert o["point_list"][t * cap:(t + 1) * cap].tolist() == want


def test_class_rule_helper():
    counts = np.asarray([0, 640, 10, 5, 640, 300])
    assert to.order_breaks_class_rule([1, 4, 5, 2, 3, 0], counts, 640) <= 0
    assert to.order_breaks_class_rule([4, 1, 5, 3, 2, 0], counts, 640) <= 0          # 10 and 5 differ by less than 641 / 64 + 1
    assert to.order_breaks_class_rule([1, 4, 2, 5, 3, 0], counts, 640) > 0           # 300 behind 10
    assert to.order_breaks_class_rule([0, 1, 4, 5, 2, 3], counts, 640) > 0
    assert to.order_breaks_class_rule([0], counts[:1], 0) <= 0


@pytest.mark.parametrize("kind", tc.DEPTH_KINDS)
@pytest.mark.parametrize("n", tc.LIST_LENGTHS)
def test_list_cases_hold_exactly_n_entries_of_their_kind(n, kind):
    case = tc.list_case(n, kind)
    _depths_ok(case)
    counts = _counts(case)
    hot = case["hot"]
    assert case["T"] == 8 and counts[hot] == n
    others = np.delete(counts, hot)
    assert (others >= 1).all() and (others < 40).all()
    mine = (case["rect"][:, 0].astype(int) + 4 * case["rect"][:, 1].astype(int)) == hot
    assert (case["rect"][:, 2] - case["rect"][:, 0] == 1).all() and (case["rect"][:, 3] - case["rect"][:, 1] == 1).all()
    d = case["depths"][mine]           # in id order
    b = d.view(np.uint32).astype(np.int64)
    if kind == "all_equal":
        assert len(np.unique(b)) == 1
    elif kind == "two_values":
        assert len(np.unique(b)) == (2 if n > 8 else len(np.unique(b))) and len(np.unique(b)) <= 2
    elif kind == "low_bits_only":
        assert np.array_equal(np.sort(b), b.min() + np.arange(n)) and (b.max() >> 16) == (b.min() >> 16)
    elif kind == "descending_in_id":
        assert (np.diff(b) <= 0).all() and (n < 3 or b[0] > b[-1])
    elif kind == "ascending_in_id":
        assert (np.diff(b) >= 0).all() and (n < 3 or b[0] < b[-1])
    elif kind == "sliver_plus_outliers":
        inside = np.abs(d.astype(np.float64) / 2.0 - 1.0) <= 1.001e-4
        if n >= 1024:
            assert 0.98 <= inside.mean() < 1.0
            out = d[~inside].astype(np.float64)
            assert out.max() / out.min() > 100.0 and out.min() >= 0.2
    if n > 2 and kind in ("uniform", "sliver_plus_outliers"):
        assert not (np.diff(b) >= 0).all() and not (np.diff(b) <= 0).all()     # the interleaving left the list unsorted


@pytest.mark.parametrize("rank_max", [96, 8])
@pytest.mark.parametrize("n", [300, 3000])
def test_crowded_cases_hold_a_pile_of_exactly_k_ties(n, rank_max):
    for pile in (rank_max, rank_max + 1):
        case = tc.crowded_case(n, pile)
        _depths_ok(case)
        assert _counts(case)[case["hot"]] == n
        mine = (case["rect"][:, 0].astype(int) + 4 * case["rect"][:, 1].astype(int)) == case["hot"]
        d = case["depths"][mine]
        vals, cnt = np.unique(d.view(np.uint32), return_counts=True)
        assert cnt.max() == pile and (cnt > 1).sum() == 1 and vals[cnt.argmax()] == case["pile_depth"].view(np.uint32)
        rest = d[d != case["pile_depth"]]
        assert rest.size == n - pile and (np.abs(rest - case["pile_depth"]) > 0.01 * case["pile_depth"]).all()


@pytest.mark.parametrize("n", [1024, 2048])
def test_equal_sample_cases(n):
    case = tc.equal_samples_case(n)
    _depths_ok(case)
    assert _counts(case)[case["hot"]] == n and case["step"] >= 16 and case["step"] % 16 == 0
    hot_ids = np.nonzero((case["rect"][:, 0].astype(int) + 4 * case["rect"][:, 1].astype(int)) == case["hot"])[0]
    assert np.array_equal(hot_ids, np.arange(n))                      # whole waves and workgroups of the hot tile's own Gaussians
    d = case["depths"][:n]
    v = case["sample_depth"]
    # every arrival position p = id + 64 * k (blocks of 64 permuted) that is a sample position (lane * n >> 6) carries v ...
    sample_pos = (np.arange(64) * n) >> 6
    assert (sample_pos % 16 == 0).all()
    assert (d[np.arange(n) % 16 == 0] == v).all() and (d[np.arange(n) % 16 != 8] == v).all()
    # ... and the rest does not: n / 16 other depths, all distinct
    rest = d[np.arange(n) % 16 == 8]
    assert (rest != v).all() and len(np.unique(rest)) == n // 16


@pytest.mark.parametrize("shape", list(tc.RECT_SHAPES))
def test_single_rectangle_cases(shape):
    case = tc.rect_single_case(shape)
    _depths_ok(case)
    gx, gy = tc.RECT_GRID
    r = case["rect"].astype(int)
    assert r.shape[0] == 65 and case["T"] == gx * gy == 1200
    w, h = r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]
    assert (w[case["at"]], h[case["at"]]) == tc.RECT_SHAPES[shape]
    rest = np.delete(np.arange(65), case["at"])
    assert ((w[rest] == 0) | (h[rest] == 0)).all() and (w[rest] == 0).any() and (h[rest] == 0).any()
    assert _counts(case).sum() == w[case["at"]] * h[case["at"]]
    assert (r[:, 2] <= gx).all() and (r[:, 3] <= gy).all()


def test_rectangle_shapes_sit_on_both_sides_of_the_wide_path():
    area = {k: w * h for k, (w, h) in tc.RECT_SHAPES.items()}
    assert area["6x8"] == 48 and area["7x7"] == 49 and area["1x30"] == 30 and area["40x1"] == 40 and area["40x30"] == 1200
    assert area["empty_w"] == 0 and area["empty_h"] == 0 and tc.RECT_SHAPES["empty_w"][0] == 0 and tc.RECT_SHAPES["empty_h"][1] == 0
    for seed in (0, 1):
        case = tc.rect_mix_case(seed=seed)
        _depths_ok(case)
        gx, gy = tc.RECT_GRID
        r = case["rect"].astype(int)
        w, h = r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]
        assert r.shape[0] == 65 and {(a, b) for a, b in zip(w.tolist(), h.tolist())} == set(tc.RECT_SHAPES.values())
        assert ((r[:, 2] == gx) & (w > 0) & (h > 0) & (w < gx)).any() and ((r[:, 3] == gy) & (w > 0) & (h > 0) & (h < gy)).any()
        assert (r[:, 2] <= gx).all() and (r[:, 3] <= gy).all()
    big = tc.big_grid_case()
    _depths_ok(big)
    r = big["rect"].astype(int)
    assert big["T"] == 90000 > 36 * 1024 and big["grid_x"] == 300
    assert sorted(zip((r[:, 2] - r[:, 0]).tolist(), (r[:, 3] - r[:, 1]).tolist())) == [(1, 299), (299, 1), (300, 300)]
    assert (r[:, 2] == 300).all() and (r[:, 3] == 300).all()


def test_wide_path_cases_need_the_correction_step():
    """The wide path divides by a float reciprocal and corrects the quotient by one either way.  With a correctly rounded reciprocal no
    rectangle of the 40 x 30 grid and none of the three of the 300 x 300 case needs that step; the widths planted here do, at s = w."""
    for gx, gy in ((40, 30), (300, 300), (299, 1), (1, 299)):
        assert not any(tc.quotient_needs_correction(w, gy) for w in (range(1, 41) if gx == 40 else [gx]))
    for case, widths in ((tc.wide_correction_case(), tc.WIDE_WIDTHS), (tc.big_grid_widths_case(), tc.BIG_WIDE_WIDTHS)):
        _depths_ok(case)
        r = case["rect"].astype(int)
        w, h = r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]
        assert set(w.tolist()) == set(widths) and (w * h > 48).all() and (h >= 2).all()
        assert all(tc.quotient_needs_correction(a, b) for a, b in zip(w.tolist(), h.tolist()))
        assert (r[:, 0] >= 1).all() and (w < case["grid_x"]).all()          # a quotient one short lands in another tile
        assert (r[:, 2] <= case["grid_x"]).all() and (r[:, 3] * case["grid_x"] <= case["T"]).all()
        _counts(case)
    assert tc.wide_correction_case()["T"] <= 8192 and tc.big_grid_widths_case()["T"] > 36 * 1024


@pytest.mark.parametrize("P", tc.P_EDGES)
def test_p_edge_cases(P):
    case = tc.p_edge_case(P)
    _depths_ok(case)
    assert case["rect"].shape[0] == P and case["T"] == 256 and case["grid_x"] == 16
    counts = _counts(case)
    assert counts[-1] >= 1 and case["rect"][P - 1].tolist() == [15, 15, 16, 16]
    if P > 97:
        r = case["rect"].astype(int)
        assert ((r[:, 2] - r[:, 0]) * (r[:, 3] - r[:, 1]) > 48).any()


@pytest.mark.parametrize("T", tc.T_EDGES)
def test_t_edge_cases(T):
    case = tc.t_edge_case(T)
    _depths_ok(case)
    gx = case["grid_x"]
    assert case["T"] == T and T % gx == 0
    if gx == T and T > 3:
        assert all(T % d for d in range(2, T))          # grid_x = T only where T has no divisor
    counts = _counts(case)
    assert counts[-1] == counts.max() and counts[-1] >= 1 and (T == 1 or counts[-1] > counts[:-1].max())
    assert 300 < case["rect"].shape[0] < 1024


def test_t_edges_straddle_the_code_paths():
    t = tc.T_EDGES
    assert 1 in t and any(x % 4 for x in t)
    for a, b in ((8192, 8193), (36864, 36865), (4096, 4097)):      # bin_rounds, LDS histogram | direct atomics, flush stride and per_thread 4 | 8
        assert a in t and b in t
    assert 4095 in t and 1025 in t                                 # per_thread 4 (T <= 4096) with a ragged last uint4; just over one trip of 1024
    assert tc.grid_for(36865) * (36865 // tc.grid_for(36865)) == 36865 and tc.grid_for(5) == 5 and tc.grid_for(4096) == 64


@pytest.mark.parametrize("kind", ["all_empty", "one_hot", "all_equal"])
def test_order_cases(kind):
    case = tc.order_case(kind)
    _depths_ok(case)
    counts = _counts(case)
    if kind == "all_empty":
        assert counts.sum() == 0 and case["rect"].shape[0] >= 1
    elif kind == "one_hot":
        assert (counts > 0).sum() == 1 and counts.max() == 500
    else:
        assert (counts == counts[0]).all() and counts[0] == 5


@pytest.mark.parametrize("cap", tc.SPARSE_CAPS)
def test_sparse_cases_plant_exactly_two_tiles_over_the_cap(cap):
    case = tc.sparse_case(cap)
    _depths_ok(case)
    counts = _counts(case)
    T = case["T"]
    assert T == 120 and case["grid_x"] == 12
    assert sorted(case["spots"].values()) == [cap - 1, cap, cap + 1, 4 * cap]
    for t, n in case["spots"].items():
        assert counts[t] == n
    over = np.nonzero(counts > cap)[0]
    assert sorted(over.tolist()) == sorted(t for t, n in case["spots"].items() if n > cap) and over.size == 2 and over.size <= 2 * T // 120
    assert (counts == 0).sum() >= T // 4 and ((counts > 0) & (counts < cap - 1)).sum() >= T // 2
