"""CPU: tests/sort_oracle.py (the reference the radix sort and the k-NN stages are held to on the GPU) pinned on small inputs whose
answers are computed here by hand or by the plainest possible Python."""
import numpy as np
import pytest

import sort_oracle as so


def _interleave(cx, cy, cz):
    code = 0
    for b in range(10):
        code |= ((cx >> b) & 1) << (3 * b) | ((cy >> b) & 1) << (3 * b + 1) | ((cz >> b) & 1) << (3 * b + 2)
    return code


@pytest.mark.parametrize("bit_lo,bit_hi", [(0, 32), (0, 8), (8, 32), (8, 24), (24, 32), (16, 16), (4, 12)])
def test_stable_sort_pairs_vs_python_sorted(bit_lo, bit_hi):
    rng = np.random.default_rng(bit_lo * 33 + bit_hi)
    n = 300
    keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    keys[::3] = keys[1]                       # many equal keys
    keys[5], keys[6] = 0xFFFFFFFF, 0
    vals = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    digit = [(int(k) >> bit_lo) & ((1 << (bit_hi - bit_lo)) - 1) for k in keys]
    perm = sorted(range(n), key=lambda i: (digit[i], i))
    got_k, got_v = so.stable_sort_pairs(keys, vals, bit_lo, bit_hi)
    assert got_k.dtype == np.uint32 and got_v.dtype == np.uint32
    np.testing.assert_array_equal(got_k, keys[perm])
    np.testing.assert_array_equal(got_v, vals[perm])
    if bit_lo == bit_hi:
        np.testing.assert_array_equal(got_k, keys)
        np.testing.assert_array_equal(got_v, vals)


def test_stable_sort_pairs_keeps_input_order_of_ties():
    keys = np.array([0x00AA0001, 0x00AA0000, 0x00BB0003, 0x00AA0002], np.uint32)   # bits [16, 24): AA AA BB AA
    k, v = so.stable_sort_pairs(keys, np.arange(4, dtype=np.uint32), 16, 24)
    np.testing.assert_array_equal(v, [0, 1, 3, 2])
    np.testing.assert_array_equal(k, keys[[0, 1, 3, 2]])
    k, v = so.stable_sort_pairs(keys, np.arange(4, dtype=np.uint32), 0, 32)
    np.testing.assert_array_equal(v, [1, 0, 3, 2])


def test_prep_morton_spreads_ten_bits():
    for x in (0, 1, 2, 0x155, 0x2AA, 511, 512, 1023):
        assert int(so.prep_morton(np.uint32(x))) == _interleave(x, 0, 0)
    assert int(so.prep_morton(np.uint32(1023))) == 0x09249249


def test_morton_stage_origin_inclusion_and_max_corner():
    """Every point lies in the positive octant away from the origin: the origin sets the minimum on every axis.  The second point is
    the max corner: 1023 on every axis, the largest 30-bit code."""
    bounds, codes = so.morton_stage(np.array([[1.0, 2.0, 4.0], [2.0, 4.0, 8.0]], np.float32))
    np.testing.assert_array_equal(bounds, np.array([0, 0, 0, 2, 4, 8], np.float32))
    # (1 - 0) / 2 * 1023 = 511.5 -> 511 on every axis
    assert int(codes[0]) == _interleave(511, 511, 511)
    assert int(codes[1]) == _interleave(1023, 1023, 1023) == 0x3FFFFFFF
    # without the origin the first point would be the min corner, code 0
    assert int(codes[0]) != 0


def test_morton_stage_origin_sets_the_maximum():
    bounds, codes = so.morton_stage(np.array([[-4.0, -8.0, -1.0], [-1.0, -2.0, -0.25]], np.float32))
    np.testing.assert_array_equal(bounds, np.array([-4, -8, -1, 0, 0, 0], np.float32))
    assert int(codes[0]) == 0
    # (-1 + 4) / 4 = (-2 + 8) / 8 = (-0.25 + 1) / 1 = 0.75;  0.75 * 1023 = 767.25 -> 767
    assert int(codes[1]) == _interleave(767, 767, 767)


def test_morton_stage_flat_axis_gives_zero_bits():
    """All points in the plane z = 0 (through the origin): ext_z = 0, so no z bit is ever set; x and y as usual."""
    pts = np.array([[1.0, 1.0, 0.0], [-1.0, 4.0, 0.0], [0.0, 0.0, 0.0]], np.float32)
    bounds, codes = so.morton_stage(pts)
    np.testing.assert_array_equal(bounds, np.array([-1, 0, 0, 1, 4, 0], np.float32))
    # x: (1 + 1) / 2 * 1023 = 1023, (-1 + 1) / 2 = 0, (0 + 1) / 2 * 1023 = 511.5 -> 511;   y: 1 / 4 * 1023 = 255.75 -> 255, 1023, 0
    assert [int(c) for c in codes] == [_interleave(1023, 255, 0), _interleave(0, 1023, 0), _interleave(511, 0, 0)]
    assert not (codes & np.uint32(0x24924924)).any()       # the z bits


def test_morton_stage_extra_points_widen_the_bounds_only():
    pts = np.array([[1.0, 1.0, 1.0], [2.0, 2.0, 2.0]], np.float32)
    extra = np.array([[4.0, -2.0, 1.5]], np.float32)
    bounds, codes = so.morton_stage(pts, extra)
    np.testing.assert_array_equal(bounds, np.array([0, -2, 0, 4, 2, 2], np.float32))
    assert codes.shape == (2,)
    # x: 1 / 4 * 1023 = 255.75, 2 / 4 * 1023 = 511.5;  y: 3 / 4 * 1023 = 767.25, 4 / 4 -> 1023;  z: 1 / 2 -> 511.5, 1023
    assert [int(c) for c in codes] == [_interleave(255, 767, 511), _interleave(511, 1023, 1023)]
    b2, c2 = so.morton_stage(extra, pts)
    np.testing.assert_array_equal(b2, bounds)
    assert int(c2[0]) == _interleave(1023, 0, 767)


def test_morton_stage_single_point_and_empty():
    bounds, codes = so.morton_stage(np.array([[3.0, 0.0, -2.0]], np.float32))
    np.testing.assert_array_equal(bounds, np.array([0, 0, -2, 3, 0, 0], np.float32))
    assert int(codes[0]) == _interleave(1023, 0, 0)
    bounds, codes = so.morton_stage(np.zeros((0, 3), np.float32))
    assert codes.size == 0 and not bounds.any()


def test_box_bounds_ragged_last_box():
    pts = np.array([[0, 0, 0], [1, 5, -1], [2, 4, -2], [3, 3, -3], [9, -9, 9]], np.float32)
    order = np.array([4, 0, 3, 1, 2], np.uint32)
    got = so.box_bounds(pts, order, 2)
    want = np.array([[0, -9, 0, 9, 0, 9], [1, 3, -3, 3, 5, -1], [2, 4, -2, 2, 4, -2]], np.float32)
    np.testing.assert_array_equal(got, want)
    assert so.box_bounds(pts, order, 1024).shape == (1, 6)
