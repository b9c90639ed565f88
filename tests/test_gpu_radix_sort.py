"""GPU: the radix sort (csrc/radix_sort.hip) through fdgs_debug_radix_sort_pairs against tests/sort_oracle.stable_sort_pairs.

A stable sort has exactly one right answer, so every comparison is array equality on the keys AND on the values.  Values are arange(n)
unless said otherwise, so the values that come back ARE the permutation.  Sizes (each the smallest that reaches the path named):
  1, 63 .. 257        wave and workgroup edges             1023 .. 1025   one 1024-key chunk, a ragged second one
  4097                several chunks                        262144 / 262145   256 / 257 chunks: radix_scan_kernel's loop once / twice
  2^20                last size of the 4-keys-per-thread instance (1024 workgroups)
  2^20 + 1            first size of the 16-keys-per-thread instance (257 chunks of 4096, the last with one key)
  2^20 + 3 * 4096     that instance with whole chunks only
"""
import numpy as np
import pytest
import torch

import sort_oracle as so

pytestmark = pytest.mark.gpu

M = 1 << 20
EDGES = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097]
SCAN = [262144, 262145]
BIG = [M, M + 1, M + 3 * 4096]
ALL_SIZES = EDGES + SCAN + BIG
FEW = [257, 1025, 4097, 262145, M + 1]         # ragged sizes of every path


def _u32(a):
    return np.ascontiguousarray(a).astype(np.uint32)


def _keys(kind, n, seed=0):
    rng = np.random.default_rng([n, seed])
    if kind == "uniform":          # every digit of every pass occupied (from a few thousand keys on)
        return _u32(rng.integers(0, 1 << 32, n, dtype=np.uint64))
    if kind == "zeros":
        return np.zeros(n, np.uint32)
    if kind == "ones":             # real keys equal to the pad value of a ragged last chunk
        return np.full(n, 0xFFFFFFFF, np.uint32)
    if kind.startswith("alt"):     # two alternating keys that differ in byte alt<b> only: one digit run spans waves, chunks, workgroups
        b = int(kind[3])
        k = np.full(n, 0x5A3C96E1, np.uint32)
        k[::2] ^= np.uint32(0x81 << (8 * b))
        return k
    if kind == "sorted":
        return np.sort(_keys("uniform", n, seed))
    if kind == "reverse":
        return np.sort(_keys("uniform", n, seed))[::-1].copy()
    if kind == "morton":           # 30-bit keys with heavy duplication, the k-NN's own shape
        pool = rng.integers(0, 1 << 30, max(n // 8, 1), dtype=np.uint64)
        return _u32(pool[rng.integers(0, pool.size, n)])
    if kind == "low24":            # keys whose low 24 bits are equal: three passes that must leave the order alone
        return _u32((rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(24)) | np.uint64(0x00C0FFEE))
    raise ValueError(kind)


class _Sorter:
    """fdgs_debug_radix_sort_pairs on numpy arrays, with a scratch tensor that outlives the calls."""

    def __init__(self, dev, max_bytes=0):
        from fdgs import _capi
        self.capi, self.dev = _capi, dev
        self.scratch = torch.empty(max(max_bytes, 256), dtype=torch.uint8, device=dev)

    def bytes_for(self, n):
        return int(self.capi.lib.fdgs_debug_radix_sort_scratch_bytes(n))

    def call(self, keys, vals, lo, hi):
        n = int(keys.size)
        if self.scratch.numel() < self.bytes_for(n):
            self.scratch = torch.empty(self.bytes_for(n), dtype=torch.uint8, device=self.dev)
        k = torch.from_numpy(keys.view(np.int32).copy()).to(self.dev)
        v = torch.from_numpy(vals.view(np.int32).copy()).to(self.dev)
        with torch.cuda.device(self.dev):
            rc = self.capi.lib.fdgs_debug_radix_sort_pairs(n, lo, hi, k.data_ptr() if n else None, v.data_ptr() if n else None,
                                                           self.scratch.data_ptr(), self.capi.current_stream_handle(self.dev))
        torch.cuda.synchronize(self.dev)
        return rc, k.cpu().numpy().view(np.uint32), v.cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def sorter(gpu_device):
    return _Sorter(gpu_device)


def _check(sorter, keys, vals=None, lo=0, hi=32):
    n = keys.size
    vals = np.arange(n, dtype=np.uint32) if vals is None else vals
    rc, gk, gv = sorter.call(keys, vals, lo, hi)
    assert rc == 0, sorter.capi.last_error()
    wk, wv = so.stable_sort_pairs(keys, vals, lo, hi)
    np.testing.assert_array_equal(gv, wv, err_msg="values (with arange: the permutation), n = %d, bits [%d, %d)" % (n, lo, hi))
    np.testing.assert_array_equal(gk, wk, err_msg="keys, n = %d, bits [%d, %d)" % (n, lo, hi))
    return gk, gv


@pytest.mark.parametrize("n", ALL_SIZES)
def test_uniform_keys_every_size(n, sorter):
    _check(sorter, _keys("uniform", n))


@pytest.mark.parametrize("n", FEW)
def test_all_keys_zero_is_the_identity(n, sorter):
    _, gv = _check(sorter, _keys("zeros", n))
    np.testing.assert_array_equal(gv, np.arange(n, dtype=np.uint32))


@pytest.mark.parametrize("n", [1, 65] + FEW + [M + 4095])
def test_all_keys_equal_to_the_pad_value_survive(n, sorter):
    """Ragged sizes: the last chunk is padded with 0xFFFFFFFF keys inside the kernel.  Real keys of that value must all come out, in input
    order, and nothing else: a pad that took part in a rank or a count would push a real pair out of its place."""
    gk, gv = _check(sorter, _keys("ones", n))
    np.testing.assert_array_equal(gv, np.arange(n, dtype=np.uint32))
    assert (gk == 0xFFFFFFFF).all()
    mixed = _keys("uniform", n, 1)
    mixed[n // 2:] = 0xFFFFFFFF               # half real pad-valued keys behind uniform ones
    _check(sorter, mixed)


@pytest.mark.parametrize("n,byte", [(257, 0), (4097, 0), (4097, 1), (4097, 2), (4097, 3), (262145, 1), (M, 2), (M + 1, 0), (M + 1, 3)])
def test_two_alternating_keys_differing_in_one_byte(n, byte, sorter):
    """Three passes see one digit only, one pass sees two: a single digit run spans every wave, chunk and workgroup, and any rank error
    breaks stability.  The result is all even positions, in order, then all odd ones (or the other way round)."""
    keys = _keys("alt%d" % byte, n)
    _, gv = _check(sorter, keys)
    first = 0 if keys[0] < keys[1 % n] or n == 1 else 1
    want = np.concatenate([np.arange(first, n, 2), np.arange(1 - first, n, 2)]).astype(np.uint32)
    np.testing.assert_array_equal(gv, want)


@pytest.mark.parametrize("kind", ["sorted", "reverse"])
@pytest.mark.parametrize("n", [1025, 4097, M + 1])
def test_sorted_and_reverse_sorted_input(n, kind, sorter):
    _check(sorter, _keys(kind, n))


@pytest.mark.parametrize("n", [255, 4097, 262145, M + 1])
def test_30_bit_keys_with_heavy_duplication(n, sorter):
    keys = _keys("morton", n)
    assert keys.max() < (1 << 30)
    _check(sorter, keys)


@pytest.mark.parametrize("n", [1025, 4097, M + 1])
def test_keys_with_equal_low_24_bits(n, sorter):
    _check(sorter, _keys("low24", n))


@pytest.mark.parametrize("n", [4097, M + 1])
def test_arbitrary_values_are_carried_not_recomputed(n, sorter):
    vals = _u32(np.random.default_rng(n + 7).integers(0, 1 << 32, n, dtype=np.uint64))
    vals[:3] = [0xFFFFFFFF, 0, 0x80000000]
    _check(sorter, _keys("morton", n), vals)
    _check(sorter, _keys("uniform", n), vals)


@pytest.mark.parametrize("lo,hi", [(0, 8), (8, 32), (8, 24), (24, 32), (16, 16)])
@pytest.mark.parametrize("n", [257, 4097, 262145, M + 1])
def test_bit_ranges(n, lo, hi, sorter):
    """(0, 8), (8, 32), (24, 32): an odd number of passes, the result lands in the second buffer.  (8, 24): ties on the selected bits keep
    their input order although the full keys differ.  (16, 16): no pass, the arrays are untouched."""
    keys = _keys("uniform", n)
    if hi - lo == 16:
        keys[n // 3:] = (keys[n // 3:] & np.uint32(0xFF0000FF)) | np.uint32(0x00123400)    # many ties on bits [8, 24) with different keys
    gk, gv = _check(sorter, keys, lo=lo, hi=hi)
    if lo == hi:
        np.testing.assert_array_equal(gk, keys)
        np.testing.assert_array_equal(gv, np.arange(n, dtype=np.uint32))


def test_empty_input_is_a_no_op(sorter):
    rc, gk, gv = sorter.call(np.zeros(0, np.uint32), np.zeros(0, np.uint32), 0, 32)
    assert rc == 0 and gk.size == 0 and gv.size == 0


@pytest.mark.parametrize("n,between", [(262145, 4097), (M + 1, 1025), (4097, M + 1)])
def test_same_input_twice_with_another_sort_in_between(n, between, gpu_device):
    """One scratch buffer, three sorts: the first and the third are the same input and must give the same, right, answer -- a histogram,
    digit total or count left over from the sort in between (another size: another number of chunks, another instance) would show."""
    s = _Sorter(gpu_device)
    s.scratch = torch.empty(max(s.bytes_for(n), s.bytes_for(between)), dtype=torch.uint8, device=gpu_device)
    ptr = s.scratch.data_ptr()
    keys = _keys("morton", n, 3)
    k1, v1 = _check(s, keys)
    _check(s, _keys("uniform", between, 5))
    k2, v2 = _check(s, keys)
    assert s.scratch.data_ptr() == ptr
    np.testing.assert_array_equal(k1, k2)
    np.testing.assert_array_equal(v1, v2)


@pytest.mark.parametrize("lo,hi", [(-1, 7), (-8, 0), (0, 33), (8, 40), (16, 8), (32, 0), (0, 12), (0, 31), (4, 8), (3, 32)])
def test_refused_bit_ranges_return_the_error_and_launch_nothing(lo, hi, sorter):
    keys = _keys("uniform", 1025)
    vals = np.arange(1025, dtype=np.uint32)
    rc, gk, gv = sorter.call(keys, vals, lo, hi)
    assert rc == 1
    assert "fdgs_debug_radix_sort_pairs" in sorter.capi.last_error() and "[%d, %d)" % (lo, hi) in sorter.capi.last_error()
    np.testing.assert_array_equal(gk, keys)
    np.testing.assert_array_equal(gv, vals)


def test_other_argument_errors(sorter, gpu_device):
    lib = sorter.capi.lib
    assert lib.fdgs_debug_radix_sort_pairs(-1, 0, 32, None, None, None, None) == 1
    assert lib.fdgs_debug_radix_sort_pairs(5, 0, 32, None, None, sorter.scratch.data_ptr(), None) == 1
    assert "NULL" in sorter.capi.last_error()
    assert lib.fdgs_debug_radix_sort_pairs(0, 0, 32, None, None, None, None) == 0
    b = [lib.fdgs_debug_radix_sort_scratch_bytes(n) for n in (0, 1, 1024, 1025, M, M + 1)]
    assert all(x % 256 == 0 and x >= 16 * max(n, 1) + 257 * 4 for x, n in zip(b, (0, 1, 1024, 1025, M, M + 1)))
