"""GPU: the stages in front of the two k-NN searches (csrc/knn.hip: bounds, Morton codes, the sort inside its real caller, box bounds)
read out of the scratch buffer of a finished fdgs_dist2_knn3 / fdgs_knn_query (fdgs_debug_knn_stage_offsets) and held, bit for bit, to
tests/sort_oracle.py.  The searches are exact whatever order the points are in -- test_gpu_knn.py and test_gpu_regularizers.py would
pass with any permutation -- so a wrong code, an unstable sort or a box that is too large costs time only, and only these tests see it.
The final distances / indices of the SAME runs are still compared with the brute-force oracles."""
import ctypes as C

import numpy as np
import pytest
import torch

import util  # noqa: F401
import regularizer_oracle as ro
import sort_oracle as so
from oracle import knn_oracle

pytestmark = pytest.mark.gpu

FLT_MAX = np.float32(3.4028234663852886e38)


def _pts(P, seed, kind):
    rng = np.random.default_rng(seed)
    if kind == "gauss":
        return (rng.standard_normal((P, 3)) * np.array([3.0, 1.0, 0.2])).astype(np.float32)
    if kind == "shifted":   # far from the origin
        return (rng.random((P, 3)) + np.array([50.0, -20.0, 7.0])).astype(np.float32)
    if kind == "dups":
        base = rng.standard_normal((max(P // 3, 1), 3)).astype(np.float32)
        return base[rng.integers(0, base.shape[0], P)]
    if kind == "plane":     # z = +0 for every point: a zero-extent axis through the origin
        p = (rng.standard_normal((P, 3)) * 2.0).astype(np.float32)
        p[:, 2] = 0.0
        return p
    if kind == "octant":    # one octant, away from the origin: the origin sets the minimum on every axis
        return (rng.random((P, 3)) * np.array([1.0, 2.0, 0.5]) + 3.0).astype(np.float32)
    if kind == "corner":    # in [0, 4) x [0, 2) x [0, 1) plus one point exactly on the max corner: 1023 on every axis
        p = (rng.random((P, 3)) * np.array([4.0, 2.0, 1.0])).astype(np.float32)
        p = np.minimum(p, np.nextafter(np.array([4.0, 2.0, 1.0], np.float32), np.float32(0)))
        p[P // 2] = [4.0, 2.0, 1.0]
        return p
    raise ValueError(kind)


def _read(scratch, off, count, dtype):
    nbytes = count * np.dtype(dtype).itemsize
    return scratch[off:off + nbytes].cpu().numpy().view(dtype)


def _offsets(query, n, m):
    from fdgs import _capi
    off = (C.c_int64 * _capi.KNN_NUM_STAGES)()
    assert _capi.lib.fdgs_debug_knn_stage_offsets(query, n, m, off) == 0, _capi.last_error()
    return [int(x) for x in off]


def _check_side(scratch, off_codes, off_order, pts, codes, label):
    """Sorted codes and order of one point set against the oracle's codes put through the stable sort.  Returns the order."""
    n = pts.shape[0]
    want_codes, want_order = so.stable_sort_pairs(codes, np.arange(n, dtype=np.uint32))
    got_codes, got_order = _read(scratch, off_codes, n, np.uint32), _read(scratch, off_order, n, np.uint32)
    np.testing.assert_array_equal(np.sort(got_order), np.arange(n, dtype=np.uint32), err_msg=label + ": the order is not a permutation")
    np.testing.assert_array_equal(got_codes, want_codes, err_msg=label + ": sorted Morton codes")
    np.testing.assert_array_equal(got_order, want_order, err_msg=label + ": sorted order (stable)")
    return got_order


def _check_boxes(scratch, off, pts, order, box, label):
    nboxes = (pts.shape[0] + box - 1) // box
    assert off[6] == nboxes and off[7] == box
    got = _read(scratch, off[1], nboxes * 6, np.float32).reshape(nboxes, 6)
    want = so.box_bounds(pts, order, box)
    assert (np.abs(got) < FLT_MAX).all(), label + ": +-FLT_MAX of an unused slot leaked into a box"
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=label + ": box bounds")


def _dist2_rows(p, rows):
    """oracle/knn_oracle.dist2_knn3's arithmetic for the rows ``rows`` only (P >= 4)."""
    q = p[rows]
    dx, dy, dz = (p[None, :, k] - q[:, None, k] for k in range(3))
    d = (dx * dx + dy * dy) + dz * dz
    d[np.arange(len(rows)), rows] = np.inf
    best = np.sort(np.partition(d, 2, axis=1)[:, :3], axis=1).astype(np.float32)
    return ((best[:, 0] + best[:, 1]) + best[:, 2]) / np.float32(3.0)


DIST2_CASES = [(1, "gauss"), (3, "gauss"), (255, "gauss"), (1024, "gauss"), (1025, "gauss"), (4097, "gauss"), (20000, "gauss"),
               (1, "shifted"), (1025, "shifted"), (4097, "shifted"),
               (255, "dups"), (4097, "dups"),
               (1, "plane"), (3, "plane"), (1025, "plane"), (4097, "plane"),
               (1, "octant"), (3, "octant"), (1024, "octant"), (1025, "octant"),
               (255, "corner"), (1024, "corner"), (1025, "corner"), (4097, "corner")]


@pytest.mark.parametrize("P,kind", DIST2_CASES)
def test_dist2_stages_bit_exact(P, kind, gpu_device):
    from fdgs import _capi
    pts = _pts(P, 31 * P + len(kind), kind)
    t = torch.from_numpy(pts).to(gpu_device)
    means = torch.zeros(P, dtype=torch.float32, device=gpu_device)
    scratch = torch.empty(_capi.lib.fdgs_knn_scratch_bytes(P), dtype=torch.uint8, device=gpu_device)
    scratch.fill_(0xA5)
    with torch.cuda.device(gpu_device):
        rc = _capi.lib.fdgs_dist2_knn3(P, t.data_ptr(), means.data_ptr(), scratch.data_ptr(), _capi.current_stream_handle(gpu_device))
    assert rc == 0, _capi.last_error()
    torch.cuda.synchronize(gpu_device)
    off = _offsets(0, 0, P)
    assert off[4] == -1 and off[5] == -1 and all(0 <= o < scratch.numel() for o in off[:4])

    bounds, codes = so.morton_stage(pts)
    assert codes.max() < (1 << 30)
    if kind == "corner":
        assert codes[P // 2] == 0x3FFFFFFF
    if kind == "plane":
        assert not (codes & np.uint32(0x24924924)).any()
    label = "%s P=%d" % (kind, P)
    np.testing.assert_array_equal(_read(scratch, off[0], 6, np.float32).view(np.uint32), bounds.view(np.uint32), err_msg=label + ": bounds")
    order = _check_side(scratch, off[2], off[3], pts, codes, label)
    _check_boxes(scratch, off, pts, order, so.KNN_BOX, label)

    got = means.cpu().numpy()
    if P <= 5000:
        want = knn_oracle.dist2_knn3(pts)
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    else:
        rows = np.random.default_rng(P).choice(P, 600, replace=False)
        np.testing.assert_array_equal(got[rows].view(np.uint32), _dist2_rows(pts, rows).view(np.uint32))


def _query_pair(n, m, kind, seed):
    """Sources of ``kind``; queries of the same kind spread 2 x wider about another centre, so that a good part of them lies outside
    the sources' extent on every axis that has one."""
    src = _pts(m, seed, kind)
    x = _pts(n, seed + 1, kind) * np.float32(2.0) + np.array([0.5, -0.25, 0.0], np.float32)
    if kind == "dups" and n >= 4:
        x[: n // 2] = src[np.arange(n // 2) % m]            # queries sitting on (duplicated) sources
    return x.astype(np.float32), src


QUERY_CASES = [(100, 255, "gauss"), (300, 256, "gauss"), (64, 257, "gauss"), (257, 256, "dups"), (5000, 300, "gauss"), (777, 4097, "gauss"),
               (1300, 1025, "shifted"), (500, 2000, "plane"), (5, 3, "gauss"), (3, 1, "octant"), (1, 600, "dups"), (2500, 20000, "gauss")]


@pytest.mark.parametrize("n,m,kind", QUERY_CASES)
def test_knn_query_stages_bit_exact(n, m, kind, gpu_device):
    """b = 1, n != m, k = 8: one set of bounds over sources AND queries, both Morton-sorted sets, boxes of 256 sources; n > m: the shared
    histogram area is sized by the queries."""
    from fdgs import _capi
    k = 8
    x, src = _query_pair(n, m, kind, 17 * n + m)
    tx, ts = torch.from_numpy(x).to(gpu_device), torch.from_numpy(src).to(gpu_device)
    idx = torch.empty((n, k), dtype=torch.int64, device=gpu_device)
    d2 = torch.empty((n, k), dtype=torch.float32, device=gpu_device)
    scratch = torch.empty(_capi.lib.fdgs_knn_query_scratch_bytes(n, m), dtype=torch.uint8, device=gpu_device)
    scratch.fill_(0xA5)
    with torch.cuda.device(gpu_device):
        rc = _capi.lib.fdgs_knn_query(1, n, m, k, tx.data_ptr(), ts.data_ptr(), idx.data_ptr(), d2.data_ptr(), scratch.data_ptr(),
                                      _capi.current_stream_handle(gpu_device))
    assert rc == 0, _capi.last_error()
    torch.cuda.synchronize(gpu_device)
    off = _offsets(1, n, m)
    assert all(0 <= o < scratch.numel() for o in off[:6])

    bounds, scodes = so.morton_stage(src, extra=x)
    bounds_q, qcodes = so.morton_stage(x, extra=src)
    np.testing.assert_array_equal(bounds, bounds_q)
    if min(n, m) >= 64 and kind != "shifted":   # the point of the placement: queries beyond the sources' own extent
        own = so.morton_stage(src)[0]
        assert ((x[:, :2] < own[:2]) | (x[:, :2] > own[3:5])).any(axis=1).sum() >= n // 20
    assert max(scodes.max(), qcodes.max()) < (1 << 30)
    label = "%s n=%d m=%d" % (kind, n, m)
    np.testing.assert_array_equal(_read(scratch, off[0], 6, np.float32).view(np.uint32), bounds.view(np.uint32), err_msg=label + ": bounds")
    sorder = _check_side(scratch, off[2], off[3], src, scodes, label + " sources")
    _check_side(scratch, off[4], off[5], x, qcodes, label + " queries")
    _check_boxes(scratch, off, src, sorder, so.KNNQ_BOX, label)

    rows = np.arange(n) if m <= 5000 else np.random.default_rng(n).choice(n, 600, replace=False)
    wi, wd = ro.knn(x, src, k, rows=rows)
    np.testing.assert_array_equal(d2.cpu().numpy()[rows].view(np.uint32), wd.view(np.uint32))
    np.testing.assert_array_equal(idx.cpu().numpy()[rows], wi)


def test_stage_offsets_argument_errors():
    from fdgs import _capi
    off = (C.c_int64 * _capi.KNN_NUM_STAGES)()
    assert _capi.lib.fdgs_debug_knn_stage_offsets(0, 0, -1, off) == 1
    assert _capi.lib.fdgs_debug_knn_stage_offsets(1, -1, 5, off) == 1
    assert _capi.lib.fdgs_debug_knn_stage_offsets(1, 5, 5, None) == 1
    assert "fdgs_debug_knn_stage_offsets" in _capi.last_error()
