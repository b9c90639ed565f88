"""CPU oracle (plain numpy) of the stages in front of the two k-NN searches: the radix sort (csrc/radix_sort.hip) and the bounds,
Morton codes and box bounds of csrc/knn.hip.  tests/test_sort_oracle.py pins it on small hand-computed inputs;
tests/test_gpu_radix_sort.py and tests/test_gpu_knn_stages.py hold the kernels to it, bit for bit.

* stable_sort_pairs: a stable sort has exactly one right answer, so a comparison is array equality on keys AND values.
* morton_stage:      knn_bounds_kernel + knn_morton_kernel in float32, the same operations in the same order (knn.hip is built with FP
                     contraction off and HIP's fp32 division is correctly rounded, as numpy's is).
* box_bounds:        knn_box_bounds_kernel: min / max of the points at positions [b * box, (b + 1) * box) of the sorted order.
"""
import numpy as np

RADIX_BITS = 8           # csrc/fdgs_common.h
MORTON_BITS = 10         # per axis: (1 << 10) - 1 = 1023 cells
KNN_BOX, KNNQ_BOX = 1024, 256   # csrc/knn.hip: sources per box of fdgs_dist2_knn3 / fdgs_knn_query


def digits(keys, bit_lo, bit_hi):
    """The selected bits [bit_lo, bit_hi) of every key, as uint64 (so that a width of 32 needs no special case)."""
    k = np.asarray(keys, dtype=np.uint32).astype(np.uint64)
    return (k >> np.uint64(bit_lo)) & np.uint64((1 << (bit_hi - bit_lo)) - 1)


def stable_sort_pairs(keys, vals, bit_lo=0, bit_hi=32):
    """(keys, vals) in the one order a stable sort by the key bits [bit_lo, bit_hi) leaves them in."""
    keys, vals = np.asarray(keys, dtype=np.uint32), np.asarray(vals, dtype=np.uint32)
    assert 0 <= bit_lo <= bit_hi <= 32 and keys.shape == vals.shape and keys.ndim == 1
    perm = np.argsort(digits(keys, bit_lo, bit_hi), kind="stable")
    return keys[perm], vals[perm]


def prep_morton(x):
    """knn.hip prep_morton: spreads the low 10 bits of x to every third bit."""
    x = np.asarray(x, dtype=np.uint32)
    x = (x | (x << np.uint32(16))) & np.uint32(0x030000FF)
    x = (x | (x << np.uint32(8))) & np.uint32(0x0300F00F)
    x = (x | (x << np.uint32(4))) & np.uint32(0x030C30C3)
    x = (x | (x << np.uint32(2))) & np.uint32(0x09249249)
    return x


def morton_stage(points, extra=None):
    """(bounds float32 [6] = min xyz, max xyz over ``points``, ``extra`` and the ORIGIN; codes uint32 [P] of ``points``).
    cell = uint32(((p - min) / ext) * 1023) per axis, all float32, truncated; an axis with ext == 0 gives 0;
    code = spread(cx) | spread(cy) << 1 | spread(cz) << 2."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    both = [p, np.zeros((1, 3), np.float32)]
    if extra is not None:
        both.append(np.ascontiguousarray(extra, dtype=np.float32).reshape(-1, 3))
    both = np.concatenate(both, axis=0)
    mn, mx = both.min(axis=0), both.max(axis=0)
    ext = mx - mn                                            # float32
    codes = np.zeros(p.shape[0], np.uint32)
    for k in range(3):
        if ext[k] > 0:
            cell = (((p[:, k] - mn[k]) / ext[k]) * np.float32((1 << MORTON_BITS) - 1)).astype(np.uint32)
            codes |= prep_morton(cell) << np.uint32(k)
    return np.concatenate([mn, mx]).astype(np.float32), codes


def box_bounds(points, order, box):
    """float32 [ceil(P / box), 6]: min xyz, max xyz of points[order[b * box : (b + 1) * box]]; the last box may be ragged."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    order = np.asarray(order).astype(np.int64)
    nboxes = (order.size + box - 1) // box
    out = np.empty((nboxes, 6), np.float32)
    for b in range(nboxes):
        q = p[order[b * box:(b + 1) * box]]
        out[b, :3], out[b, 3:] = q.min(axis=0), q.max(axis=0)
    return out
