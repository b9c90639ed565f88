"""Plain numpy statement of the tile binning (csrc/tilebin.hip): what the count, scan, scatter and per-tile sort passes must leave behind.

Input: rect [P, 4] uint16 (x0, y0, x1, y1: the tiles [x0, x1) x [y0, y1) of a grid ``grid_x`` tiles wide), bits [P] uint32 (the bits of the
depths), grid_x, T.  An instance is a (Gaussian, covered tile) pair; tile = y * grid_x + x; its sort key is (bits, Gaussian index), a total
order since the indices are unique.  Pinned by tests/test_tilebin_oracle_host.py against a per-instance loop.
"""
import numpy as np


def instances(rect, grid_x):
    """(tile, gid) of every instance, Gaussian by Gaussian, rows of a rectangle top to bottom (int64)."""
    r = np.asarray(rect).astype(np.int64).reshape(-1, 4)
    w, h = r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]
    assert (w >= 0).all() and (h >= 0).all(), "x0 > x1 or y0 > y1"
    cnt = w * h
    gid = np.repeat(np.arange(r.shape[0], dtype=np.int64), cnt)
    k = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    wg = w[gid]
    tile = (r[gid, 1] + k // np.maximum(wg, 1)) * grid_x + r[gid, 0] + k % np.maximum(wg, 1)
    return tile, gid


def bin_compact(rect, bits, grid_x, T):
    """dict: counts [T], starts [T] (exclusive scan), R, longest, tile / key / gid [R] of the instances in (tile, bits, gid) order
    (point_list = gid), ranges [T, 2] with (0, 0) for empty tiles."""
    bits = np.asarray(bits).astype(np.uint32)
    tile, gid = instances(rect, grid_x)
    assert tile.size == 0 or (tile.min() >= 0 and tile.max() < T), "a rectangle leaves the grid"
    counts = np.bincount(tile, minlength=T).astype(np.int64)
    starts = np.cumsum(counts) - counts
    key = bits[gid].astype(np.int64)
    o = np.lexsort((gid, key, tile))
    ranges = np.stack([starts, starts + counts], axis=1)
    ranges[counts == 0] = 0
    return dict(counts=counts.astype(np.uint32), starts=starts.astype(np.uint32), R=int(counts.sum()), longest=int(counts.max()) if T else 0,
                tile=tile[o], key=key[o].astype(np.uint32), gid=gid[o].astype(np.uint32), point_list=gid[o].astype(np.uint32),
                ranges=ranges.astype(np.uint32))


def bin_sparse(rect, bits, grid_x, T, cap):
    """The sparse layout: tile t owns the slots [t * cap, (t + 1) * cap).  dict: counts [T] (true counts), R, longest, over [T] bool (count >
    cap), stored [T] = min(count, cap), ranges [T, 2] = (t * cap, t * cap + stored) or (0, 0), point_list [T * cap] with -1 (as int64) in
    the slots nobody owns and in every slot of an over-full tile (which of its instances arrive first is not determined), and the compact
    oracle under 'compact' (the per-tile sets: slice [starts[t], starts[t] + counts[t]) of its key / gid)."""
    c = bin_compact(rect, bits, grid_x, T)
    counts = c["counts"].astype(np.int64)
    stored = np.minimum(counts, cap)
    base = np.arange(T, dtype=np.int64) * cap
    ranges = np.stack([base, base + stored], axis=1)
    ranges[counts == 0] = 0
    pl = np.full(T * cap, -1, np.int64)
    over = counts > cap
    for t in np.nonzero(~over & (counts > 0))[0]:
        s = int(c["starts"][t])
        pl[base[t]:base[t] + counts[t]] = c["gid"][s:s + counts[t]]
    return dict(counts=c["counts"], R=c["R"], longest=c["longest"], over=over, stored=stored, ranges=ranges.astype(np.uint32), point_list=pl,
                compact=c)


def order_breaks_class_rule(order, counts, gmax):
    """The rule of tile_order_block, free of how its float division rounds: of two tiles whose counts differ by more than (gmax + 1) / 64 + 1
    the longer comes first.  Returns the largest count[later] - count[earlier] over all pairs minus that threshold (<= 0: the rule holds)."""
    c = np.asarray(counts).astype(np.int64)[np.asarray(order).astype(np.int64)]
    if c.size < 2:
        return -1.0
    worst = (c[1:] - np.minimum.accumulate(c)[:-1]).max()
    return float(worst) - ((float(gmax) + 1.0) / 64.0 + 1.0)
