"""Inputs for the tile binning stage tests (tests/test_gpu_tilebin_stages.py): rectangles by shape, lists by planting.

A case is a dict: name, rect [P, 4] uint16, depths [P] float32, grid_x, T, plus what was planted ('hot': the tile, 'n': its list length,
...), so that tests/test_tilebin_oracle_host.py can assert the property on the host.  To give tile t exactly n entries, n Gaussians carry
the 1x1 rectangle of t and nobody else touches t.  Depths are finite floats >= 0.2 only (the near plane of preprocess_fwd).
"""
import numpy as np

NEAR = np.float32(0.2)
LIST_LENGTHS = [1, 2, 63, 64, 65, 96, 97, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385]
DEPTH_KINDS = ["uniform", "all_equal", "two_values", "sliver_plus_outliers", "low_bits_only", "descending_in_id", "ascending_in_id"]
P_EDGES = [1, 63, 64, 65, 1023, 1024, 1025, 4097]
T_EDGES = [1, 2, 3, 5, 1023, 1025, 4095, 4096, 4097, 8192, 8193, 36864, 36865]
RECT_GRID = (40, 30)
RECT_SHAPES = {"1x1": (1, 1), "6x8": (6, 8), "7x7": (7, 7), "1x30": (1, 30), "40x1": (40, 1), "40x30": (40, 30),
               "empty_w": (0, 3), "empty_h": (3, 0)}
SPARSE_GRID = (12, 10)
SPARSE_CAPS = [64, 256]


def _seed(name):
    return int(np.frombuffer(name.encode(), np.uint8).astype(np.int64).sum()) * 7919 + len(name)


def depths_of(kind, n, rng):
    """n float32 depths >= 0.2 in ID ORDER of the list's Gaussians."""
    if kind == "uniform":
        d = rng.uniform(0.2, 100.0, n)
    elif kind == "all_equal":
        d = np.full(n, 1.5)
    elif kind == "two_values":
        d = rng.choice([0.75, 3.25], n)
    elif kind == "sliver_plus_outliers":   # 99 % within 1e-4 relative, 1 % over four decades
        d = 2.0 * (1.0 + 1e-4 * rng.random(n))
        out = rng.random(n) < 0.01
        d[out] = 10.0 ** rng.uniform(-0.5, 3.5, int(out.sum()))
    elif kind == "low_bits_only":          # consecutive bit patterns, shuffled
        b = np.float32(1.0).view(np.uint32) + rng.permutation(n).astype(np.uint32)
        return b.view(np.float32).copy()
    elif kind == "descending_in_id":
        d = np.sort(rng.uniform(0.2, 100.0, n))[::-1]
    elif kind == "ascending_in_id":
        d = np.sort(rng.uniform(0.2, 100.0, n))
    else:
        raise ValueError(kind)
    return np.maximum(d.astype(np.float32), NEAR)


def _unit(tile, grid_x):
    x, y = tile % grid_x, tile // grid_x
    return [x, y, x + 1, y + 1]


def planted(name, grid_x, T, lists, background=None, seed=0):
    """lists: {tile: depths in the id order of that tile's Gaussians}; background: (rect [B, 4], depths [B]) of further Gaussians, which must
    not touch a planted tile.  The Gaussians of all lists and the background are interleaved at random (ids are the positions)."""
    rects, deps, owner = [], [], []
    for t, d in lists.items():
        rects += [_unit(t, grid_x)] * len(d)
        deps.append(np.asarray(d, np.float32))
        owner += [t] * len(d)
    if background is not None:
        rects += [list(r) for r in np.asarray(background[0]).tolist()]
        deps.append(np.asarray(background[1], np.float32))
        owner += [-1] * len(background[1])
    rect = np.asarray(rects, np.uint16).reshape(-1, 4)
    dep = np.concatenate(deps) if deps else np.zeros(0, np.float32)
    owner = np.asarray(owner, np.int64)
    # a random interleaving that keeps every owner's Gaussians in their given order (so 'ascending_in_id' stays ascending in the id)
    rng = np.random.default_rng(_seed(name) + seed)
    perm = np.argsort(rng.random(rect.shape[0]), kind="stable")      # position -> source
    for t in set(owner.tolist()):
        pos = np.nonzero(owner[perm] == t)[0]
        perm[pos] = np.sort(perm[pos])
    return dict(name=name, rect=np.ascontiguousarray(rect[perm]), depths=np.ascontiguousarray(dep[perm]), grid_x=grid_x, T=T,
                planted={t: len(d) for t, d in lists.items()})


def list_case(n, kind, hot=5):
    """One tile among 8 (a 4 x 2 grid) holds n entries of the depth kind; the other seven hold short random lists."""
    name = "list_%d_%s" % (n, kind)
    rng = np.random.default_rng(_seed(name))
    lists = {hot: depths_of(kind, n, rng)}
    for t in range(8):
        if t != hot:
            lists[t] = depths_of("uniform", int(rng.integers(1, 40)), rng)
    c = planted(name, 4, 8, lists)
    c.update(hot=hot, n=n, kind=kind)
    return c


def crowded_case(n, pile, hot=2):
    """A list of n entries in which exactly `pile` share one depth; every other depth of the list is distinct and at least 1 % away
    from the pile's, so the pile's bucket holds the pile and (almost surely) nothing else."""
    name = "crowded_%d_%d" % (n, pile)
    rng = np.random.default_rng(_seed(name))
    v = np.float32(7.0)
    d = np.empty(0, np.float32)
    while d.size < n - pile:
        x = np.unique(rng.uniform(0.2, 1000.0, 2 * n).astype(np.float32))
        x = x[(np.abs(x - v) > 0.01 * v) & (x >= NEAR)]
        d = np.unique(np.concatenate([d, x]))
    d = rng.permutation(d)[:n - pile]
    dep = rng.permutation(np.concatenate([d, np.full(pile, v, np.float32)]))
    lists = {hot: dep}
    for t in range(8):
        if t != hot:
            lists[t] = depths_of("uniform", int(rng.integers(1, 40)), rng)
    c = planted(name, 4, 8, lists)
    c.update(hot=hot, n=n, pile=pile, pile_depth=v)
    return c


def equal_samples_case(n):
    """A list whose 64 sample positions all carry one depth while the rest of it does not.  The per-tile sort takes its splitters from
    the list positions lane * n / 64 in ARRIVAL order.  The hot tile's Gaussians are the ids 0 .. n - 1 (n a multiple of 1024), all 1x1: the
    64 lanes of a wave arrive in lane order, waves and workgroups as whole blocks of 64 and 1024 entries, so an entry's arrival position
    equals its id modulo 64.  Every id carries the depth v except those with id % 16 == 8, so every position that is a multiple of
    n / 64 (16 or more) holds v whatever order the blocks arrive in."""
    assert n % 1024 == 0
    name = "equal_samples_%d" % n
    rng = np.random.default_rng(_seed(name))
    v = np.float32(3.0)
    dep = np.full(n, v, np.float32)
    odd = np.arange(n) % 16 == 8
    dep[odd] = np.unique(rng.uniform(0.2, 50.0, 4 * n).astype(np.float32))[:int(odd.sum())][rng.permutation(int(odd.sum()))]
    dep = np.maximum(dep, NEAR)
    rect = [_unit(5, 4)] * n
    others = [t for t in range(8) if t != 5]
    extra = [_unit(others[i % 7], 4) for i in range(70)]
    c = dict(name=name, rect=np.asarray(rect + extra, np.uint16), depths=np.concatenate([dep, depths_of("uniform", 70, rng)]), grid_x=4, T=8,
             planted={5: n}, hot=5, n=n, sample_depth=v, step=n // 64)
    return c


def _place(shape, gx, gy, rng, touch=None):
    w, h = shape
    x0 = int(rng.integers(0, gx - max(w, 1) + 1))
    y0 = int(rng.integers(0, gy - max(h, 1) + 1))
    if touch == "right":
        x0 = gx - w
    if touch == "bottom":
        y0 = gy - h
    return [x0, y0, x0 + w, y0 + h]


def rect_single_case(shape_name, P=65, at=37):
    """P Gaussians on the 40 x 30 grid: one rectangle of the named shape, the others empty (alternately x0 == x1 and y0 == y1)."""
    gx, gy = RECT_GRID
    name = "rect_single_%s" % shape_name
    rng = np.random.default_rng(_seed(name))
    rect = np.zeros((P, 4), np.uint16)
    for g in range(P):
        rect[g] = _place(RECT_SHAPES["empty_w" if g % 2 else "empty_h"], gx, gy, rng)
    rect[at] = _place(RECT_SHAPES[shape_name], gx, gy, rng)
    return dict(name=name, rect=rect, depths=depths_of("uniform", P, rng), grid_x=gx, T=gx * gy, shape=RECT_SHAPES[shape_name], at=at)


def rect_mix_case(P=65, seed=0):
    """Every shape several times, some touching the last column / the last row, on the 40 x 30 grid."""
    gx, gy = RECT_GRID
    name = "rect_mix_%d_%d" % (P, seed)
    rng = np.random.default_rng(_seed(name))
    names = list(RECT_SHAPES)
    rect = np.zeros((P, 4), np.uint16)
    shapes = []
    for g in range(P):
        s = names[g % len(names)]
        rect[g] = _place(RECT_SHAPES[s], gx, gy, rng, touch=[None, "right", "bottom", None][(g // len(names)) % 4])
        shapes.append(s)
    return dict(name=name, rect=rect, depths=depths_of("two_values" if seed else "uniform", P, rng), grid_x=gx, T=gx * gy, shapes=shapes)


def big_grid_case():
    """300 x 300 tiles (more than an LDS histogram holds: the direct kernel): the whole grid, a 299 x 1 and a 1 x 299 rectangle."""
    rect = np.asarray([[0, 0, 300, 300], [1, 299, 300, 300], [299, 1, 300, 300]], np.uint16)
    return dict(name="big_grid", rect=rect, depths=np.asarray([2.0, 1.0, 3.0], np.float32), grid_x=300, T=90000)


# Widths whose quotient s / w by a correctly rounded float reciprocal comes out one short at s = w (tests/test_tilebin_oracle_host.py
# asserts it): rectangles that need the correction step of walk_rect_tiles' wide path.  No width up to 40 does, nor do 299 and 300.
WIDE_WIDTHS = [41, 47, 55, 61]
BIG_WIDE_WIDTHS = [41, 61, 97, 123, 245, 293]


def quotient_needs_correction(w, h):
    s = np.arange(w * h, dtype=np.int64)
    q = (s.astype(np.float32) * (np.float32(1.0) / np.float32(w))).astype(np.int64)
    return bool((q != s // w).any())


def wide_correction_case():
    """64 x 8 tiles (LDS histogram), 65 rectangles of the widths above, 2 to 8 rows, none starting in column 0 or as wide as the grid
    (a quotient one short would then land in the right tile all the same)."""
    gx, gy = 64, 8
    rng = np.random.default_rng(_seed("wide_correction"))
    rect = np.zeros((65, 4), np.uint16)
    for g in range(65):
        w, h = WIDE_WIDTHS[g % 4], 2 + g % 7
        x0, y0 = int(rng.integers(1, gx - w + 1)), int(rng.integers(0, gy - h + 1))
        rect[g] = [x0, y0, x0 + w, y0 + h]
    return dict(name="wide_correction", rect=rect, depths=depths_of("uniform", 65, rng), grid_x=gx, T=gx * gy)


def big_grid_widths_case():
    """300 x 300 tiles (direct kernel): three rows of each width above, ending in the last row, none starting in column 0."""
    rect = np.asarray([[300 - w - (i % 2), 297, 300 - (i % 2), 300] for i, w in enumerate(BIG_WIDE_WIDTHS)], np.uint16)
    rng = np.random.default_rng(_seed("big_grid_widths"))
    return dict(name="big_grid_widths", rect=rect, depths=depths_of("uniform", rect.shape[0], rng), grid_x=300, T=90000)


def grid_for(T):
    """grid_x: the divisor of T nearest to sqrt(T); T itself when T has none but 1 and T."""
    best = 1
    for d in range(1, int(T ** 0.5) + 1):
        if T % d == 0:
            best = d
    return T if best == 1 else T // best


def _small_rects(n, gx, gy, rng, most=3):
    rect = np.zeros((n, 4), np.uint16)
    for g in range(n):
        rect[g] = _place((int(rng.integers(1, min(most, gx) + 1)), int(rng.integers(1, min(most, gy) + 1))), gx, gy, rng)
    return rect


def p_edge_case(P):
    """P Gaussians with small rectangles (a few of them larger than 48 tiles) on a 16 x 16 grid."""
    name = "p_edge_%d" % P
    rng = np.random.default_rng(_seed(name))
    rect = _small_rects(P, 16, 16, rng)
    for g in range(0, P, 97):
        rect[g] = _place((8, 7), 16, 16, rng)
    rect[P - 1] = [15, 15, 16, 16]     # the last Gaussian is live, in the last tile
    return dict(name=name, rect=rect, depths=depths_of("uniform", P, rng), grid_x=16, T=256)


def t_edge_case(T, n_rects=300):
    """A few hundred small rectangles on T tiles; the last tile is non-empty and holds the longest list."""
    from tilebin_oracle import instances
    name = "t_edge_%d" % T
    rng = np.random.default_rng(_seed(name))
    gx = grid_for(T)
    gy = T // gx
    rect = _small_rects(n_rects, gx, gy, rng, most=2)
    tile, _ = instances(rect, gx)
    counts = np.bincount(tile, minlength=T)
    more = int(counts[:-1].max() if T > 1 else 0) + 3 - int(counts[-1])
    rect = np.concatenate([rect, np.asarray([_unit(T - 1, gx)] * max(more, 1), np.uint16)])
    rect = rect[rng.permutation(rect.shape[0])]
    return dict(name=name, rect=np.ascontiguousarray(rect), depths=depths_of("uniform", rect.shape[0], rng), grid_x=gx, T=T)


def order_case(kind):
    """The tile order's corner cases on a 9 x 7 grid: no instance at all, one hot tile, every tile the same count."""
    gx, gy = 9, 7
    T = gx * gy
    rng = np.random.default_rng(_seed("order_" + kind))
    if kind == "all_empty":
        rect = np.asarray([_place(RECT_SHAPES["empty_w" if g % 2 else "empty_h"], gx, gy, rng) for g in range(65)], np.uint16)
    elif kind == "one_hot":
        rect = np.asarray([_unit(40, gx)] * 500, np.uint16)
    elif kind == "all_equal":
        rect = np.asarray([[0, 0, gx, gy]] * 5, np.uint16)
    else:
        raise ValueError(kind)
    return dict(name="order_" + kind, rect=rect, depths=depths_of("uniform", rect.shape[0], rng), grid_x=gx, T=T)


def sparse_case(cap):
    """12 x 10 tiles: tiles with cap - 1, cap, cap + 1 and 4 * cap entries, a third of the others empty, the rest short lists (< cap).
    Exactly two tiles are over the cap."""
    gx, gy = SPARSE_GRID
    T = gx * gy
    name = "sparse_%d" % cap
    rng = np.random.default_rng(_seed(name))
    spots = {17: cap - 1, 58: cap, 59: cap + 1, T - 1: 4 * cap}
    lists = {t: depths_of("sliver_plus_outliers" if n > cap else "uniform", n, rng) for t, n in spots.items()}
    for t in range(T):
        if t not in spots and t % 3 != 0:
            lists[t] = depths_of("two_values" if t % 5 == 0 else "uniform", int(rng.integers(1, min(cap - 1, 40))), rng)
    c = planted(name, gx, T, lists)
    c.update(cap=cap, spots=spots)
    return c
