"""The clouds tests/test_gpu_seed.py thins, as numpy arrays: name -> (xyz [N, 3], rgb [N, 3], t [N], cell, cell_t).  Every case is
run with its times and without them.  Seeded; built once per session."""
import numpy as np


def _cloud(rng, n, lo=-1.0, hi=1.0):
    return (rng.uniform(lo, hi, (n, 3)).astype(np.float32), rng.uniform(0, 1, (n, 3)).astype(np.float32),
            rng.uniform(0.0, 2.0, n).astype(np.float32))


def cases():
    rng = np.random.default_rng(20240607)
    out = {}
    for n in (0, 1, 2, 63, 64, 65, 257, 5000):                     # around a wave, around a workgroup, many workgroups
        out["n%d" % n] = _cloud(rng, n) + (0.25, 0.5)
    xyz, rgb, t = _cloud(rng, 500, 0.1, 0.2)
    out["one_cell"] = (xyz, rgb, (0.5 + 0.01 * t).astype(np.float32), 4.0, 4.0)
    g = np.stack(np.meshgrid(np.arange(7), np.arange(7), np.arange(6), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    g = g[rng.permutation(len(g))]
    out["own_cell"] = (g, rng.uniform(0, 1, g.shape).astype(np.float32), (np.arange(len(g)) % 5).astype(np.float32), 0.5, 0.5)
    out["negative"] = _cloud(rng, 700, -5.0, -1.0) + (0.5, 0.25)
    # exactly on cell faces: coordinates that are whole multiples of the cell size above the minimum, all exact in float32
    f = (rng.integers(0, 9, (600, 3)) * 0.25 - 1.0).astype(np.float32)
    f[0] = -1.0
    ft = (rng.integers(0, 5, 600) * 0.5).astype(np.float32)
    ft[0] = 0.0
    out["faces"] = (f, rng.uniform(0, 1, f.shape).astype(np.float32), ft, 0.25, 0.5)
    # one cell with 300 members and one with 1100 (runs that straddle a wave and a workgroup), scattered among 400 others
    a, b, c = _cloud(rng, 300, 0.30, 0.45), _cloud(rng, 1100, -0.70, -0.55), _cloud(rng, 400)
    xyz, rgb, t = (np.concatenate(p) for p in zip(a, b, c))
    t[:300], t[300:1400] = 0.1 + 0.05 * t[:300] / 2.0, 1.1 + 0.05 * t[300:1400] / 2.0
    xyz[1400], t[1400] = -1.0, 0.0                                # pins the origin: the two clusters sit inside one cell each
    p = rng.permutation(len(xyz))
    out["big_cells"] = (xyz[p], rgb[p], t[p], 0.25, 0.5)
    xyz, rgb, t = _cloud(rng, 200)
    rep = rng.integers(1, 5, 200)
    p = rng.permutation(int(rep.sum()))
    out["duplicates"] = (np.repeat(xyz, rep, 0)[p], np.repeat(rgb, rep, 0)[p], np.repeat(t, rep)[p], 0.125, 0.25)
    return out
