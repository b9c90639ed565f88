"""numpy restatements of csrc/seed.hip (include/fdgs_seed.h), operation for operation where the kernels are held to bits:

* ``philox4x32_10``    -- Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3" (SC'11); checked against the
  known-answer vectors published with the algorithm (Random123 kat_vectors) in tests/test_seed_host.py.
* ``cell_keys``        -- floor((v - origin) * inv_cell) in float32, two roundings; the 64-bit key.
* ``thin``             -- stable order by key, one row per cell, sequential compensated float32 sums in ascending point index, one division.
* ``init_f32`` / ``init_f64`` -- create_from_pcd's segments in float32 (bit-exact for everything but the logarithm) and float64.
"""
import numpy as np

C0 = 0.28209479177387814
AXIS_CELLS = 65536


def philox4x32_10(counter, key):
    """counter: uint32 [..., 4], key: uint32 [..., 2] (broadcast) -> uint32 [..., 4]."""
    c = [np.asarray(counter[..., k], dtype=np.uint64) for k in range(4)]
    k0 = np.asarray(key[..., 0], dtype=np.uint64) + np.zeros_like(c[0])
    k1 = np.asarray(key[..., 1], dtype=np.uint64) + np.zeros_like(c[0])
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & mask, p1 >> np.uint64(32), p1 & mask
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0 = (k0 + np.uint64(0x9E3779B9)) & mask
        k1 = (k1 + np.uint64(0xBB67AE85)) & mask
    return np.stack(c, axis=-1).astype(np.uint32)


def draws(N, seed, stream_id):
    """(words uint32 [N, 4], uniforms float32 [N, 4]) of points 0 .. N - 1: counter = (i, stream_id, 0, 0), key = the seed's halves."""
    counter = np.zeros((N, 4), np.uint32)
    counter[:, 0] = np.arange(N, dtype=np.uint32)
    counter[:, 1] = np.uint32(stream_id)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    w = philox4x32_10(counter, key[None, :])
    u = (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return w, u


def box(u, lo, extent):
    return u[:, :3] * np.float32(extent) + np.float32(lo)


def times(u, t0, t1):
    span = np.float32(t1) - np.float32(t0)
    return (u[:, 0] * np.float32(1.2) - np.float32(0.1)) * span + np.float32(t0)


def grid_of(xyz, t, cell, cell_t):
    """(origin, inv_cell) float32 [4] as fdgs.seed.thin hands them to the kernel."""
    origin, inv = np.zeros(4, np.float32), np.zeros(4, np.float32)
    if len(xyz):
        origin[:3] = xyz.min(0)
        if t is not None:
            origin[3] = t.min()
    inv[:3] = np.float32(1.0) / np.float32(cell)
    inv[3] = np.float32(2.0 ** -100) if t is None or cell_t is None else np.float32(1.0) / np.float32(cell_t)
    return origin, inv


def cell_keys(xyz, t, origin, inv):
    """uint64 [N]: (ix << 48) | (iy << 32) | (iz << 16) | it with i = clamp(floor((v - origin) * inv), 0, 65535) in float32."""
    v = np.concatenate([xyz.astype(np.float32), (np.zeros(len(xyz), np.float32) if t is None else t.astype(np.float32))[:, None]], axis=1)
    f = np.floor((v - origin[None, :].astype(np.float32)) * inv[None, :].astype(np.float32))
    assert f.dtype == np.float32
    i = np.where(f >= 0, np.minimum(f, np.float32(AXIS_CELLS - 1)), np.float32(0)).astype(np.uint64)
    if t is None:
        i[:, 3] = 0
    return (i[:, 0] << np.uint64(48)) | (i[:, 1] << np.uint64(32)) | (i[:, 2] << np.uint64(16)) | i[:, 3]


def thin(xyz, rgb, t, origin, inv):
    """dict(key uint64 [M], count, first int32 [M], xyz, rgb float32 [M, 3], t float32 [M] or None, members: list of index arrays)."""
    keys = cell_keys(xyz, t, origin, inv)
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    heads = np.flatnonzero(np.concatenate([[True], sk[1:] != sk[:-1]])) if len(sk) else np.zeros(0, np.int64)
    ends = np.concatenate([heads[1:], [len(sk)]]).astype(np.int64)
    M = len(heads)
    out = dict(key=sk[heads], count=(ends - heads).astype(np.int32), first=order[heads].astype(np.int32), members=[order[a:b] for a, b in zip(heads, ends)],
               xyz=np.zeros((M, 3), np.float32), rgb=np.zeros((M, 3), np.float32), t=None if t is None else np.zeros(M, np.float32))
    cols = [("xyz", xyz.astype(np.float32)), ("rgb", rgb.astype(np.float32))] + ([] if t is None else [("t", t.astype(np.float32))])
    for r, idx in enumerate(out["members"]):
        assert (np.diff(idx) > 0).all()                     # ascending point index: what the stable sort leaves
        n = np.float32(len(idx))
        for name, col in cols:
            acc, comp = col[idx[0]].copy(), np.zeros_like(col[idx[0]])
            for j in idx[1:]:                               # Kahan's compensated sum, one rounding per operation
                y = (col[j] - comp).astype(np.float32)
                nxt = (acc + y).astype(np.float32)
                comp = ((nxt - acc).astype(np.float32) - y).astype(np.float32)
                acc = nxt
            out[name][r] = acc / n
    return out


def mean_bound(values, idx):
    """(float64 mean, the sequential-sum bound (n - 1) 2^-24 sum|x_i| / n) of rows ``idx`` of ``values``, per column."""
    x = values[idx].astype(np.float64)
    n = len(idx)
    return x.mean(0), (n - 1) * 2.0 ** -24 * np.abs(x).sum(0) / n


def init_constants(time_duration):
    x = np.float32(0.1)
    opacity = np.log(x / (np.float32(1.0) - x))
    with np.errstate(divide="ignore", invalid="ignore"):
        scaling_t = np.log(np.sqrt((np.float32(time_duration[1]) - np.float32(time_duration[0])) / np.float32(5.0)))
    return np.float32(opacity), np.float32(scaling_t)


def init_f32(xyz, rgb, t, dist2, M, gaussian_dim, time_duration):
    """The eight segments in float32, one rounding per operation (``_scaling``: numpy's float32 log, NOT held to bits)."""
    P = len(xyz)
    opacity, scaling_t = init_constants(time_duration)
    feats = np.zeros((P, M, 3), np.float32)
    feats[:, 0, :] = (rgb.astype(np.float32) - np.float32(0.5)) / np.float32(C0)
    ident = np.tile(np.array([1, 0, 0, 0], np.float32), (P, 1))
    four = gaussian_dim == 4
    return {"_xyz": xyz.astype(np.float32), "_opacity": np.full((P, 1), opacity, np.float32),
            "_scaling": np.repeat(np.log(np.sqrt(np.maximum(dist2.astype(np.float32), np.float32(1e-7))))[:, None], 3, axis=1),
            "_rotation": ident, "_t": (t.astype(np.float32).reshape(P, 1) if four else np.zeros((P, 1), np.float32)),
            "_scaling_t": np.full((P, 1), scaling_t if four else 0.0, np.float32), "_rotation_r": ident.copy(), "_features": feats}


def scaling_f64(dist2):
    """log(sqrt(max(d2, 1e-7))) in float64 of the float32 inputs (the clamp constant is the float32 one the kernel compares with)."""
    return np.log(np.sqrt(np.maximum(dist2.astype(np.float64), np.float64(np.float32(1e-7)))))
