"""numpy restatement of csrc/compress.hip: k-means assignment and update in float64, column quantisation and the decode in float32
with exactly the operations the kernels perform (no fused multiply-add), and the decode of a whole CompressedModel into a flat bucket."""
import numpy as np

U = 2.0 ** -24   # unit roundoff of float32

# fdgs.train_host.GaussianParams.NAMES with the floats per row of the geometry segments
BUCKET = (("_xyz", 3), ("_opacity", 1), ("_scaling", 3), ("_rotation", 4), ("_t", 1), ("_scaling_t", 1), ("_rotation_r", 4))


def dist2(x, c):
    """[N, K] squared distances in float64, as |x|^2 + |c|^2 - 2 x.c (one matrix product: the direct sum over N K D elements takes
    numpy tens of seconds at the largest case).  Its own rounding, about (D + 3) 2^-53 (|x|^2 + |c|^2), is 2^-29 of the float32 bars the
    tests hold the kernels to; equal codebook rows give equal columns, so argmin's lowest-index rule decides their ties."""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    return np.maximum((x * x).sum(1)[:, None] + (c * c).sum(1)[None, :] - 2.0 * (x @ c.T), 0.0)


def assign(x, c):
    """(index [N] int32 -- the lowest k on ties --, d [N, K] float64)."""
    d = dist2(x, c)
    return np.argmin(d, axis=1).astype(np.int32), d


def assign_bar(x, c):
    """Per row: how far above the minimum the chosen centroid's float64 squared distance may lie when the comparison runs in float32,
    as the direct sum or as |c|^2 - 2 x.c (gamma_{D+2} on either side of the comparison): 4 (D + 4) u (|x|^2 + max_k |c_k|^2)."""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    return 4.0 * (x.shape[1] + 4) * U * ((x * x).sum(1) + (c * c).sum(1).max())


def update(x, index, c_old, w=None):
    """(codebook float64 [K, D], counts int32 [K], total weight [K]); rows without members or weight keep c_old."""
    x, c = np.asarray(x, np.float64), np.array(c_old, np.float64)
    K = c.shape[0]
    w = np.ones(x.shape[0], np.float64) if w is None else np.asarray(w, np.float64)
    counts = np.bincount(index, minlength=K).astype(np.int32)
    wsum = np.bincount(index, weights=w, minlength=K)
    num = np.zeros_like(c)
    np.add.at(num, index, x * w[:, None])
    live = wsum > 0
    c[live] = num[live] / wsum[live, None]
    return c, counts, wsum


def objective(x, c, index, w=None):
    """sum_n w_n |x_n - c_index[n]|^2 in float64."""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    d = ((x - c[index]) ** 2).sum(1)
    return float(d.sum() if w is None else (d * np.asarray(w, np.float64)).sum())


def ranges(lo, hi, bits):
    """float32 (step, inv) of columns [lo, hi]: (hi - lo) / qmax and qmax / (hi - lo), 0 where hi == lo."""
    qmax = np.float32((1 << bits) - 1)
    span = (np.asarray(hi, np.float32) - np.asarray(lo, np.float32)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        step = np.where(span > 0, span / qmax, np.float32(0)).astype(np.float32)
        inv = np.where(span > 0, qmax / span, np.float32(0)).astype(np.float32)
    return step, inv


def quantize(x, lo, inv, bits):
    """min(max(rint((x - lo) * inv), 0), qmax) in float32, as uint8 / uint16."""
    x, lo, inv = np.asarray(x, np.float32), np.asarray(lo, np.float32), np.asarray(inv, np.float32)
    t = np.rint(((x - lo[None, :]).astype(np.float32) * inv[None, :]).astype(np.float32))
    return np.minimum(np.maximum(t, np.float32(0)), np.float32((1 << bits) - 1)).astype(np.uint8 if bits == 8 else np.uint16)


def dequantize(q, lo, step):
    """lo + float(q) * step: one float32 product, one float32 sum."""
    prod = (q.astype(np.float32) * np.asarray(step, np.float32)[None, :]).astype(np.float32)
    return (np.asarray(lo, np.float32)[None, :] + prod).astype(np.float32)


def decode_segment(tensors, meta, name):
    q = np.asarray(tensors[name])
    if int(meta["bits"][name]) == 32:
        return q.astype(np.float32)
    return dequantize(q, meta["lo"][name], meta["step"][name])


def decode_model(tensors, meta):
    """The flat bucket (float32 [P * floats per Gaussian]) of a CompressedModel given as numpy arrays + its metadata dict."""
    P, M = int(meta["P"]), int(meta["M"])
    parts = [decode_segment(tensors, meta, name).reshape(P * C) for name, C in BUCKET]
    feats = np.empty((P, M, 3), np.float32)
    feats[:, 0, :] = decode_segment(tensors, meta, "dc")
    if M > 1:
        if "sh_codebook" in tensors:
            rest = np.asarray(tensors["sh_codebook"], np.float32)[np.asarray(tensors["sh_index"]).astype(np.int64)]
        else:
            rest = np.asarray(tensors["sh_rest"], np.float32)
        feats[:, 1:, :] = rest.reshape(P, M - 1, 3)
    parts.append(feats.reshape(-1))
    return np.concatenate(parts)
