"""The written definition of the frame resize (fdgs.resize, csrc/frame_resize.hip) in numpy: Pillow's ``Image.resize(size)`` with its
default filter BICUBIC on 8-bit RGB / RGBA images -- what the reference's loader calls for every image (utils/camera_utils.py:19-49
``loadCam`` -> utils/general_utils.py:22-28 ``PILtoTorch``) -- restated from its arithmetic, and the compositing step of the
reference's readers that comes before it (utils/data_utils.py:20-23).

Per axis n_in -> n_out, in float64 with every operation rounded on its own:

    scale = n_in / n_out, filterscale = max(scale, 1), support = 2 filterscale, ksize = ceil(support) * 2 + 1
    per output xx:  center = (xx + 0.5) scale, xmin = max(0, int(center - support + 0.5)),
                    xmax = min(n_in, int(center + support + 0.5)) - xmin,
                    w[x] = bicubic((x + xmin - center + 0.5) * (1 / filterscale)), a = -0.5; summed left to right, divided by the sum
                    k[x] = int(w * 2^22 +- 0.5)                                   (truncation toward zero)
    one pass:       out = clip(0, 255, (2^21 + sum k[x] in[xmin + x]) >> 22)     int32, arithmetic shift

horizontal pass first, into a uint8 intermediate, vertical pass over that; an unchanged axis is skipped; RGBA is premultiplied
before (whenever a pass runs) and divided by the new alpha afterwards.  tests/golden/resize/*.npz hold Pillow's own results; this
file equals them byte for byte (tests/test_resize_host.py).  ``resize_wrong_float32`` / ``resize_wrong_float_intermediate`` are the
kernels one must NOT write.
"""
import math

import numpy as np

PRECISION_BITS = 22


def _bicubic(t):
    a = -0.5
    t = abs(t)
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0
    if t < 2.0:
        return (((t - 5.0) * t + 8.0) * t - 4.0) * a
    return 0.0


def weights(n_in, n_out):
    """(ksize, bounds int32 [n_out, 2], normalised float64 weights [n_out, ksize]) of one axis."""
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((n_out, 2), np.int32)
    w = np.zeros((n_out, ksize), np.float64)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        xmax = min(n_in, int(center + support + 0.5)) - xmin
        total = 0.0
        for x in range(xmax):
            v = _bicubic((x + xmin - center + 0.5) * ss)
            w[xx, x] = v
            total += v
        if total != 0.0:
            for x in range(xmax):
                w[xx, x] /= total
        bounds[xx] = (xmin, xmax)
    return ksize, bounds, w


def coefficients(n_in, n_out):
    """(ksize, bounds int32 [n_out, 2], fixed-point taps int32 [n_out, ksize])."""
    ksize, bounds, w = weights(n_in, n_out)
    one = float(1 << PRECISION_BITS)
    k = np.where(w < 0.0, np.trunc(w * one - 0.5), np.trunc(w * one + 0.5)).astype(np.int32)
    return ksize, bounds, k


def _pass_axis0(img, n_out):
    """One pass along axis 0 of a uint8 array [n_in, ...]."""
    n_in = img.shape[0]
    _, bounds, k = coefficients(n_in, n_out)
    out = np.empty((n_out,) + img.shape[1:], np.uint8)
    src = img.astype(np.int32)
    for i in range(n_out):
        lo, n = int(bounds[i, 0]), int(bounds[i, 1])
        kk = k[i, :n].reshape((n,) + (1,) * (img.ndim - 1))
        with np.errstate(over="ignore"):
            acc = (kk * src[lo:lo + n]).sum(axis=0, dtype=np.int32) + np.int32(1 << (PRECISION_BITS - 1))
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return out


def premultiply(img):
    c = img[..., :3].astype(np.uint32)
    a = img[..., 3:4].astype(np.uint32)
    t = c * a + 128
    out = img.copy()
    out[..., :3] = (((t >> 8) + t) >> 8).astype(np.uint8)
    return out


def unpremultiply(img):
    c = img[..., :3].astype(np.uint32)
    a = img[..., 3:4].astype(np.uint32)
    div = np.minimum(255, (255 * c) // np.maximum(a, 1)).astype(np.uint8)
    out = img.copy()
    keep = (a == 0) | (a == 255)
    out[..., :3] = np.where(keep, img[..., :3], div)
    return out


def resize_image(img, size):
    """uint8 [H, W, C] (C = 3 or 4) -> [size[1], size[0], C]; ``size`` = (W, H) in PIL's order."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] not in (3, 4):
        raise ValueError("image must be uint8 [H, W, 3 or 4]")
    Wd, Hd = int(size[0]), int(size[1])
    Hs, Ws, C = img.shape
    if (Hs, Ws) == (Hd, Wd):
        return img.copy()
    work = premultiply(img) if C == 4 else img
    if Ws != Wd:
        work = _pass_axis0(work.transpose(1, 0, 2), Wd).transpose(1, 0, 2)
    if Hs != Hd:
        work = _pass_axis0(work, Hd)
    work = np.ascontiguousarray(work)
    return unpremultiply(work) if C == 4 else work


def resize(frames, size):
    """uint8 [N, H, W, C] -> [N, size[1], size[0], C]."""
    return np.stack([resize_image(f, size) for f in np.asarray(frames)])


def composite(frames_rgba, white, keep_alpha=False):
    """RGBA uint8 [..., 4] over a white / black background, the reference readers' float64 formula; the reference's
    ``np.array(arr * 255.0, dtype=np.byte)`` read as unsigned equals this floor for all 65 536 (c, a) pairs."""
    u = np.asarray(frames_rgba)
    if u.dtype != np.uint8 or u.shape[-1] != 4:
        raise ValueError("frames must be uint8 [..., 4]")
    norm = u / 255.0
    bg = 1.0 if white else 0.0
    arr = norm[..., :3] * norm[..., 3:4] + bg * (1 - norm[..., 3:4])
    rgb = np.floor(arr * 255.0).astype(np.uint8)
    return np.concatenate([rgb, u[..., 3:4]], axis=-1) if keep_alpha else rgb


# ---- the kernels one must NOT write (the tests show that their inputs tell the difference) ----------------------------------------------
def _float_pass_axis0(img_f, n_out, dtype):
    n_in = img_f.shape[0]
    _, bounds, w = weights(n_in, n_out)
    out = np.empty((n_out,) + img_f.shape[1:], dtype)
    for i in range(n_out):
        lo, n = int(bounds[i, 0]), int(bounds[i, 1])
        acc = np.zeros(img_f.shape[1:], dtype)
        for x in range(n):
            acc = (acc + dtype(w[i, x]) * img_f[lo + x].astype(dtype)).astype(dtype)
        out[i] = acc
    return out


def _round_u8(x):
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def resize_wrong_float32(img, size):
    """float32 weights and accumulation with round-to-nearest instead of the fixed-point sum (RGB only)."""
    img = np.asarray(img)
    Wd, Hd = size
    work = img
    if img.shape[1] != Wd:
        work = _round_u8(_float_pass_axis0(work.transpose(1, 0, 2), Wd, np.float32)).transpose(1, 0, 2)
    if img.shape[0] != Hd:
        work = _round_u8(_float_pass_axis0(work, Hd, np.float32))
    return np.ascontiguousarray(work)


def resize_wrong_float_intermediate(img, size):
    """The fixed-point taps, but a float (not uint8) intermediate between the two passes (RGB only)."""
    img = np.asarray(img)
    Wd, Hd = size
    one = float(1 << PRECISION_BITS)

    def fpass(x, n_out):
        _, bounds, k = coefficients(x.shape[0], n_out)
        out = np.empty((n_out,) + x.shape[1:], np.float64)
        for i in range(n_out):
            lo, n = int(bounds[i, 0]), int(bounds[i, 1])
            out[i] = (k[i, :n].reshape((n,) + (1,) * (x.ndim - 1)) * x[lo:lo + n]).sum(axis=0) / one
        return out

    work = img.astype(np.float64)
    if img.shape[1] != Wd:
        work = fpass(work.transpose(1, 0, 2), Wd).transpose(1, 0, 2)
    if img.shape[0] != Hd:
        work = fpass(work, Hd)
    return np.ascontiguousarray(np.clip(np.floor(work + 0.5), 0, 255).astype(np.uint8))
