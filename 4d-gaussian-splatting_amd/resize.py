"""Full-size 8-bit frames resized on the GPU to the training resolution (csrc/frame_resize.hip), byte for byte what the
reference's loader gets from PIL.

The reference resizes every image on the host, one at a time: utils/camera_utils.py:19-49 ``loadCam`` works out the target size
from ``--resolution`` and calls ``PILtoTorch(image, resolution)`` = ``pil_image.resize(resolution)`` (Pillow's default filter,
BICUBIC); its ``dataloader`` mode (utils/data_utils.py:16-34) does so for every view of every step, after compositing RGBA images
over the background.  Pillow's resize of 8-bit images is integer arithmetic on tables of fixed-point taps, so it can be reproduced
exactly: the tables are built here on the host in float64 (``coefficients``), cached per axis pair and device, and the kernels do
integer work only.

* ``target_resolution(orig_w, orig_h, resolution, ...)`` -- ``loadCam``'s size, scale and scaled intrinsics.
* ``coefficients(n_in, n_out)`` -- the taps and bounds of one axis as numpy int32.
* ``resize_frames(frames_u8, size, index=None, out=None)`` -- the checked wrapper of ``fdgs_frames_resize``.
* ``composite(frames_rgba, white, keep_alpha=False)`` -- the checked wrapper of ``fdgs_frames_composite``.
* ``resized_store(frames, size, ...)`` -- a ``FrameStore`` of the resized frames, built chunk by chunk: the full-size set never
  has to fit the device.  ``pyramid(frames, sizes, ...)`` -- one store per size from one upload per chunk.

There is no CPU path: the frames may live on the host, the resize runs on the GPU.
"""
import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _capi
from .frames import FrameStore, _as_u8_frames, _check_frames

PRECISION_BITS = 22


# ---- loadCam's arithmetic --------------------------------------------------------------------------------------------------------------
def target_resolution(orig_w: int, orig_h: int, resolution, resolution_scale: float = 1.0, cx=None, cy=None, fl_x=None, fl_y=None):
    """``((W, H), scale, intrinsics)`` as utils/camera_utils.py:19-45 computes them: for ``resolution`` in {1, 2, 3, 4, 8}
    ``round(orig / (resolution_scale * resolution))`` (Python's round: half to even); for -1 the original size, capped at 1600 px
    width; any other number is a target width; the last two as ``int(orig / scale)``.  ``intrinsics``: cx, cy, fl_x, fl_y divided by
    ``scale`` (None where not given)."""
    if resolution in [1, 2, 3, 4, 8]:
        size = round(orig_w / (resolution_scale * resolution)), round(orig_h / (resolution_scale * resolution))
        scale = resolution_scale * resolution
    else:
        if resolution == -1:
            global_down = orig_w / 1600 if orig_w > 1600 else 1
        else:
            global_down = orig_w / resolution
        scale = float(global_down) * float(resolution_scale)
        size = (int(orig_w / scale), int(orig_h / scale))
    intr = {name: (None if v is None else v / scale) for name, v in (("cx", cx), ("cy", cy), ("fl_x", fl_x), ("fl_y", fl_y))}
    return size, scale, intr


# ---- Pillow's tables -------------------------------------------------------------------------------------------------------------------
def coefficients(n_in: int, n_out: int) -> Tuple[np.ndarray, np.ndarray]:
    """The tables of one axis ``n_in`` -> ``n_out``: ``(k, bounds)``, ``k`` int32 [n_out, ksize] the taps in fixed point (22
    fractional bits; zero behind a row's count), ``bounds`` int32 [n_out, 2] = (xmin, count).  float64, every operation rounded on
    its own, the sum of a row's weights taken left to right -- Pillow's order."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in <= 0 or n_out <= 0:
        raise ValueError("fdgs.resize: an axis must be positive, got %d -> %d" % (n_in, n_out))
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(0, np.trunc(center - support + 0.5).astype(np.int64))
    xmax = np.minimum(n_in, np.trunc(center + support + 0.5).astype(np.int64)) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    t = np.abs(((x + xmin[:, None]) - center[:, None] + 0.5) * ss)
    a = -0.5
    w = np.where(t < 1.0, ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0, np.where(t < 2.0, (((t - 5.0) * t + 8.0) * t - 4.0) * a, 0.0))
    w = np.where(x < xmax[:, None], w, 0.0)
    total = np.zeros(n_out, np.float64)
    for j in range(ksize):   # left to right, not numpy's pairwise sum
        total = total + w[:, j]
    w = np.where((total != 0.0)[:, None], w / np.where(total != 0.0, total, 1.0)[:, None], w)
    one = float(1 << PRECISION_BITS)
    k = np.where(w < 0.0, np.trunc(w * one - 0.5), np.trunc(w * one + 0.5)).astype(np.int32)
    return np.ascontiguousarray(k), np.ascontiguousarray(np.stack([xmin, xmax], axis=1).astype(np.int32))


_tables = {}    # (n_in, n_out, device) -> (k, bounds, ksize) on the device
_scratch = {}   # device -> uint8 scratch of the two-launch path (grown on demand)
_MAX_TABLES = 64


def _device_tables(n_in, n_out, dev):
    key = (n_in, n_out, str(dev))
    hit = _tables.get(key)
    if hit is None:
        k, b = coefficients(n_in, n_out)
        if len(_tables) >= _MAX_TABLES:
            _tables.pop(next(iter(_tables)))
        hit = _tables[key] = (torch.from_numpy(k).to(dev), torch.from_numpy(b).to(dev), int(k.shape[1]))
    return hit


def _check_size(size):
    try:
        Wd, Hd = (int(s) for s in size)
    except (TypeError, ValueError):
        raise ValueError("fdgs.resize: size must be (W, H), got %r" % (size,))
    if Wd <= 0 or Hd <= 0 or (Wd, Hd) != tuple(size):
        raise ValueError("fdgs.resize: size must be two positive integers (W, H), got %r" % (size,))
    return Wd, Hd


def resize_frames(frames_u8: torch.Tensor, size: Sequence[int], index: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out[b] = PIL.Image.fromarray(frames_u8[index[b]]).resize(size)`` byte for byte, for the B entries of ``index``, on the
    current stream, without a host synchronisation.  ``frames_u8``: uint8 [N, Hs, Ws, C] on the GPU, C = 3 or 4; ``size`` = (W, H)
    in PIL's order; ``index``: int32 [B] on the same GPU (default: every frame in order; a frame may appear several times, an
    entry outside [0, N) leaves its frame of ``out`` unwritten); ``out``: contiguous uint8 [M, H, W, C] with M >= B (default: a new
    [B, H, W, C]).  One launch; two, through a cached scratch buffer of the device, where a tile's source window does not fit LDS
    (thousands of taps) -- such calls must not run concurrently on two streams of one device.  Returns ``out``."""
    N, Hs, Ws, C = _check_frames(frames_u8)
    Wd, Hd = _check_size(size)
    if not frames_u8.is_cuda:
        raise ValueError("fdgs.resize: frames must be a GPU tensor; there is no CPU path")
    dev = frames_u8.device
    if index is None:
        index = torch.arange(N, dtype=torch.int32, device=dev)
    if (not isinstance(index, torch.Tensor) or index.dtype != torch.int32 or index.dim() != 1 or not index.is_contiguous()
            or index.numel() == 0 or index.device != dev):
        raise ValueError("fdgs.resize: index must be a contiguous int32 tensor [B] (B >= 1) on %s, got %s %s" % (
            dev, tuple(getattr(index, "shape", ())), getattr(index, "dtype", type(index))))
    B = int(index.numel())
    if B > 65535:
        raise ValueError("fdgs.resize: a call takes at most 65535 frames, got %d" % B)
    if out is None:
        out = torch.empty((B, Hd, Wd, C), dtype=torch.uint8, device=dev)
    if (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != dev or out.dim() != 4 or not out.is_contiguous()
            or tuple(out.shape[1:]) != (Hd, Wd, C) or out.shape[0] < B):
        raise ValueError("fdgs.resize: out must be a contiguous uint8 tensor [M >= %d, %d, %d, %d] on %s, got %s %s" % (
            B, Hd, Wd, C, dev, tuple(getattr(out, "shape", ())), getattr(out, "dtype", type(out))))
    need = _capi.lib.fdgs_frames_resize_scratch_bytes(B, Hs, Ws, Hd, Wd, C)
    if need < 0:
        raise ValueError("fdgs.resize: unsupported sizes %s -> %s (a frame must stay below 2^31 - 4096 bytes)" % ((Hs, Ws, C), (Hd, Wd, C)))
    scratch = None
    if need > 0:
        scratch = _scratch.get(str(dev))
        if scratch is None or scratch.numel() < need:
            scratch = _scratch[str(dev)] = _capi.scratch(need, dev)
    kx, bx, ksx = _device_tables(Ws, Wd, dev)
    ky, by, ksy = _device_tables(Hs, Hd, dev)
    _capi.call("fdgs_frames_resize", dev, frames_u8.data_ptr(), N, Hs, Ws, C, index.data_ptr(), B, out.data_ptr(), int(out.shape[0]), Hd, Wd,
               kx.data_ptr(), bx.data_ptr(), ksx, ky.data_ptr(), by.data_ptr(), ksy, None if scratch is None else scratch.data_ptr(),
               arg_error=ValueError)
    return out


def composite(frames_rgba: torch.Tensor, white: bool, keep_alpha: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """RGBA frames over a white (``white``) or black background, the reference readers' float64 formula
    ``floor(((c / 255) * (a / 255) + bg * (1 - a / 255)) * 255)`` (utils/data_utils.py:20-23): uint8 [N, H, W, 4] on the GPU ->
    [N, H, W, 3], or [N, H, W, 4] with the alpha byte kept.  One launch on the current stream.  ``out``: optional, the leading
    N frames of a contiguous tensor of that shape."""
    N, H, W, C = _check_frames(frames_rgba)
    if C != 4:
        raise ValueError("fdgs.resize: compositing needs RGBA frames (C = 4), got C = %d" % C)
    if not frames_rgba.is_cuda:
        raise ValueError("fdgs.resize: frames must be a GPU tensor; there is no CPU path")
    dev = frames_rgba.device
    Co = 4 if keep_alpha else 3
    if out is None:
        out = torch.empty((N, H, W, Co), dtype=torch.uint8, device=dev)
    if (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != dev or out.dim() != 4 or not out.is_contiguous()
            or tuple(out.shape[1:]) != (H, W, Co) or out.shape[0] < N):
        raise ValueError("fdgs.resize: out must be a contiguous uint8 tensor [M >= %d, %d, %d, %d] on %s, got %s" % (
            N, H, W, Co, dev, tuple(getattr(out, "shape", ()))))
    _capi.call("fdgs_frames_composite", dev, frames_rgba.data_ptr(), N, H, W, int(bool(white)), int(bool(keep_alpha)), out.data_ptr(),
               arg_error=ValueError)
    return out[:N]


# ---- stores of resized frames ----------------------------------------------------------------------------------------------------------
def _build(frames, sizes, residency, chunk, background, slots, device):
    if residency not in ("device", "host"):
        raise ValueError("fdgs.resize: residency must be \"device\" or \"host\", got %r" % (residency,))
    if background not in (None, "white", "black"):
        raise ValueError("fdgs.resize: background must be None, \"white\" or \"black\", got %r" % (background,))
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("fdgs.resize: chunk must be at least 1, got %r" % (chunk,))
    sizes = [_check_size(s) for s in sizes]
    if not sizes:
        raise ValueError("fdgs.resize: no sizes")
    data = _as_u8_frames(frames)
    N, Hs, Ws, C = (int(s) for s in data.shape)
    if background is not None and C != 4:
        raise ValueError("fdgs.resize: a background needs RGBA frames (C = 4), got C = %d" % C)
    if device is None:
        device = data.device if data.is_cuda else torch.device("cuda", torch.cuda.current_device())
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("fdgs.resize: the resize runs on the GPU; device must be a GPU, got %s" % dev)
    chunk = min(chunk, N, 65535)
    Co = 3 if background is not None else C
    main = torch.cuda.current_stream(dev)
    with torch.cuda.device(dev):
        if residency == "device":
            results = [torch.empty((N, Hd, Wd, Co), dtype=torch.uint8, device=dev) for Wd, Hd in sizes]
            small = None
        else:
            results = [torch.empty((N, Hd, Wd, Co), dtype=torch.uint8).pin_memory() for Wd, Hd in sizes]
            small = [torch.empty((chunk, Hd, Wd, Co), dtype=torch.uint8, device=dev) for Wd, Hd in sizes]
        comp = torch.empty((chunk, Hs, Ws, 3), dtype=torch.uint8, device=dev) if background is not None else None
        on_host = not data.is_cuda
        if on_host:
            # two device staging chunks filled on a copy stream; pageable sources go through two pinned chunks first
            copy_stream = torch.cuda.Stream(dev)
            copy_stream.wait_stream(main)
            stage = [torch.empty((chunk, Hs, Ws, C), dtype=torch.uint8, device=dev) for _ in range(2)]
            pinned = None if data.is_pinned() else [torch.empty((chunk, Hs, Ws, C), dtype=torch.uint8).pin_memory() for _ in range(2)]
            uploaded, consumed = [None, None], [None, None]

            def upload(c):
                s, lo, hi = c % 2, c * chunk, min(N, (c + 1) * chunk)
                src = data[lo:hi]
                if pinned is not None:
                    if uploaded[s] is not None:
                        uploaded[s].synchronize()      # the pinned chunk is free once its last upload has left it
                    pinned[s][:hi - lo].copy_(src)
                    src = pinned[s][:hi - lo]
                with torch.cuda.stream(copy_stream):
                    if consumed[s] is not None:
                        copy_stream.wait_event(consumed[s])
                    stage[s][:hi - lo].copy_(src, non_blocking=True)
                    uploaded[s] = torch.cuda.Event()
                    uploaded[s].record(copy_stream)

            upload(0)
        elif data.device != dev:
            raise ValueError("fdgs.resize: the frames live on %s, the store was asked for on %s" % (data.device, dev))
        nchunks = (N + chunk - 1) // chunk
        for c in range(nchunks):
            lo, hi = c * chunk, min(N, (c + 1) * chunk)
            n = hi - lo
            if on_host:
                if c + 1 < nchunks:
                    upload(c + 1)
                main.wait_event(uploaded[c % 2])
                full = stage[c % 2][:n]
            else:
                full = data[lo:hi]
            if background is not None:
                full = composite(full, background == "white", out=comp)
            for r, sm, (Wd, Hd) in zip(results, small or [None] * len(sizes), sizes):
                if sm is None:
                    resize_frames(full, (Wd, Hd), out=r[lo:hi])
                else:
                    resize_frames(full, (Wd, Hd), out=sm)
                    r[lo:hi].copy_(sm[:n], non_blocking=True)
            if on_host:
                consumed[c % 2] = torch.cuda.Event()
                consumed[c % 2].record(main)
        if residency == "host":
            main.synchronize()   # the pinned results are complete
    return [FrameStore(r, residency=residency, slots=slots, device=dev) for r in results]


def resized_store(frames, size, *, residency: str = "device", chunk: int = 8, background: Optional[str] = None,
                  slots: Optional[int] = None, device=None) -> FrameStore:
    """A ``FrameStore`` of ``frames`` resized to ``size`` = (W, H): what the reference's loader keeps per camera, as uint8.
    ``frames``: full-size uint8 frames [N, H, W, C] on the host or the device -- an array, a tensor or a list, as ``FrameStore``
    accepts.  Host frames travel ``chunk`` at a time through two device staging buffers on a copy stream (pageable memory through
    two pinned chunks first), so the upload of the next chunk overlaps the resize of this one; each chunk is composited over
    ``background`` (None, "white" or "black": RGBA in, RGB out, ``composite``) if given, then resized.  The small frames stay on
    the device (``residency="device"``) or are copied to pinned host memory ("host").  Peak device memory: the result (device
    residency) plus two full-size chunks, plus one composited chunk with a background -- never the full-size set.  ``slots`` and
    ``device`` as for ``FrameStore``.  The result does not depend on ``chunk``."""
    return _build(frames, [size], residency, chunk, background, slots, device)[0]


def pyramid(frames, sizes, *, residency: str = "device", chunk: int = 8, background: Optional[str] = None,
            slots: Optional[int] = None, device=None):
    """One ``FrameStore`` per entry of ``sizes`` (the reference's ``resolution_scales``), each equal to ``resized_store`` of that
    size; the source is uploaded (and composited) once per chunk, not once per level."""
    return _build(frames, list(sizes), residency, chunk, background, slots, device)
