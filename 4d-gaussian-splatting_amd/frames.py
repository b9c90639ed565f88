"""Ground-truth frames kept as 8-bit images and decoded on the GPU (csrc/frames.hip).

The reference's loader turns every image into a float32 tensor on the host (utils/general_utils.py:22-28 ``PILtoTorch``:
``np.array(pil) / 255.0`` permuted to [C, H, W]; scene/cameras.py:53-57 multiplies by the alpha channel; utils/data_utils.py:16-34
does the same per batch) and moves it to the device inside the step (train.py:106).  Here the frames stay uint8, on the device or
in pinned host memory -- a quarter of the memory or of the bus traffic -- and one kernel launch per batch writes exactly those
float tensors, bit for bit: ``v = float(u8) / 255.0f``, and with an alpha channel ``mask = a / 255.0f``, ``rgb = v * mask``.

* ``decode_frames(frames_u8, index, out, mask_out=None)`` -- the checked wrapper of ``fdgs_frames_decode``.
* ``FrameStore`` -- N frames, a ring of float slots, ``store.batch(idx)`` / ``store[i]``; usable wherever a sequence of ground-truth
  tensors is (``harness.train(..., gts=store)``, ``metrics.evaluate(model, cams, store, ...)``).

And the way back (csrc/frame_encode.hip): float images out as uint8 frames, torchvision ``save_image``'s rule
``img.mul(255).add(0.5).clamp(0, 255).to(uint8)`` bit for bit (NaN -> 0), the exact inverse of the decode for all 256 bytes.

* ``encode_frames(images, index, frames_u8, alphas=None)`` / ``encode_gray(planes, index, frames_u8)`` -- the checked wrappers of
  ``fdgs_frames_encode`` / ``fdgs_frames_encode_gray`` (the reference's grey depth image, utils/image_utils.py:21-28).
* ``FrameWriter`` -- the counterpart of ``FrameStore``: N frames written one launch at a time, on the device or through a ring of
  device slots into pinned host memory.

There is no CPU path: the frames may live on the host, the decode runs on the GPU.
"""
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _capi

_ALIGN = 64   # floats: every slot starts on a 256-byte boundary, as a tensor of its own would


def _check_frames(frames_u8):
    if not isinstance(frames_u8, torch.Tensor) or frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or not frames_u8.is_contiguous():
        raise ValueError("fdgs.frames: frames must be a contiguous uint8 tensor [N, H, W, C], got %s %s" % (
            tuple(getattr(frames_u8, "shape", ())), getattr(frames_u8, "dtype", type(frames_u8))))
    N, H, W, C = (int(s) for s in frames_u8.shape)
    if C not in (3, 4):
        raise ValueError("fdgs.frames: frames must have 3 (RGB) or 4 (RGBA) channels, got C = %d" % C)
    if N <= 0 or H <= 0 or W <= 0:
        raise ValueError("fdgs.frames: empty frame array %s" % ((N, H, W, C),))
    return N, H, W, C


def decode_frames(frames_u8: torch.Tensor, index: torch.Tensor, out: torch.Tensor, mask_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out[b] = PILtoTorch(frames_u8[index[b]])`` (times its alpha plane for RGBA frames) for the B entries of ``index``, in one
    launch on the current stream, without a host synchronisation.  ``frames_u8``: uint8 [N, H, W, C] on the GPU, C = 3 or 4;
    ``index``: int32 [B] on the same GPU (a frame may appear several times; an entry outside [0, N) leaves its image unwritten);
    ``out``: float32 [B, 3, H, W], ``mask_out`` (RGBA only, optional): float32 [B, 1, H, W] -- both may be strided along the first
    dimension (slots of a larger buffer) and contiguous within an image.  Returns ``out``."""
    N, H, W, C = _check_frames(frames_u8)
    for name, t in (("frames", frames_u8), ("index", index), ("out", out), ("mask_out", mask_out)):
        if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise ValueError("fdgs.frames: %s must be a GPU tensor; there is no CPU path" % name)
    dev = frames_u8.device
    if index.dtype != torch.int32 or index.dim() != 1 or not index.is_contiguous() or index.numel() == 0 or index.device != dev:
        raise ValueError("fdgs.frames: index must be a contiguous int32 tensor [B] (B >= 1) on %s, got %s %s" % (dev, tuple(index.shape), index.dtype))
    B = int(index.numel())

    def strided(t, name, planes):
        if (t.dtype != torch.float32 or t.device != dev or tuple(t.shape) != (B, planes, H, W) or not t[0].is_contiguous()
                or (B > 1 and t.stride(0) < planes * H * W)):
            raise ValueError("fdgs.frames: %s must be float32 [%d, %d, %d, %d] on %s with contiguous images, got %s %s strides %s" % (
                name, B, planes, H, W, dev, tuple(t.shape), t.dtype, tuple(t.stride())))
        return int(t.stride(0)) if B > 1 else planes * H * W

    out_stride = strided(out, "out", 3)
    mask_stride = 0
    if mask_out is not None:
        if C != 4:
            raise ValueError("fdgs.frames: mask_out needs RGBA frames (C = 4), got C = %d" % C)
        mask_stride = strided(mask_out, "mask_out", 1)
    _capi.call("fdgs_frames_decode", dev, frames_u8.data_ptr(), N, H, W, C, index.data_ptr(), B, out.data_ptr(), out_stride,
               None if mask_out is None else mask_out.data_ptr(), mask_stride, arg_error=ValueError)
    return out


def _as_u8_frames(frames) -> torch.Tensor:
    """uint8 [N, H, W, C] from an array, a tensor or a list of [H, W, C] arrays / tensors of one shape (on whatever device it is)."""
    if isinstance(frames, (list, tuple)):
        if len(frames) == 0:
            raise ValueError("fdgs.frames: no frames")
        items = [f if isinstance(f, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(f)) for f in frames]
        shapes = {tuple(f.shape) for f in items}
        if len(shapes) != 1:
            raise ValueError("fdgs.frames: all frames of a store must have one shape, got %s" % sorted(shapes))
        if items[0].dim() != 3:
            raise ValueError("fdgs.frames: a frame must be [H, W, C], got %s" % (tuple(items[0].shape),))
        if any(f.dtype != torch.uint8 for f in items):
            raise ValueError("fdgs.frames: frames must be uint8, got %s" % sorted({str(f.dtype) for f in items}))
        frames = torch.stack(items)
    elif isinstance(frames, np.ndarray):
        frames = torch.from_numpy(np.ascontiguousarray(frames))
    if isinstance(frames, torch.Tensor) and frames.dtype == torch.uint8 and frames.dim() == 4:
        frames = frames.contiguous()
    _check_frames(frames)
    return frames


def ring_runs(cursor: int, n: int, slots: int) -> List[tuple]:
    """The next ``n`` slots of a ring of ``slots`` from ``cursor`` on, as runs (first slot, count) of consecutive slots: one run, or
    two where the ring wraps.  (A decode launch writes consecutive slots, so a batch that wraps takes two launches; never with
    ``slots`` a multiple of the batch size.)"""
    if n < 1 or n > slots:
        raise ValueError("fdgs.frames: a batch of %d frames does not fit a ring of %d slots" % (n, slots))
    first = cursor % slots
    if first + n <= slots:
        return [(first, n)]
    return [(first, slots - first), (0, n - (slots - first))]


def check_index(idx, N: int) -> List[int]:
    """``idx`` as a list of frame numbers in [0, N) (negative numbers count from the end); ValueError otherwise -- checked on the host,
    before anything is uploaded or launched."""
    out = []
    for i in idx:
        j = int(i)
        if j != i or not -N <= j < N:
            raise ValueError("fdgs.frames: frame index %r out of range for %d frames" % (i, N))
        out.append(j % N)
    if not out:
        raise ValueError("fdgs.frames: an empty batch")
    return out


class FrameStore:
    """N ground-truth frames of one shape kept as uint8 [N, H, W, C] (C = 3, or 4 with an alpha channel) and handed out as the
    float32 [3, H, W] tensors the reference's loader produces (module docstring), decoded by one launch per batch.

    ``frames``: a uint8 array / tensor [N, H, W, C] or a list of [H, W, C] arrays of one shape -- what ``PILtoTorch`` is handed.
    ``residency="device"``: the frames live on ``device``.  ``residency="host"``: in pinned host memory; ``prefetch(idx)`` starts the
    upload of a batch into a device staging ring of ``slots`` uint8 frames on a copy stream of the store's own, ``batch(idx)`` makes
    the caller's stream wait for it (an event) and decodes from the staging ring; without a matching ``prefetch`` it uploads on the
    spot.  A staging slot is not overwritten before the decode that last read it has finished (an event the copy stream waits for).
    ``slots``: the number of float images (and masks, and staging frames) of the ring; default: twice the first batch's size, at
    least 2 (``harness.train`` asks for twice its batch size: ``reserve``).

    Lifetime rule: a tensor returned by ``batch`` / ``masks`` / ``store[i]`` is a view of a ring slot and is valid until ``slots``
    further frames have been decoded by this store; after that it holds another frame.  Clone what must live longer.  The decode
    runs on the caller's current stream, so reusing a slot is ordered behind everything enqueued on that stream before -- work on
    OTHER streams that still reads a slot must have been joined to the caller's stream first.  ``StepPipeline.step`` does that:
    its streams F and B wait for the caller's stream in ``_begin`` and the caller's stream waits for both (and for stream A) in
    ``_join``, so a decode enqueued on the caller's stream after ``step()`` returned is ordered behind every reader of the previous
    step's slots, and the step's readers (the loss kernels and the opacity-mask term, all on stream B) behind the decode.  This
    holds for every mode of the pipeline, ``overlap_steps`` included: a carried step lets stream F start without waiting for the
    caller's stream, but stream F never reads a ground truth, and stream B waits in every step.  B slots would therefore do for
    ``harness.train``; 2 B keep the previous batch readable while the next one is decoded (the logging line, a caller's own look at
    the last step's images) and let a host store upload one batch ahead.

    ``len(store)``, ``store.shape`` = (H, W, C), ``store.has_alpha``; ``store[i]`` decodes one frame, so a store can be passed
    wherever a sequence of ground-truth tensors is accepted (mind the lifetime rule: do not build a list of more than ``slots``)."""

    def __init__(self, frames, residency: str = "device", slots: Optional[int] = None, device=None):
        if residency not in ("device", "host"):
            raise ValueError("fdgs.frames: residency must be \"device\" or \"host\", got %r" % (residency,))
        if slots is not None and int(slots) < 2:
            raise ValueError("fdgs.frames: a store needs at least 2 slots, got %r" % (slots,))
        data = _as_u8_frames(frames)
        self.N, self.H, self.W, self.C = (int(s) for s in data.shape)
        if device is None:
            device = data.device if data.is_cuda else torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("fdgs.frames: the decode runs on the GPU; device must be a GPU, got %s" % self.device)
        self.residency = residency
        if residency == "device":
            self.frames = data.to(self.device)
        else:
            self.frames = data.cpu() if data.is_pinned() else data.cpu().pin_memory()
        self.slots = None if slots is None else int(slots)
        self._explicit = slots is not None
        self._cursor = 0           # float / mask slots handed out so far
        self._ring = self._mask_ring = None
        # host residency
        self._stage = None         # uint8 [slots, H, W, C] on the device
        self._stage_cursor = 0
        self._stage_read = []      # per staging slot: the event behind the decode that last read it
        self._pending = []         # prefetched batches not yet decoded: (frame numbers, first staging cursor, upload event)
        self._copy_stream = None
        # the batches' frame numbers travel through a small ring of pinned rows; a row is reused once the decode that read it is done
        self._idx_rows = 8
        self._idx_host = self._idx_dev = None
        self._idx_done = [None] * self._idx_rows
        self._idx_k = 0
        self.launches = 0          # decode launches so far

    def __len__(self):
        return self.N

    @property
    def shape(self):
        return (self.H, self.W, self.C)

    @property
    def has_alpha(self):
        return self.C == 4

    def reserve(self, batch_size: int):
        """``harness.train``: batches of ``batch_size`` frames are coming.  A store built without ``slots`` gets a ring of at least
        twice that; one built with an explicit ``slots`` keeps it -- ValueError if a batch does not fit."""
        B = max(1, int(batch_size))
        if self._explicit:
            if self.slots < B:
                raise ValueError("fdgs.frames: a batch of %d frames does not fit a ring of %d slots" % (B, self.slots))
        elif self.slots is None or self.slots < 2 * B:
            self._drop_rings()
            self.slots = max(2, 2 * B)

    def _drop_rings(self):
        # (tensors handed out keep the old ring alive; pending uploads went into the old staging ring)
        self._ring = self._mask_ring = self._stage = None
        self._pending, self._stage_read = [], []
        self._cursor = self._stage_cursor = 0

    def _rings(self, n):
        if self.slots is None:
            self.slots = max(2, 2 * n)
        if n > self.slots:
            if self._explicit:
                raise ValueError("fdgs.frames: a batch of %d frames does not fit a ring of %d slots" % (n, self.slots))
            self._drop_rings()
            self.slots = 2 * n
        if self._ring is None:
            HW = self.H * self.W
            pad = lambda k: (k + _ALIGN - 1) // _ALIGN * _ALIGN
            self._ring = torch.empty((self.slots, pad(3 * HW)), dtype=torch.float32, device=self.device)
            if self.has_alpha:
                self._mask_ring = torch.empty((self.slots, pad(HW)), dtype=torch.float32, device=self.device)
            if self.residency == "host":
                self._stage = torch.empty((self.slots, self.H, self.W, self.C), dtype=torch.uint8, device=self.device)
                self._stage_read = [None] * self.slots
                if self._copy_stream is None:
                    self._copy_stream = torch.cuda.Stream(self.device)
                # (the staging ring may be memory that work queued on the allocating stream still uses)
                self._copy_stream.wait_stream(torch.cuda.current_stream(self.device))
        if self._idx_host is None or self._idx_host.shape[1] < self.slots:
            self._idx_host = torch.empty((self._idx_rows, self.slots), dtype=torch.int32).pin_memory()
            self._idx_dev = torch.empty((self._idx_rows, self.slots), dtype=torch.int32, device=self.device)
            self._idx_done = [None] * self._idx_rows

    def _images(self, first, n):
        HW = self.H * self.W
        return self._ring[first:first + n, :3 * HW].unflatten(1, (3, self.H, self.W))

    def _masks(self, first, n):
        return self._mask_ring[first:first + n, :self.H * self.W].unflatten(1, (1, self.H, self.W))

    def _device_index(self, numbers):
        """``numbers`` as an int32 device tensor: through the next pinned row, on the current stream, without a synchronisation
        (the host waits only if the decode that used this row ``_idx_rows`` launches ago is still running)."""
        r = self._idx_k % self._idx_rows
        self._idx_k += 1
        if self._idx_done[r] is not None:
            self._idx_done[r].synchronize()
        n = len(numbers)
        self._idx_host[r, :n] = torch.tensor(numbers, dtype=torch.int32)
        dst = self._idx_dev[r, :n]
        dst.copy_(self._idx_host[r, :n], non_blocking=True)
        return r, dst

    # -- host residency ------------------------------------------------------------------------------------------------------
    def prefetch(self, idx: Sequence[int]):
        """Host residency: start the upload of the frames ``idx`` into the next staging slots on the store's copy stream; the next
        ``batch`` of the same frame numbers decodes from there.  Device residency: nothing to do."""
        numbers = check_index(idx, self.N)
        if self.residency != "host":
            return
        self._rings(len(numbers))
        self._upload(numbers)

    def _upload(self, numbers):
        n, S = len(numbers), self.slots
        first = self._stage_cursor
        self._stage_cursor += n
        # uploads whose staging slots are taken again before they were decoded are forgotten (batch() then uploads anew)
        self._pending = [p for p in self._pending if p[1] + S >= self._stage_cursor]
        cs = self._copy_stream
        with torch.cuda.stream(cs):
            for j, f in enumerate(numbers):
                s = (first + j) % S
                if self._stage_read[s] is not None:
                    cs.wait_event(self._stage_read[s])
                    self._stage_read[s] = None
                self._stage[s].copy_(self.frames[f], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(cs)
        entry = (tuple(numbers), first, ev)
        self._pending.append(entry)
        return entry

    # -- decoding ------------------------------------------------------------------------------------------------------------
    def batch(self, idx: Sequence[int], masks: bool = False):
        """The frames ``idx`` as a list of float32 [3, H, W] tensors (views of the next ``len(idx)`` ring slots), decoded by one
        launch on the caller's current stream; with ``masks=True`` (RGBA stores) ``(images, masks)``, the masks [1, H, W] written
        by the same launch.  See the lifetime rule in the class docstring."""
        numbers = check_index(idx, self.N)
        if masks and not self.has_alpha:
            raise ValueError("fdgs.frames: masks need an alpha channel; the store's frames are RGB")
        n = len(numbers)
        self._rings(n)
        main = torch.cuda.current_stream(self.device)
        if self.residency == "host":
            hit = next((p for p in self._pending if p[0] == tuple(numbers)), None)
            if hit is None:
                hit = self._upload(numbers)
            self._pending.remove(hit)
            main.wait_event(hit[2])
            source, numbers = self._stage, [(hit[1] + j) % self.slots for j in range(n)]
            staged = list(numbers)
        else:
            source, staged = self.frames, ()
        images, mask_list, done = [], [], None
        with torch.cuda.device(self.device):
            k = 0
            for first, count in ring_runs(self._cursor, n, self.slots):
                row, index = self._device_index(numbers[k:k + count])
                out = self._images(first, count)
                mk = self._masks(first, count) if masks else None
                decode_frames(source, index, out, mk)
                self.launches += 1
                done = torch.cuda.Event()
                done.record(main)
                self._idx_done[row] = done
                images += list(out.unbind(0))
                if masks:
                    mask_list += list(mk.unbind(0))
                k += count
        self._cursor += n
        for s in staged:
            self._stage_read[s] = done
        return (images, mask_list) if masks else images

    def masks(self, idx: Sequence[int]):
        """The alpha planes ``a / 255`` of the frames ``idx`` as float32 [1, H, W] tensors (RGBA stores); takes ring slots like
        ``batch`` does.  A caller that wants images and masks of one batch uses ``batch(idx, masks=True)``: one launch for both."""
        return self.batch(idx, masks=True)[1]

    def __getitem__(self, i):
        if isinstance(i, slice):
            raise TypeError("fdgs.frames: a FrameStore hands out single frames or batch(idx); slices would outlive the ring")
        j = int(i)
        if not -self.N <= j < self.N:
            raise IndexError("fdgs.frames: frame index %d out of range for %d frames" % (j, self.N))
        return self.batch([j])[0]


# ---- the way back: float images -> uint8 frames ---------------------------------------------------------------------------------
def _check_encode(images, index, frames_u8, planes, what):
    """Shared argument checks of the two encoders; returns (N, H, W, C, B, stride of ``images`` in floats)."""
    for name, t in ((what, images), ("index", index), ("frames", frames_u8)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise ValueError("fdgs.frames: %s must be a GPU tensor; there is no CPU path" % name)
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or not frames_u8.is_contiguous() or 0 in frames_u8.shape:
        raise ValueError("fdgs.frames: frames must be a contiguous uint8 tensor [N, H, W, C], got %s %s" % (tuple(frames_u8.shape), frames_u8.dtype))
    N, H, W, C = (int(s) for s in frames_u8.shape)
    dev = frames_u8.device
    if index.dtype != torch.int32 or index.dim() != 1 or not index.is_contiguous() or index.numel() == 0 or index.device != dev:
        raise ValueError("fdgs.frames: index must be a contiguous int32 tensor [B] (B >= 1) on %s, got %s %s" % (dev, tuple(index.shape), index.dtype))
    B = int(index.numel())
    return N, H, W, C, B, _batch_stride(images, what, B, planes, H, W, dev)


def _batch_stride(t, name, B, planes, H, W, dev):
    if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != dev or tuple(t.shape) != (B, planes, H, W)
            or not t[0].is_contiguous() or (B > 1 and t.stride(0) < planes * H * W)):
        raise ValueError("fdgs.frames: %s must be float32 [%d, %d, %d, %d] on %s with contiguous images, got %s %s" % (
            name, B, planes, H, W, dev, tuple(getattr(t, "shape", ())), getattr(t, "dtype", type(t))))
    return int(t.stride(0)) if B > 1 else planes * H * W


def encode_frames(images: torch.Tensor, index: torch.Tensor, frames_u8: torch.Tensor, alphas: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``frames_u8[index[b]] = (images[b] * 255 + 0.5).clamp(0, 255).to(uint8)`` in [H, W, C] order for the B entries of ``index``, in
    one launch on the current stream, without a host synchronisation (NaN -> 0; the product and the sum are rounded separately).
    ``images``: float32 [B, 3, H, W]; ``frames_u8``: contiguous uint8 [N, H, W, C], C = 3 or 4; with C = 4 ``alphas``: float32
    [B, 1, H, W] for the fourth byte -- both may be strided along the first dimension and contiguous within an image; ``index``:
    int32 [B] on the same GPU (an entry outside [0, N) writes nothing).  Gradients are not tracked.  Returns ``frames_u8``."""
    images = images.detach() if isinstance(images, torch.Tensor) else images
    N, H, W, C, B, stride = _check_encode(images, index, frames_u8, 3, "images")
    if C not in (3, 4):
        raise ValueError("fdgs.frames: frames must have 3 (RGB) or 4 (RGBA) channels, got C = %d" % C)
    if (alphas is not None) != (C == 4):
        raise ValueError("fdgs.frames: alphas go with RGBA frames (C = 4) and only with them, got C = %d and alphas %s" % (
            C, "given" if alphas is not None else "missing"))
    astride = 0
    if alphas is not None:
        alphas = alphas.detach() if isinstance(alphas, torch.Tensor) else alphas
        astride = _batch_stride(alphas, "alphas", B, 1, H, W, frames_u8.device)
    dev = frames_u8.device
    _capi.call("fdgs_frames_encode", dev, images.data_ptr(), stride, None if alphas is None else alphas.data_ptr(), astride, B, H, W, C,
               frames_u8.data_ptr(), N, index.data_ptr(), arg_error=ValueError)
    return frames_u8


def gray_scratch(B: int, H: int, W: int, device) -> torch.Tensor:
    """Device scratch of ``encode_gray`` for batches of up to B planes [H, W] (the min / max partials)."""
    nbytes = _capi.lib.fdgs_frames_encode_gray_scratch_bytes(int(B), int(H), int(W))
    if nbytes < 0:
        raise ValueError("fdgs.frames: invalid plane shape %s" % ((B, H, W),))
    return _capi.scratch(nbytes, device).view(torch.float32)


def encode_gray(planes: torch.Tensor, index: torch.Tensor, frames_u8: torch.Tensor, scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The reference's grey depth image (``easy_cmap``, utils/image_utils.py:21-28): ``g = clamp((d - d.min()) / (d.max() - d.min()),
    0, 1)`` per plane, then the quantisation of ``encode_frames``, into ``frames_u8[index[b]]``: contiguous uint8 [N, H, W, 1] -- ONE
    channel (``easy_cmap`` writes the same value three times; ``frames.expand(-1, -1, -1, 3)`` is that image).  A constant plane gives
    0 / 0 = NaN in the reference and 0 here.  ``planes``: float32 [B, 1, H, W], may be strided along the first dimension.  Two
    launches on the current stream (min / max, encode); ``scratch``: ``gray_scratch(B, H, W, device)``, allocated if not given."""
    planes = planes.detach() if isinstance(planes, torch.Tensor) else planes
    N, H, W, C, B, stride = _check_encode(planes, index, frames_u8, 1, "planes")
    if C != 1:
        raise ValueError("fdgs.frames: grey frames have one channel [N, H, W, 1], got C = %d" % C)
    dev = frames_u8.device
    need = _capi.lib.fdgs_frames_encode_gray_scratch_bytes(B, H, W)
    if need < 0:
        raise ValueError("fdgs.frames: invalid plane shape %s" % ((B, H, W),))
    if scratch is None:
        scratch = gray_scratch(B, H, W, dev)
    elif scratch.device != dev or not scratch.is_contiguous() or scratch.numel() * scratch.element_size() < need:
        raise ValueError("fdgs.frames: scratch must be a contiguous tensor of at least %d bytes on %s" % (need, dev))
    _capi.call("fdgs_frames_encode_gray", dev, planes.data_ptr(), stride, B, H, W, frames_u8.data_ptr(), N, index.data_ptr(), scratch.data_ptr(),
               arg_error=ValueError)
    return frames_u8


class FrameWriter:
    """``n_frames`` frames of one shape collected as uint8 [N, H, W, C] -- what ``FrameStore`` accepts -- from float images on the
    GPU, encoded by one launch per ``write`` / ``write_batch`` on the caller's current stream (``encode_frames``; ``channels`` = 3,
    4 with an alpha plane as the fourth byte, or 1: grey planes through ``write_gray`` / ``encode_gray``).

    ``residency="device"``: the launch writes straight into the [N, H, W, C] device tensor.  ``residency="host"``: into a ring of
    ``slots`` device frames (default 2); each slot is then copied into a pinned [N, H, W, C] host tensor on a copy stream of the
    writer's own, which waits for the encode's event; the copy leaves an event per slot, and the encode that takes the slot again
    is ordered behind it ON THE STREAM (``wait_event``): the host never waits in ``write``, the render of the next view is enqueued
    while this one's copy travels.  ``finish()`` waits for the outstanding copies and returns the tensor; ``.frames`` before
    ``finish()`` raises.  The inputs are read by the encode only, on the caller's stream: they may be reused as soon as ``write``
    returned, stream-ordered."""

    def __init__(self, n_frames: int, H: int, W: int, channels: int = 3, residency: str = "host", slots: Optional[int] = None, device=None):
        if residency not in ("device", "host"):
            raise ValueError("fdgs.frames: residency must be \"device\" or \"host\", got %r" % (residency,))
        if channels not in (1, 3, 4):
            raise ValueError("fdgs.frames: a writer has 1 (grey), 3 (RGB) or 4 (RGBA) channels, got %r" % (channels,))
        N, H, W = int(n_frames), int(H), int(W)
        if N <= 0 or H <= 0 or W <= 0:
            raise ValueError("fdgs.frames: empty frame array %s" % ((N, H, W, channels),))
        if slots is not None and int(slots) < 1:
            raise ValueError("fdgs.frames: a writer needs at least 1 slot, got %r" % (slots,))
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("fdgs.frames: the encode runs on the GPU; device must be a GPU, got %s" % self.device)
        self.N, self.H, self.W, self.C = N, H, W, int(channels)
        self.residency = residency
        self.launches = 0          # encode launches so far (a grey batch: one reduction + one encode = 1)
        self._finished = False
        self._scratch = None
        if residency == "device":
            self.slots = N
            self._frames = self._target = torch.empty((N, H, W, self.C), dtype=torch.uint8, device=self.device)
            self._numbers = torch.arange(N, dtype=torch.int32, device=self.device)
        else:
            self.slots = min(N, 2 if slots is None else int(slots))
            self._frames = torch.empty((N, H, W, self.C), dtype=torch.uint8).pin_memory()
            self._target = torch.empty((self.slots, H, W, self.C), dtype=torch.uint8, device=self.device)
            # slot numbers of a run that starts anywhere in the ring and wraps: one launch for any run of up to `slots` frames
            self._numbers = (torch.arange(2 * self.slots, dtype=torch.int32, device=self.device) % self.slots).contiguous()
            self._copied = [None] * self.slots      # per slot: the event behind the copy that last read it
            self._cursor = 0
            self._copy_stream = torch.cuda.Stream(self.device)

    def __len__(self):
        return self.N

    @property
    def shape(self):
        return (self.H, self.W, self.C)

    @property
    def frames(self) -> torch.Tensor:
        if not self._finished:
            raise RuntimeError("fdgs.frames: FrameWriter.frames before finish(): copies may still be travelling")
        return self._frames

    def finish(self) -> torch.Tensor:
        """Waits for the outstanding copies (host residency; a device-resident result is stream-ordered like any tensor) and
        returns uint8 [N, H, W, C]."""
        if self.residency == "host":
            for ev in self._copied:
                if ev is not None:
                    ev.synchronize()
        self._finished = True
        return self._frames

    def _run(self, first, B, encode):
        """Frames first .. first + B - 1 (B <= slots): ``encode(index, target)`` once, then the copies of host residency."""
        if self.residency == "device":
            encode(self._numbers[first:first + B], self._target)
            self._finished = False
            self.launches += 1
            return
        main = torch.cuda.current_stream(self.device)
        c = self._cursor % self.slots
        used = [(c + j) % self.slots for j in range(B)]
        for s in used:
            if self._copied[s] is not None:
                main.wait_event(self._copied[s])
        encode(self._numbers[c:c + B], self._target)
        self._finished = False
        self.launches += 1
        self._cursor += B
        done = torch.cuda.Event()
        done.record(main)
        cs = self._copy_stream
        cs.wait_event(done)
        with torch.cuda.stream(cs):
            k = 0
            for s0, count in ring_runs(c, B, self.slots):
                self._frames[first + k:first + k + count].copy_(self._target[s0:s0 + count], non_blocking=True)
                k += count
            ev = torch.cuda.Event()
            ev.record(cs)
        for s in used:
            self._copied[s] = ev

    def _batches(self, first, images, planes, name, extra=None):
        first = int(first)
        if not isinstance(images, torch.Tensor) or images.dim() != 4 or tuple(images.shape[1:]) != (planes, self.H, self.W):
            raise ValueError("fdgs.frames: %s must be float32 [B, %d, %d, %d], got %s" % (name, planes, self.H, self.W, tuple(getattr(images, "shape", ()))))
        B = int(images.shape[0])
        if B < 1 or not 0 <= first <= self.N - B:
            raise ValueError("fdgs.frames: frames %d .. %d out of range for %d frames" % (first, first + B - 1, self.N))
        if extra is not None and (not isinstance(extra, torch.Tensor) or tuple(extra.shape) != (B, 1, self.H, self.W)):
            raise ValueError("fdgs.frames: alphas must be float32 [%d, 1, %d, %d], got %s" % (B, self.H, self.W, tuple(getattr(extra, "shape", ()))))
        step = min(self.slots, 65535)   # a launch takes at most 65535 images, a run of host residency at most the ring
        for k in range(0, B, step):
            yield first + k, images[k:k + step], (None if extra is None else extra[k:k + step])

    def write_batch(self, first: int, images: torch.Tensor, alphas: Optional[torch.Tensor] = None):
        """Frames ``first`` .. ``first + B - 1`` from ``images`` float32 [B, 3, H, W] (and ``alphas`` [B, 1, H, W] with 4 channels): one
        launch (host residency: one per ``slots`` frames)."""
        if self.C == 1:
            raise ValueError("fdgs.frames: a grey writer (channels = 1) takes write_gray")
        if (alphas is not None) != (self.C == 4):
            raise ValueError("fdgs.frames: alphas go with 4 channels and only with them (channels = %d)" % self.C)
        for f, im, al in list(self._batches(first, images, 3, "images", alphas)):
            self._run(f, int(im.shape[0]), lambda index, target, im=im, al=al: encode_frames(im, index, target, al))

    def write(self, i: int, image: torch.Tensor, alpha: Optional[torch.Tensor] = None):
        """Frame ``i`` from ``image`` float32 [3, H, W] (and ``alpha`` [1, H, W] with 4 channels): one launch."""
        if not isinstance(image, torch.Tensor) or image.dim() != 3:
            raise ValueError("fdgs.frames: image must be float32 [3, %d, %d], got %s" % (self.H, self.W, tuple(getattr(image, "shape", ()))))
        if alpha is not None and (not isinstance(alpha, torch.Tensor) or alpha.dim() != 3):
            raise ValueError("fdgs.frames: alpha must be float32 [1, %d, %d], got %s" % (self.H, self.W, tuple(getattr(alpha, "shape", ()))))
        self.write_batch(i, image[None], None if alpha is None else alpha[None])

    def write_gray(self, first: int, planes: torch.Tensor):
        """Grey frames (``encode_gray``) ``first`` .. from ``planes`` float32 [B, 1, H, W] or one plane [1, H, W] / [H, W]."""
        if self.C != 1:
            raise ValueError("fdgs.frames: write_gray needs a grey writer (channels = 1), this one has %d channels" % self.C)
        if isinstance(planes, torch.Tensor) and planes.dim() in (2, 3):
            planes = planes.reshape(1, 1, self.H, self.W) if planes.numel() == self.H * self.W and planes.is_contiguous() else planes
        for f, pl, _ in list(self._batches(first, planes, 1, "planes")):
            B = int(pl.shape[0])
            if self._scratch is None:
                self._scratch = gray_scratch(min(self.slots, 65535), self.H, self.W, self.device)
            self._run(f, B, lambda index, target, pl=pl: encode_gray(pl, index, target, self._scratch))
