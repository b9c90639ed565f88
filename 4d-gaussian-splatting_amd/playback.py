"""Camera paths rendered to 8-bit frames: what comes OUT of a trained model (bullet time, free-view video, a time sweep).

``render_path`` is the forward-only loop of ``fdgs.metrics.evaluate`` with a ``fdgs.frames.FrameWriter`` behind it instead of the
metrics kernels: per view one ``render_raw`` (with the environment-map composite when ``pipe.env_map_res`` is set) and ONE encode
launch (csrc/frame_encode.hip) -- no chain of elementwise PyTorch launches, no float image crossing the bus, no host wait per frame.
With ``residency="host"`` the bytes of view i travel to pinned host memory on the writer's copy stream while view i + 1 renders.

``with_timestamp`` / ``time_sweep`` build the simplest path, a fixed camera through time.  Pose interpolation is up to the caller:
any sequence of cameras of one image size is a path.
"""
import copy
from typing import Callable, List, Optional, Sequence

import torch

from .frames import FrameWriter


def with_timestamp(cam, t: float):
    """A shallow copy of ``cam`` (its matrices are shared, not copied) at time ``t``."""
    c = copy.copy(cam)
    c.timestamp = float(t)
    return c


def time_sweep(cam, t0: float, t1: float, n: int) -> List:
    """``n`` copies of ``cam`` at times evenly spaced from ``t0`` to ``t1`` inclusive (n = 1: ``t0``)."""
    n = int(n)
    if n < 1:
        raise ValueError("fdgs.playback.time_sweep: need at least one view, got n = %d" % n)
    return [with_timestamp(cam, t0 if n == 1 else t0 + (t1 - t0) * (k / (n - 1))) for k in range(n)]


@torch.no_grad()
def render_path(model, cameras: Sequence, pipe, bg: torch.Tensor, *, alpha: bool = False, depth: bool = False, residency: str = "host",
                out: Optional[FrameWriter] = None, on_render: Optional[Callable] = None, scaling_modifier: float = 1.0) -> dict:
    """Renders every camera of ``cameras`` (one image size, else ValueError) and returns
    {"frames": uint8 [N, H, W, 3] -- [N, H, W, 4] with ``alpha=True``, the fourth byte the rendered alpha --, "views": N} and, with
    ``depth=True``, "depth": uint8 [N, H, W, 1], the reference's grey depth image (``fdgs.frames.encode_gray``).  The quantisation is
    ``(v * 255 + 0.5).clamp(0, 255).to(uint8)`` (torchvision's ``save_image``), so ``FrameStore(result["frames"])`` decodes to within
    half a step of the clamped render.  ``residency``: "host" (pinned memory) or "device".  ``out``: a ``FrameWriter`` of N frames of
    this shape to write the colour frames through (its ring and its pinned tensor are then reused from call to call); default: a new
    one.  ``on_render(i, results)``: called with view i's ``render_raw`` dict on the render stream before the encode -- the hook for
    metrics; clone what must outlive the call.  No host synchronisation before the end."""
    from .fused import render_raw
    N = len(cameras)
    if N == 0:
        raise ValueError("fdgs.playback.render_path: no cameras")
    sizes = {(int(c.image_height), int(c.image_width)) for c in cameras}
    if len(sizes) != 1:
        raise ValueError("fdgs.playback.render_path: all cameras of a path must share one image size, got %s" % sorted(sizes))
    (H, W), C = next(iter(sizes)), 4 if alpha else 3
    dev = bg.device
    if out is None:
        out = FrameWriter(N, H, W, channels=C, residency=residency, device=dev)
    elif not isinstance(out, FrameWriter) or (len(out), out.shape) != (N, (H, W, C)):
        raise ValueError("fdgs.playback.render_path: out must be a FrameWriter of %d frames %s" % (N, (H, W, C)))
    grey = FrameWriter(N, H, W, channels=1, residency=residency, device=dev) if depth else None
    for i, cam in enumerate(cameras):
        results = render_raw(cam, model, pipe, bg, scaling_modifier=scaling_modifier)
        if on_render is not None:
            on_render(i, results)
        out.write(i, results["render"], results["alpha"] if alpha else None)
        if grey is not None:
            grey.write_gray(i, results["depth"])
    res = {"frames": out.finish(), "views": N}
    if grey is not None:
        res["depth"] = grey.finish()
    return res
