"""Evaluation metrics on the GPU (csrc/metrics.hip): L1, PSNR, SSIM and MS-SSIM of a render against its ground truth.

The reference's ``training_report`` (train.py:276-345) renders every test camera and five training cameras and computes, on
``clamp(render, 0, 1)``, ``l1_loss``, ``psnr``, ``ssim`` (utils/loss_utils.py, utils/image_utils.py) and torchmetrics'
``MultiScaleStructuralSimilarityIndexMeasure(data_range=1.0)`` -- the last one on the CPU.  Here one kernel per scale and one
reduction write the four numbers of a view into a row of device memory; ``evaluate`` fills one row per view and reads them back
once.  There is no CPU path: CPU tensors raise.  ``tests/metrics_oracle.py`` is the float64 statement of the four definitions.
"""
import torch

from . import _capi

CLAMP, NO_MSSSIM = 1, 2   # include/fdgs.h: FDGS_METRICS_CLAMP, FDGS_METRICS_NO_MSSSIM
MIN_SIDE = 176            # five scales of an 11-tap window: H // 16 > 10 and W // 16 > 10

_SCRATCH = {}


def _scratch(dev, Cn, H, W):
    """Device scratch of fdgs_eval_metrics: one buffer per (device, stream), grown to the largest size asked for.  The calls are
    stream-ordered on that stream, so the next call may reuse it at once; a buffer that is replaced stays alive until the work
    queued on the stream before it is done (the caching allocator's stream semantics)."""
    nbytes = _capi.lib.fdgs_eval_metrics_scratch_bytes(Cn, H, W)
    if nbytes < 0:
        raise ValueError("fdgs.metrics: invalid image shape %s" % ((Cn, H, W),))
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    buf = _SCRATCH.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = _SCRATCH[key] = _capi.scratch(nbytes, dev, floor=256)
    return buf


def _check_msssim_size(H, W):
    # torchmetrics 0.11.4 (functional/image/ssim.py, _multiscale_ssim_update): five betas, an 11-tap window
    if H // 16 <= 10:
        raise ValueError("For a given number of `betas` parameters 5 and kernel size 11, the image height must be larger than 160.")
    if W // 16 <= 10:
        raise ValueError("For a given number of `betas` parameters 5 and kernel size 11, the image width must be larger than 160.")


def image_metrics(img: torch.Tensor, gt: torch.Tensor, clamp: bool = True, msssim: bool = True, out: torch.Tensor = None) -> torch.Tensor:
    """``[l1, psnr, ssim, msssim]`` of one view as a float32 [4] tensor on the GPU (``out`` if given: any contiguous float32 [4]
    view, e.g. a row of a [V, 4] buffer).  ``img``, ``gt``: [C, H, W] (C >= 1).  ``clamp``: clamp ``img`` to [0, 1] first, as the
    reference's evaluation does (``gt`` is used as it is).  ``msssim=False``: ``out[3]`` = NaN and any size is allowed; otherwise
    both sides must be at least 176 pixels (ValueError, torchmetrics' wording).  No host synchronisation."""
    if not img.is_cuda or not gt.is_cuda:
        raise RuntimeError("fdgs: image_metrics needs GPU tensors; there is no CPU path")
    if img.dim() != 3 or tuple(gt.shape) != tuple(img.shape):
        raise ValueError("fdgs.metrics: img and gt must both be [C, H, W], got %s and %s" % (tuple(img.shape), tuple(gt.shape)))
    Cn, H, W = (int(s) for s in img.shape)
    if msssim:
        _check_msssim_size(H, W)
    dev = img.device
    a = img.detach().contiguous().float()
    b = gt.detach().to(dev).contiguous().float()
    if out is None:
        out = torch.empty(4, dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or out.numel() != 4 or not out.is_contiguous() or out.device != dev:
        raise ValueError("fdgs.metrics: out must be a contiguous float32 tensor of 4 elements on %s" % dev)
    flags = (CLAMP if clamp else 0) | (0 if msssim else NO_MSSSIM)
    scratch = _scratch(dev, Cn, H, W)
    _capi.call("fdgs_eval_metrics", dev, a.data_ptr(), b.data_ptr(), Cn, H, W, flags, scratch.data_ptr(), out.data_ptr(), arg_error=ValueError)
    return out


def psnr(img: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """utils/image_utils.py:17-19 reduced as training_report does (``psnr(...).mean()``): the mean over channels of
    20 log10(1 / sqrt(mse_c)); a 0-d GPU tensor.  No clamp (the reference's function does not clamp)."""
    return image_metrics(img, gt, clamp=False, msssim=False)[1]


def ssim(img: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """utils/loss_utils.py:34-66 (11x11 Gaussian window, sigma 1.5, zero padding, mean over pixels and channels); 0-d GPU tensor."""
    return image_metrics(img, gt, clamp=False, msssim=False)[2]


def msssim(img: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """torchmetrics' MultiScaleStructuralSimilarityIndexMeasure(data_range=1.0) of one image pair (utils/loss_utils.py:68-73);
    0-d GPU tensor.  Both sides must be at least 176 pixels."""
    return image_metrics(img, gt, clamp=False, msssim=True)[3]


@torch.no_grad()
def evaluate(model, cameras, gts, pipe, bg: torch.Tensor, msssim: bool = True) -> dict:
    """training_report's inner loop (train.py:311-334) for one set of views: a forward-only ``render_raw`` of every camera (with
    the environment-map composite when ``pipe.env_map_res`` is set), then ``image_metrics`` of the clamped render against ``gts[i]``
    into row i of one [V, 4] device buffer, read back once at the end.  Returns the per-view means accumulated in float64 in view
    order (train.py:327-334) under "l1", "psnr", "ssim", "msssim" (NaN with ``msssim=False``), "views": V, and "rows": the
    per-view [V, 4] float32 tensor (on the host) in the order l1, psnr, ssim, msssim."""
    from .fused import render_raw
    V = len(cameras)
    if V == 0 or len(gts) != V:
        raise ValueError("fdgs.metrics.evaluate: need one ground truth per camera (got %d cameras, %d images)" % (V, len(gts)))
    dev = bg.device
    rows = torch.empty((V, 4), dtype=torch.float32, device=dev)
    for v in range(V):
        image = render_raw(cameras[v], model, pipe, bg)["render"]
        image_metrics(image, gts[v], clamp=True, msssim=msssim, out=rows[v])
    host = rows.cpu()
    sums = [0.0, 0.0, 0.0, 0.0]
    for r in host.double().tolist():
        for k in range(4):
            sums[k] += r[k]
    return {"l1": sums[0] / V, "psnr": sums[1] / V, "ssim": sums[2] / V, "msssim": sums[3] / V, "views": V, "rows": host}
