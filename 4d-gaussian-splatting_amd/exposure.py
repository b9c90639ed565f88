"""Per-camera colour correction on the GPU (csrc/exposure.hip, include/fdgs_exposure.h).

The cameras of a multi-camera rig differ in exposure and white balance.  Each training camera gets a learned affine colour transform
``A = [M | o]`` (3 x 4, a row of 12 floats of one device table), applied to the render before the loss; held-out views are aligned
to their ground truth in closed form before the metrics.

* ``ExposureModel``      -- the table ``[num_cameras, 12]`` (identity at the start), its Adam moments and per-camera step counts;
  ``step(indices, slots)`` is one launch that updates the rows a step's views name and nothing else.
* ``apply``              -- ``M c + o`` per pixel, differentiable in the image and in the table (``torch.autograd``): what a
  hand-written loop around ``render()`` / ``render_raw()`` calls.  ``apply_`` / ``backward_`` are the raw launches on the current
  stream (``StepPipeline(exposure=)``).
* ``fit_affine``         -- the ridge-regularised least-squares transform of a render onto its ground truth: the moments on the GPU
  in float64 in a fixed order, the 4 x 4 solve on the host.  One host read.
* ``evaluate_corrected`` -- ``metrics.evaluate``'s numbers, raw and (``_cc``) after ``fit_affine`` + ``apply`` per view.

Every sum is float64 in a fixed order without atomics: two runs give the same bits.  There is no CPU path.
"""
from typing import Sequence

import numpy as np
import torch

from . import _capi, _exposure_capi

MAX_VIEWS = _exposure_capi.EXPOSURE_MAX_VIEWS
_p = _capi._ptr
_PARTIALS = {}


def _image(t, name):
    _capi.need_gpu(t, name)
    if t.dim() != 3 or t.shape[0] != 3 or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError("fdgs.exposure: '%s' must be a contiguous float32 tensor [3, H, W]; got %s %s" % (name, tuple(t.shape), t.dtype))
    return t


def _table(t):
    """The device table [N, 12] of an ``ExposureModel``, a table tensor, or one row [12] as a table of one camera."""
    t = t.table if isinstance(t, ExposureModel) else t
    _capi.need_gpu(t, "table")
    t = t.detach()
    if t.dim() == 1:
        t = t.view(1, -1)
    if t.dim() != 2 or t.shape[1] != 12 or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError("fdgs.exposure: the table must be a contiguous float32 tensor [num_cameras, 12]; got %s %s" % (tuple(t.shape), t.dtype))
    return t


def _partials(dev, doubles):
    """Device scratch of the two reductions: one buffer per (device, stream), grown to the largest size asked for (the calls are
    stream-ordered on that stream, so the next one may reuse it at once)."""
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    buf = _PARTIALS.get(key)
    if buf is None or buf.numel() < 8 * doubles:
        buf = _PARTIALS[key] = _capi.scratch(8 * doubles, dev, floor=256)
    return buf


def apply_(image: torch.Tensor, table, index: int, out: torch.Tensor = None) -> torch.Tensor:
    """``M c + o`` of row ``index`` of ``table`` for every pixel of ``image`` [3, H, W] into ``out`` (default: in place) on the
    current stream."""
    image, tab = _image(image, "image"), _table(table)
    out = image if out is None else _image(out, "out")
    H, W = int(image.shape[1]), int(image.shape[2])
    if out.shape != image.shape:
        raise ValueError("fdgs.exposure: out is %s, the image %s" % (tuple(out.shape), tuple(image.shape)))
    _exposure_capi.call("fdgs_exposure_apply", image.device, H, W, _p(image), _p(tab), int(tab.shape[0]), int(index), _p(out), arg_error=ValueError)
    return out


def backward_(g: torch.Tensor, image: torch.Tensor, table, index: int, slot: torch.Tensor, out: torch.Tensor = None, accumulate: bool = False,
              image_grad: bool = True) -> torch.Tensor:
    """The backward of ``apply_`` on the current stream, one pass: ``g`` [3, H, W] is the gradient of the corrected image, ``image``
    the UNCORRECTED one.  ``M^T g`` goes into ``out`` (default: in place into ``g``; ``image_grad=False``: not computed) and the 12
    sums ``dA`` into ``slot`` (any contiguous float32 view of 12 elements; written, or added with ``accumulate``).  Returns ``out``."""
    g, image, tab = _image(g, "g"), _image(image, "image"), _table(table)
    _capi.need_gpu(slot, "slot")
    if slot.dtype != torch.float32 or slot.numel() != 12 or not slot.is_contiguous():
        raise ValueError("fdgs.exposure: slot must be a contiguous float32 tensor of 12 elements")
    if g.shape != image.shape:
        raise ValueError("fdgs.exposure: the gradient is %s, the image %s" % (tuple(g.shape), tuple(image.shape)))
    out = None if not image_grad else (g if out is None else _image(out, "out"))
    H, W, dev = int(image.shape[1]), int(image.shape[2]), image.device
    parts = _partials(dev, int(_exposure_capi.lib.fdgs_exposure_num_partials(H, W)))
    _exposure_capi.call("fdgs_exposure_backward", dev, H, W, _p(g), _p(image), _p(tab), int(tab.shape[0]), int(index), _p(out), _p(parts), _p(slot),
                        int(bool(accumulate)), arg_error=ValueError)
    return out


class ExposureModel:
    """One affine colour transform per training camera and its own Adam (``torch.optim.Adam(lr, betas, eps)``'s formula with a step
    count per camera: a camera that is not in a step keeps its row, its moments and its count bit for bit).

    ``table`` [N, 12] float32 starts as ``[I | 0]``; ``exp_avg`` / ``exp_avg_sq`` [N, 12] float32 and ``steps`` [N] int32 start at zero."""

    def __init__(self, num_cameras: int, device, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-15):
        if int(num_cameras) < 1:
            raise ValueError("fdgs.exposure: num_cameras must be at least 1, got %d" % int(num_cameras))
        self.num_cameras = int(num_cameras)
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        row = torch.tensor([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=torch.float32)
        _capi.need_gpu(torch.empty(0, device=device), "table", what="the exposure table")
        self.table = row.repeat(self.num_cameras, 1).to(device).contiguous()
        self.exp_avg = torch.zeros_like(self.table)
        self.exp_avg_sq = torch.zeros_like(self.table)
        self.steps = torch.zeros(self.num_cameras, dtype=torch.int32, device=device)

    @property
    def device(self):
        return self.table.device

    def index_of(self, cam) -> int:
        """The row of a camera: its ``uid``."""
        uid = getattr(cam, "uid", None)
        if uid is None or not 0 <= int(uid) < self.num_cameras:
            raise ValueError("fdgs.exposure: camera uid %r is not a row of a table of %d cameras" % (uid, self.num_cameras))
        return int(uid)

    def row(self, index: int) -> torch.Tensor:
        return self.table[int(index)]

    def step(self, indices: Sequence[int], slots: torch.Tensor):
        """One Adam step of the rows ``indices`` names (one per view of the step, a camera may come twice) with the views' gradient
        slots ``slots`` [B, 12] (``backward_``'s), on the current stream; one launch, no host wait."""
        _capi.need_gpu(slots, "slots")
        B = len(indices)
        if slots.dtype != torch.float32 or not slots.is_contiguous() or tuple(slots.shape) != (B, 12):
            raise ValueError("fdgs.exposure: slots must be a contiguous float32 tensor [%d, 12]; got %s %s" % (B, tuple(slots.shape), slots.dtype))
        _exposure_capi.call("fdgs_exposure_adam", self.table.device, self.num_cameras, _p(self.table), _p(self.exp_avg), _p(self.exp_avg_sq),
                            _p(self.steps), B, _p(slots), _exposure_capi.host_ints(indices), self.lr, self.betas[0], self.betas[1], self.eps,
                            arg_error=ValueError)

    def state_dict(self) -> dict:
        """Plain tensors (on the host) and floats: stored next to a ``fdgs.checkpoint`` file, whose own layout does not change."""
        return {"table": self.table.cpu().clone(), "exp_avg": self.exp_avg.cpu().clone(), "exp_avg_sq": self.exp_avg_sq.cpu().clone(),
                "steps": self.steps.cpu().clone(), "lr": self.lr, "beta1": self.betas[0], "beta2": self.betas[1], "eps": self.eps}

    def load_state_dict(self, state: dict):
        if tuple(state["table"].shape) != (self.num_cameras, 12):
            raise ValueError("fdgs.exposure: the state holds %s, this model %s" % (tuple(state["table"].shape), (self.num_cameras, 12)))
        for name in ("table", "exp_avg", "exp_avg_sq", "steps"):
            getattr(self, name).copy_(state[name].to(getattr(self, name).dtype))
        self.lr, self.betas, self.eps = float(state["lr"]), (float(state["beta1"]), float(state["beta2"])), float(state["eps"])


class _Apply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, table, index):
        _capi.need_gpu(image, "image")
        c = image.detach().contiguous().float()
        tab = _table(table)
        out = apply_(c, tab, index, out=torch.empty_like(c))
        ctx.save_for_backward(c, tab)
        ctx.index, ctx.table_shape = int(index), table.shape
        return out

    @staticmethod
    def backward(ctx, g):
        c, tab = ctx.saved_tensors
        need_i, need_t = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_i or need_t):
            return None, None, None
        g = g.contiguous().float()
        g_tab = torch.zeros_like(tab)
        g_img = backward_(g, c, tab, ctx.index, g_tab[ctx.index], out=torch.empty_like(g) if need_i else None, image_grad=need_i)
        return g_img, g_tab.view(ctx.table_shape) if need_t else None, None


def apply(image: torch.Tensor, model, index: int) -> torch.Tensor:
    """The corrected image ``M c + o`` of camera ``index``; ``model``: an ``ExposureModel`` or a table tensor [N, 12].
    Differentiable in the image and in the table (the gradient of the table is zero outside row ``index``)."""
    return _Apply.apply(image, model.table if isinstance(model, ExposureModel) else model, int(index))


def fit_moments(image: torch.Tensor, gt: torch.Tensor, clamp: bool = True) -> torch.Tensor:
    """The 22 float64 moments of ``fdgs_colour_fit_moments`` of a render against its ground truth, on the GPU; no host wait."""
    image, gt = _image(image.detach(), "image"), _image(gt.detach(), "gt")
    if gt.shape != image.shape or gt.device != image.device:
        raise ValueError("fdgs.exposure: the ground truth is %s on %s, the image %s on %s" % (tuple(gt.shape), gt.device, tuple(image.shape), image.device))
    H, W, dev = int(image.shape[1]), int(image.shape[2]), image.device
    out = torch.empty(22, dtype=torch.float64, device=dev)
    parts = _partials(dev, int(_exposure_capi.lib.fdgs_colour_fit_num_partials(H, W)))
    _exposure_capi.call("fdgs_colour_fit_moments", dev, H, W, _p(image), _p(gt), int(bool(clamp)), _p(parts), _p(out), arg_error=ValueError)
    return out


def solve_affine(moments, n: int, ridge: float = 1e-6) -> np.ndarray:
    """``A = (N / n + ridge [I | 0]) (M / n + ridge I)^-1`` in float64 on the host from the 22 moments: [12]."""
    m = np.asarray(moments, np.float64)
    M = np.zeros((4, 4))
    M[np.triu_indices(4)] = m[:10]
    M = M + np.triu(M, 1).T
    N = m[10:].reshape(3, 4)
    lhs = M / n + ridge * np.eye(4)
    rhs = N / n + ridge * np.eye(3, 4)
    return np.linalg.solve(lhs, rhs.T).T.reshape(12)   # (lhs is symmetric)


def fit_affine(image: torch.Tensor, gt: torch.Tensor, ridge: float = 1e-6, clamp: bool = True) -> torch.Tensor:
    """The affine colour transform that takes ``image`` (clamped to [0, 1] first with ``clamp``, as ``metrics.evaluate`` clamps) closest
    to ``gt`` in the least-squares sense, pulled towards the identity by ``ridge`` (so a constant image has an answer too): a float32
    [12] row on the image's device.  One host read: evaluation only."""
    m = fit_moments(image, gt, clamp).cpu().numpy()
    A = solve_affine(m, int(image.shape[1]) * int(image.shape[2]), ridge)
    return torch.from_numpy(A).to(image.device, torch.float32)


@torch.no_grad()
def evaluate_corrected(model, cameras, gts, pipe, bg: torch.Tensor, msssim: bool = True) -> dict:
    """``metrics.evaluate``'s dictionary computed twice: on the clamped renders as they are ("l1", "psnr", "ssim", "msssim", "rows")
    and after each view's clamped render went through its own ``fit_affine`` + ``apply_`` ("l1_cc", ... "rows_cc"); "fits": the views'
    rows [V, 12] (on the host), "views": V."""
    from .fused import render_raw
    from .metrics import image_metrics
    V = len(cameras)
    if V == 0 or len(gts) != V:
        raise ValueError("fdgs.exposure.evaluate_corrected: need one ground truth per camera (got %d cameras, %d images)" % (V, len(gts)))
    dev = bg.device
    rows = torch.empty((2, V, 4), dtype=torch.float32, device=dev)
    fits = torch.empty((V, 12), dtype=torch.float32, device=dev)
    for v in range(V):
        image = render_raw(cameras[v], model, pipe, bg)["render"].detach().float().clamp(0.0, 1.0).contiguous()
        gt = gts[v].detach().to(dev, torch.float32).contiguous()
        image_metrics(image, gt, clamp=True, msssim=msssim, out=rows[0, v])
        fits[v] = fit_affine(image, gt, clamp=False)
        image_metrics(apply_(image, fits, v), gt, clamp=True, msssim=msssim, out=rows[1, v])
    host = rows.cpu()
    out = {"views": V, "fits": fits.cpu()}
    for tag, block in (("", host[0]), ("_cc", host[1])):
        sums = [0.0, 0.0, 0.0, 0.0]
        for r in block.double().tolist():
            for k in range(4):
                sums[k] += r[k]
        for k, name in enumerate(("l1", "psnr", "ssim", "msssim")):
            out[name + tag] = sums[k] / V
        out["rows" + tag] = block
    return out
