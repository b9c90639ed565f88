"""Depth supervision on the rendered depth map, on the GPU (csrc/depth_loss.hip).

Every forward writes ``depth = sum_i z_i alpha_i T_i`` next to ``alpha = 1 - T`` and every backward takes a gradient for both; this
module produces such gradients from a depth prior (a monocular network, a sensor, multi-view stereo):

* ``depth_loss(depth, alpha, prior, mask, mode="pearson" | "ssi")`` -- ``1 - rho(z, prior)``, or the scale-and-shift-invariant L1
  ``sum |s z + b - prior| / n`` with ``(s, b)`` the least-squares alignment, over the valid pixels;
* ``depth_normals(depth, alpha, intrinsics, mask, viewmatrix=None)`` -- the normal map of the rendered depth and its validity, with
  the backward to ``depth`` and ``alpha``; ``normal_loss(normals, valid, prior_normals)`` compares it with a normal prior;
* ``intrinsics_of(cam)`` -- ``(fl_x, fl_y, cx, cy)`` of a camera, pixel centres at +0.5.

The per-pixel depth is ``z = depth / alpha`` where ``alpha >= alpha_min`` (``alpha=None``: ``z = depth``, every pixel passes).  A
pixel is valid if it passes that test, ``mask`` is None or ``> 0`` there, and -- for ``depth_loss`` -- the prior is finite and ``> 0``.
Invalid pixels contribute nothing and receive exactly 0 gradient.  All kernels run on the current stream and nothing waits for the
device: values stay device scalars.  No atomics: two runs on one input are bit-identical.  There is no CPU path.
"""
import ctypes as C

import torch

from . import _capi

MODES = {"pearson": _capi.FDGS_DEPTH_PEARSON, "ssi": _capi.FDGS_DEPTH_SSI}


def _plane(t, name, like=None):
    """A [1, H, W] (or [H, W]) image as a detached contiguous float32 GPU tensor; None stays None."""
    if t is None:
        return None
    _capi.need_gpu(t, name)
    if like is not None and (t.numel() != like.numel() or t.shape[-2:] != like.shape[-2:]):
        raise ValueError("fdgs: '%s' must have the depth's [1, H, W] shape %s; got %s" % (name, tuple(like.shape), tuple(t.shape)))
    return t.detach().contiguous().float()


def _depth_in(d, a, m, alpha_min):
    if d.dim() < 2 or d.numel() != d.shape[-2] * d.shape[-1]:
        raise ValueError("fdgs: depth must be one [1, H, W] image; got %s" % (tuple(d.shape),))
    return _capi.FdgsDepthIn(int(d.shape[-2]), int(d.shape[-1]), d.data_ptr(), _capi._ptr(a), _capi._ptr(m), float(alpha_min))


class _DepthLoss(torch.autograd.Function):
    """Value and gradient in the forward (the gradient is linear in the upstream scalar: the backward scales it), as _OpaMask."""

    @staticmethod
    def forward(ctx, depth, alpha, prior, mask, mode, alpha_min, stats_out):
        if mode not in MODES:
            raise ValueError("fdgs: depth_loss mode must be 'pearson' or 'ssi'; got %r" % (mode,))
        d = _plane(depth, "depth")
        a, p, m = _plane(alpha, "alpha", d), _plane(prior, "prior", d), _plane(mask, "mask", d)
        if p is None:
            raise ValueError("fdgs: depth_loss needs a prior")
        dev = d.device
        din = _depth_in(d, a, m, alpha_min)
        need_d = depth.requires_grad
        need_a = alpha is not None and alpha.requires_grad
        g_d = torch.empty_like(d) if need_d else None
        g_a = torch.empty_like(a) if need_a else None
        grads = _capi.FdgsDepthGrads(_capi._ptr(g_d), _capi._ptr(g_a), None, 1.0, 0) if (need_d or need_a) else None
        parts = torch.empty(_capi.lib.fdgs_depth_loss_num_partials(din.H, din.W), dtype=torch.float64, device=dev)
        out = torch.empty(4, dtype=torch.float32, device=dev)
        _capi.call("fdgs_depth_loss", dev, C.byref(din), p.data_ptr(), MODES[mode], None if grads is None else C.byref(grads),
                   parts.data_ptr(), out.data_ptr())
        ctx.save_for_backward(g_d, g_a)
        ctx.shapes = (depth.shape, None if alpha is None else alpha.shape)
        ctx.dtypes = (depth.dtype, None if alpha is None else alpha.dtype)
        if stats_out is not None:
            stats_out.append(out[1:])
        return out[0]

    @staticmethod
    def backward(ctx, grad_out):
        g_d, g_a = ctx.saved_tensors
        up = grad_out.float()
        gd = None if g_d is None else (g_d * up).view(ctx.shapes[0]).to(ctx.dtypes[0])
        ga = None if g_a is None else (g_a * up).view(ctx.shapes[1]).to(ctx.dtypes[1])
        return gd, ga, None, None, None, None, None


def depth_loss(depth, alpha, prior, mask=None, mode: str = "pearson", alpha_min: float = 0.5, return_stats: bool = False):
    """A depth-prior loss on ``render()``'s ``"depth"`` and ``"alpha"`` (both [1, H, W]; ``alpha`` may be None), a device scalar.

    ``mode="pearson"``: ``1 - rho(z, prior)``, invariant to any positive affine map of either side.  ``mode="ssi"``:
    ``sum |s z + b - prior| / n`` where ``(s, b) = argmin sum (s z + b - prior)^2`` is computed on the device from the same moments and
    is treated as a CONSTANT for the gradient (the usual detached alignment): ``dL/dz_i = s sign(r_i) / n``.
    Sums run over the valid pixels (module docstring), in float64 and in a fixed order.  Degenerate inputs -- fewer than two valid
    pixels, or a variance of ``z`` or of the prior at or below ``1e-12 max(1, mean^2)`` -- give exactly 1 (pearson) or 0 (ssi) and an
    all-zero gradient, never a NaN.  Gradients reach ``depth`` and ``alpha``; prior and mask are constants.
    ``return_stats=True``: also a [3] float32 device tensor ``(n, rho, 0)`` (pearson) or ``(n, s, b)`` (ssi)."""
    stats = [] if return_stats else None
    loss = _DepthLoss.apply(depth, alpha, prior, mask, mode, float(alpha_min), stats)
    return (loss, stats[0]) if return_stats else loss


def _vm(viewmatrix, dev):
    return None if viewmatrix is None else viewmatrix.detach().to(dev, torch.float32).contiguous()


class _DepthNormals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, alpha, mask, intrinsics, alpha_min, viewmatrix):
        d = _plane(depth, "depth")
        a, m = _plane(alpha, "alpha", d), _plane(mask, "mask", d)
        dev = d.device
        din = _depth_in(d, a, m, alpha_min)
        fx, fy, cx, cy = (float(v) for v in intrinsics)
        vm = _vm(viewmatrix, dev)
        normals = torch.empty((3, din.H, din.W), dtype=torch.float32, device=dev)
        valid = torch.empty((1, din.H, din.W), dtype=torch.uint8, device=dev)
        _capi.call("fdgs_depth_normals", dev, C.byref(din), fx, fy, cx, cy, _capi._ptr(vm), normals.data_ptr(), valid.data_ptr())
        ctx.save_for_backward(d, a, m, vm)
        ctx.intr, ctx.alpha_min = (fx, fy, cx, cy), float(alpha_min)
        ctx.shapes = (depth.shape, None if alpha is None else alpha.shape)
        ctx.dtypes = (depth.dtype, None if alpha is None else alpha.dtype)
        ctx.mark_non_differentiable(valid)
        return normals, valid

    @staticmethod
    def backward(ctx, g_normals, _g_valid):
        d, a, m, vm = ctx.saved_tensors
        need_d, need_a = ctx.needs_input_grad[0], a is not None and ctx.needs_input_grad[1]
        if not (need_d or need_a):
            return None, None, None, None, None, None
        dev = d.device
        g = g_normals.contiguous().float()
        din = _depth_in(d, a, m, ctx.alpha_min)
        g_d = torch.empty_like(d) if need_d else None
        g_a = torch.empty_like(a) if need_a else None
        grads = _capi.FdgsDepthGrads(_capi._ptr(g_d), _capi._ptr(g_a), None, 1.0, 0)
        _capi.call("fdgs_depth_normals_backward", dev, C.byref(din), *ctx.intr, _capi._ptr(vm), g.data_ptr(), C.byref(grads))
        gd = None if g_d is None else g_d.view(ctx.shapes[0]).to(ctx.dtypes[0])
        ga = None if g_a is None else g_a.view(ctx.shapes[1]).to(ctx.dtypes[1])
        return gd, ga, None, None, None, None


def depth_normals(depth, alpha, intrinsics, mask=None, alpha_min: float = 0.5, viewmatrix=None):
    """``(normals [3, H, W], valid [1, H, W] uint8)`` of the rendered depth; differentiable in ``depth`` and ``alpha``.

    ``intrinsics = (fl_x, fl_y, cx, cy)`` (``intrinsics_of(cam)``), pixel centres at +0.5:
    ``P(u, v) = ((u + .5 - cx) / fl_x z, (v + .5 - cy) / fl_y z, z)``, ``a = P(u+1, v) - P(u-1, v)``, ``b = P(u, v+1) - P(u, v-1)``,
    ``n = (b x a) / |b x a|``: towards the camera, ``n_z < 0`` on a fronto-parallel plane.  A normal is valid only if the pixel and its
    four neighbours are inside the image and valid (module docstring) and ``|b x a|^2 > 1e-20``; otherwise ``n = 0``, ``valid = 0``
    and the stencil gets no gradient.  ``viewmatrix``: the camera's ``world_view_transform`` as the rasterizer takes it; given, the
    normals are rotated to world space in the kernel."""
    if not depth.is_cuda:
        raise RuntimeError("fdgs: depth_normals needs GPU tensors; there is no CPU path")
    return _DepthNormals.apply(depth, alpha, mask, tuple(intrinsics), float(alpha_min), viewmatrix)


def normal_loss(normals, valid, prior_normals):
    """``mean over valid of (1 - n . n_prior)``; 0 where no normal is valid.  Plain tensor operations on the normal map (the stencil
    is the kernel-worthy part); no host synchronisation."""
    v = valid.to(normals.dtype)
    return ((1.0 - (normals * prior_normals).sum(-3, keepdim=True)) * v).sum() / v.sum().clamp(min=1.0)


def intrinsics_of(cam):
    """``(fl_x, fl_y, cx, cy)`` in pixels, the quantities ``fdgs_env_composite`` takes (pixel centres at +0.5: a view-space point
    (x, y, z) lands at ``u = fl_x x / z + cx``, ``v = fl_y y / z + cy``, and pixel (i, j) covers [i, i + 1) x [j, j + 1)).

    Read from the projection the rasterizer itself uses -- ``inverse(world_view_transform) @ full_proj_transform`` -- so that a
    camera with the centre-shift projection gets its own principal point: ``fl_x = P[0][0] W / 2``, ``cx = (1 + P[2][0]) W / 2`` and
    likewise in y.  A camera without those matrices must carry ``fl_x / fl_y / cx / cy`` itself, as for ``env_composite``.
    ``cam``: an object with the reference Camera's attribute names or a ``fdgs.synth`` camera / scene dict.  One host read of two
    4 x 4 matrices: call it once per camera, outside the training step."""
    get = (lambda k: cam.get(k)) if isinstance(cam, dict) else (lambda k: getattr(cam, k, None))
    wv, full = get("world_view_transform"), get("full_proj_transform")
    if wv is None or full is None:
        vals = [get(k) for k in ("fl_x", "fl_y", "cx", "cy")]
        if any(v is None for v in vals):
            raise ValueError("fdgs: intrinsics_of needs world_view_transform and full_proj_transform, or fl_x / fl_y / cx / cy")
        return tuple(float(v) for v in vals)
    W, H = int(get("image_width")), int(get("image_height"))
    proj = torch.linalg.solve(wv.detach().double().cpu(), full.detach().double().cpu())
    return (float(proj[0, 0]) * 0.5 * W, float(proj[1, 1]) * 0.5 * H, (1.0 + float(proj[2, 0])) * 0.5 * W,
            (1.0 + float(proj[2, 1])) * 0.5 * H)
