"""Optical flow of a 4D model: how far every Gaussian moves on the screen between two views (csrc/flow.hip).

``gaussian_flow(cam, cam_to, ...)`` returns, per Gaussian, ``pix(mu(cam_to.timestamp); cam_to) - pix(mu(cam.timestamp); cam)`` in
pixels, where ``mu(t)`` is the mean as the rasterizer's preprocess has it at time ``t`` (``rot_4d``: the conditional mean
``p + Sigma[0:3,3] / Sigma[3,3] (t - t_i)``; otherwise the plain mean, so the flow is the camera's alone and exactly 0 with one
camera) and ``pix`` is the preprocess's own projection: for a Gaussian the forward keeps in both views the flow equals the difference
of its two screen positions bit for bit.  A Gaussian behind either camera's near plane (view-space z <= 0.2) has flow 0 and no
gradient.  This is what the rasterizer's ``flow_2d`` input takes: ``render(..., flow_to=cam_to)`` / ``render_raw(..., flow_to=cam_to)``
feed it and return the blended image ``sum_i flow_i alpha_i T_i`` as ``"flow"`` (not divided by alpha).

Differentiable: the backward kernel is the analytic gradient with respect to the six tensors as passed (``raw=True``: through exp and
the quaternion normalisation).  One launch each way, no atomics, bitwise reproducible.  The cameras are constants.
"""
import ctypes as C

import torch

from . import _capi, layout


def _flow_in(cam, cam_to, tensors, rot_4d, gaussian_dim, raw, scaling_modifier):
    """fdgs_flow_in for the six contiguous float32 device tensors (None where absent) + what must stay alive during the call."""
    means3D = tensors[0]
    dev = means3D.device
    W, H = int(cam.image_width), int(cam.image_height)
    if (int(cam_to.image_width), int(cam_to.image_height)) != (W, H):
        raise ValueError("fdgs.flow.gaussian_flow: both cameras must share one image size, got %dx%d and %dx%d" % (
            W, H, int(cam_to.image_width), int(cam_to.image_height)))
    f = _capi._dev_f32
    vm, pm = f(cam.world_view_transform.to(dev), "world_view_transform"), f(cam.full_proj_transform.to(dev), "full_proj_transform")
    same = cam_to.world_view_transform is cam.world_view_transform and cam_to.full_proj_transform is cam.full_proj_transform
    vm_to = None if same else f(cam_to.world_view_transform.to(dev), "world_view_transform")
    pm_to = None if same else f(cam_to.full_proj_transform.to(dev), "full_proj_transform")
    p = _capi._ptr
    a = _capi.FdgsFlowIn(int(means3D.shape[0]), W, H, *[p(t) for t in tensors], p(vm), p(pm), p(vm_to), p(pm_to), float(cam.timestamp),
                         float(cam_to.timestamp), float(scaling_modifier), int(bool(rot_4d)), int(gaussian_dim), int(bool(raw)))
    return a, (vm, pm, vm_to, pm_to)


class _GaussianFlow(torch.autograd.Function):
    ARGS = ("means3D", "ts", "scales", "scales_t", "rotations", "rotations_r")   # the kernels' tensors (fdgs_flow_in), by fdgs.layout's kernel names

    @staticmethod
    def forward(ctx, means3D, ts, scales, scales_t, rotations, rotations_r, cam, cam_to, rot_4d, gaussian_dim, raw, scaling_modifier):
        given = (means3D, ts, scales, scales_t, rotations, rotations_r)
        names = _GaussianFlow.ARGS
        _capi.need_gpu(means3D, "means3D")
        # without rot_4d the kernels read the mean only
        tensors = [_capi._dev_f32(t.detach(), n) if (t is not None and (rot_4d or n == "means3D")) else None for t, n in zip(given, names)]
        dev = means3D.device
        P = int(means3D.shape[0])
        flows = torch.empty((P, 2), dtype=torch.float32, device=dev)
        a, keep = _flow_in(cam, cam_to, tensors, rot_4d, gaussian_dim, raw, scaling_modifier)
        _capi.call("fdgs_gaussian_flow_forward", dev, C.byref(a), flows.data_ptr())
        del keep
        ctx.cams, ctx.settings = (cam, cam_to), (rot_4d, gaussian_dim, raw, scaling_modifier)
        ctx.shapes = [None if t is None else t.shape for t in given]
        ctx.present = [t is not None for t in tensors]
        ctx.save_for_backward(*[t for t in tensors if t is not None])
        return flows

    @staticmethod
    def backward(ctx, dL_dflows):
        saved = list(ctx.saved_tensors)
        tensors = [saved.pop(0) if here else None for here in ctx.present]
        dev = tensors[0].device
        rot_4d, gaussian_dim, raw, scaling_modifier = ctx.settings
        # the kernel ADDS: zeroed buffers for the inputs autograd asks about (without rot_4d only the mean has a gradient)
        grads = [torch.zeros(t.shape, dtype=torch.float32, device=dev) if (t is not None and need) else None
                 for t, need in zip(tensors, ctx.needs_input_grad[:6])]
        if any(g is not None for g in grads):
            g_in = _capi._dev_f32(dL_dflows, "dL_dflows")
            a, keep = _flow_in(ctx.cams[0], ctx.cams[1], tensors, rot_4d, gaussian_dim, raw, scaling_modifier)
            out = _capi.FdgsFlowGrads(*[_capi._ptr(g) for g in grads])
            _capi.call("fdgs_gaussian_flow_backward", dev, C.byref(a), g_in.data_ptr(), 1.0, C.byref(out))
            del keep
        shaped = [None if g is None else g.reshape(s) for g, s in zip(grads, ctx.shapes)]
        return tuple(shaped) + (None,) * 6


def gaussian_flow(cam, cam_to, means3D, ts, scales, scales_t, rotations, rotations_r, *, rot_4d, gaussian_dim, raw, scaling_modifier=1.0):
    """[P, 2] float32: the screen motion of every Gaussian from ``cam`` (at ``cam.timestamp``) to ``cam_to`` (at ``cam_to.timestamp``), in
    pixels; see the module docstring.  ``cam_to``: any camera object of the same image size (``world_view_transform``,
    ``full_proj_transform``, ``timestamp``); ``fdgs.playback.with_timestamp(cam, t1)`` is the fixed-camera case.  ``raw``: scales /
    scales_t / rotations / rotations_r are the model's raw parameters (the kernels apply exp and the normalisation), else the
    activated values; ``scaling_modifier`` as in ``render()``.  Without ``rot_4d`` only ``means3D`` is read (the others may be None)."""
    if int(means3D.shape[0]) == 0:
        return torch.zeros((0, 2), dtype=torch.float32, device=means3D.device)
    return _GaussianFlow.apply(means3D, ts, scales, scales_t, rotations, rotations_r, cam, cam_to, bool(rot_4d), int(gaussian_dim), bool(raw),
                               float(scaling_modifier))


def model_flow(cam, cam_to, pc, *, raw, scaling_modifier=1.0):
    """``gaussian_flow`` of a reference-style model ``pc``: its raw parameters (``raw=True``, what ``render_raw`` feeds) or its activated
    getters (``raw=False``, what ``render`` feeds: autograd continues through them)."""
    rot_4d = bool(pc.rot_4d) and int(pc.gaussian_dim) == 4
    if not rot_4d:
        return gaussian_flow(cam, cam_to, pc._xyz if raw else pc.get_xyz, None, None, None, None, None, rot_4d=False,
                             gaussian_dim=int(pc.gaussian_dim), raw=raw, scaling_modifier=scaling_modifier)
    t = [getattr(pc, layout.BY_KERNEL[k].name if raw else "get" + layout.BY_KERNEL[k].name) for k in _GaussianFlow.ARGS]
    return gaussian_flow(cam, cam_to, *t, rot_4d=True, gaussian_dim=4, raw=raw, scaling_modifier=scaling_modifier)
