"""Fused photometric loss (1 - lambda) L1 + lambda (1 - SSIM) on the GPU (csrc/ssim.hip).

Drop-in for the reference's ``(1.0 - opt.lambda_dssim) * l1_loss(image, gt) + opt.lambda_dssim * (1.0 - ssim(image, gt))``
(train.py:115-117, utils/loss_utils.py:17-64).  One forward kernel and one backward kernel instead of five
grouped 11x11 convolutions and their autograd graph.  ``gt`` is treated as a constant (no gradient), as in
training.  There is no CPU path: CPU tensors raise.  ``fdgs.train_host.photometric_loss`` is the PyTorch
statement of the same loss, used as the reference in the tests.
"""
import os

import torch

from . import _capi


class _FusedL1SSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, gt, lambda_dssim):
        if not img.is_cuda or not gt.is_cuda:
            raise RuntimeError("fdgs: fused_l1_ssim needs GPU tensors; there is no CPU path")
        img_c, gt_c = img.contiguous().float(), gt.contiguous().float()
        C, H, W = img_c.shape[-3], img_c.shape[-2], img_c.shape[-1]
        dev = img_c.device
        d1, d2, d3 = (torch.empty_like(img_c) for _ in range(3))
        nparts = _capi.lib.fdgs_l1_ssim_num_partials(C, H, W)
        parts = torch.empty((2, nparts), dtype=torch.float32, device=dev)
        out = torch.empty(3, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _capi.call("fdgs_l1_ssim_forward", dev, img_c.data_ptr(), gt_c.data_ptr(), C, H, W, d1.data_ptr(), d2.data_ptr(), d3.data_ptr(),
                       parts[0].data_ptr(), parts[1].data_ptr(), guard=False)
            _capi.call("fdgs_l1_ssim_loss", dev, parts[0].data_ptr(), parts[1].data_ptr(), nparts, C, H, W, float(lambda_dssim),
                       out.data_ptr(), guard=False)
        ctx.save_for_backward(img_c, gt_c, d1, d2, d3)
        ctx.lambda_dssim = float(lambda_dssim)
        ctx.shape = img.shape
        return out[0]

    @staticmethod
    def backward(ctx, grad_out):
        img_c, gt_c, d1, d2, d3 = ctx.saved_tensors
        C, H, W = img_c.shape[-3], img_c.shape[-2], img_c.shape[-1]
        dev = img_c.device
        up = grad_out.reshape(1).contiguous().float()
        g = torch.empty_like(img_c)
        _capi.call("fdgs_l1_ssim_backward", dev, img_c.data_ptr(), gt_c.data_ptr(), C, H, W, d1.data_ptr(), d2.data_ptr(), d3.data_ptr(),
                   up.data_ptr(), ctx.lambda_dssim, g.data_ptr())
        return g.view(ctx.shape), None, None


def fused_l1_ssim(image: torch.Tensor, gt: torch.Tensor, lambda_dssim: float = 0.2) -> torch.Tensor:
    """(1 - lambda) * L1(image, gt) + lambda * (1 - SSIM(image, gt)); image, gt: [3, H, W] on the GPU."""
    return _FusedL1SSIM.apply(image, gt, lambda_dssim)


# l1_ssim_grad: the forward + backward pair with the three derivative maps in memory (default), or, "fused": True, ONE kernel that
# rebuilds the maps around every tile (fdgs_l1_ssim_value_and_grad: a third of the HBM traffic, 1.7 x the window arithmetic).  Measured
# on MI355X at 3x1014x1352, one stream: pair 64 us, one kernel 76 us; the two-stream C3 step: 2.53 against 2.56 ms -- the pair stays
# the default (FDGS_SSIM_FUSED=1 in the environment selects the one-kernel form at import).
ssim_options = {"fused": os.environ.get("FDGS_SSIM_FUSED", "0") == "1"}


def l1_ssim_grad(image: torch.Tensor, gt: torch.Tensor, lambda_dssim: float, upstream: torch.Tensor, parts: torch.Tensor = None):
    """Value and gradient kernels only: returns ``(d(upstream * loss)/d image, handle)``; ``l1_ssim_loss(handle)`` reduces
    the per-tile partial sums to the loss value later (e.g. after the rasterizer backward has been enqueued, so that the
    small reduction is off the critical path).  ``parts``: a [2, num_partials] float32 slice to leave the partial sums in (a row of
    ``partials_buffer``: ``l1_ssim_loss_batch`` then reduces all views of a step in one launch)."""
    if not image.is_cuda or not gt.is_cuda:
        raise RuntimeError("fdgs: l1_ssim_grad needs GPU tensors; there is no CPU path")
    img_c, gt_c = image.contiguous().float(), gt.contiguous().float()
    C, H, W = img_c.shape[-3], img_c.shape[-2], img_c.shape[-1]
    dev = img_c.device
    nparts = _capi.lib.fdgs_l1_ssim_num_partials(C, H, W)
    if parts is None:
        parts = torch.empty((2, nparts), dtype=torch.float32, device=dev)
    elif tuple(parts.shape) != (2, nparts) or not parts.is_contiguous() or parts.dtype != torch.float32:
        raise RuntimeError("fdgs: parts must be a contiguous float32 [2, %d] tensor" % nparts)
    if ssim_options["fused"]:
        g = torch.empty_like(img_c)
        _capi.call("fdgs_l1_ssim_value_and_grad", dev, img_c.data_ptr(), gt_c.data_ptr(), C, H, W, upstream.data_ptr(), float(lambda_dssim),
                   g.data_ptr(), parts[0].data_ptr(), parts[1].data_ptr())
        return g, (parts, nparts, C, H, W, float(lambda_dssim))
    d1, d2, d3, g = (torch.empty_like(img_c) for _ in range(4))
    with torch.cuda.device(dev):   # one guard and one stream look-up for the pair: this runs once per view of a training step
        st = _capi.current_stream_handle(dev)
        _capi.call("fdgs_l1_ssim_forward", dev, img_c.data_ptr(), gt_c.data_ptr(), C, H, W, d1.data_ptr(), d2.data_ptr(), d3.data_ptr(),
                   parts[0].data_ptr(), parts[1].data_ptr(), guard=False, stream=st)
        _capi.call("fdgs_l1_ssim_backward", dev, img_c.data_ptr(), gt_c.data_ptr(), C, H, W, d1.data_ptr(), d2.data_ptr(), d3.data_ptr(),
                   upstream.data_ptr(), float(lambda_dssim), g.data_ptr(), guard=False, stream=st)
    return g, (parts, nparts, C, H, W, float(lambda_dssim))


def l1_ssim_loss(handle) -> torch.Tensor:
    """Loss value of a ``l1_ssim_grad`` call (deterministic reduction kernel, current stream)."""
    parts, nparts, C, H, W, lam = handle
    dev = parts.device
    out = torch.empty(3, dtype=torch.float32, device=dev)
    _capi.call("fdgs_l1_ssim_loss", dev, parts[0].data_ptr(), parts[1].data_ptr(), nparts, C, H, W, lam, out.data_ptr())
    return out[0]


def partials_buffer(num_views: int, C: int, H: int, W: int, device) -> torch.Tensor:
    """[num_views, 2, num_partials]: one row per view for ``l1_ssim_grad(parts=buffer[v])``."""
    return torch.empty((num_views, 2, _capi.lib.fdgs_l1_ssim_num_partials(C, H, W)), dtype=torch.float32, device=device)


def l1_ssim_loss_batch(buffer: torch.Tensor, handles) -> list:
    """The loss values of the ``l1_ssim_grad`` calls that left their partial sums in rows 0 .. len(handles) - 1 of ``buffer``: ONE
    launch (a workgroup per view) instead of one per view; bit-identical to ``l1_ssim_loss`` per handle.  Returns a list of 0-d tensors."""
    n = len(handles)
    _parts, nparts, C, H, W, lam = handles[0]
    dev = buffer.device
    out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    _capi.call("fdgs_l1_ssim_loss_batch", dev, buffer.data_ptr(), n, nparts, C, H, W, lam, out.data_ptr())
    return [out[v, 0] for v in range(n)]


def l1_ssim_value_and_grad(image: torch.Tensor, gt: torch.Tensor, lambda_dssim: float, upstream: torch.Tensor):
    """The same loss without autograd: returns ``(loss, d(upstream * loss)/d image)``.  ``upstream`` is a 1-element
    float32 GPU tensor (e.g. 1 / batch_size).  All kernels are enqueued on the current stream."""
    g, handle = l1_ssim_grad(image, gt, lambda_dssim, upstream)
    return l1_ssim_loss(handle), g


# ---- the reference trainer's other loss terms (train.py:119-159) ----

class _RigidMotion(torch.autograd.Function):
    """(L_rigid, L_motion) from the raw parameters: k-NN of the means, velocities and both values in the forward
    (fdgs_knn_query + fdgs_rigid_motion_forward), one fused backward weighted by both upstream scalars."""

    @staticmethod
    def forward(ctx, scaling, scaling_t, rotation, rotation_r, t, xyz, k):
        from .knn import knn
        dev = scaling.device
        P = int(scaling.shape[0])
        ins = [v.detach().contiguous().float() for v in (scaling, scaling_t, rotation, rotation_r, t)]
        idx, d2 = knn(xyz.detach()[None], xyz.detach()[None], k)
        velocity = torch.empty((P, 3), dtype=torch.float32, device=dev)
        losses = torch.empty(2, dtype=torch.float32, device=dev)
        scratch = _capi.scratch(_capi.lib.fdgs_rigid_motion_scratch_bytes(P, k), dev)
        _capi.call("fdgs_rigid_motion_forward", dev, P, k, *[v.data_ptr() for v in ins], idx.data_ptr(), d2.data_ptr(), velocity.data_ptr(),
                   losses.data_ptr(), scratch.data_ptr())
        ctx.save_for_backward(*ins, idx, d2, velocity)
        ctx.k, ctx.scratch = k, scratch
        ctx.mark_non_differentiable(velocity)
        return losses[0], losses[1], velocity

    @staticmethod
    def backward(ctx, g_rigid, g_motion, _g_velocity):
        scaling, scaling_t, rotation, rotation_r, t, idx, d2, velocity = ctx.saved_tensors
        dev, P = scaling.device, int(scaling.shape[0])
        zero = torch.zeros((), dtype=torch.float32, device=dev)
        g = torch.stack([zero if g_rigid is None else g_rigid.float().reshape(()),
                         zero if g_motion is None else g_motion.float().reshape(())])
        outs = [torch.zeros_like(v) for v in (scaling, scaling_t, rotation, rotation_r)]
        _capi.call("fdgs_rigid_motion_backward", dev, P, ctx.k, scaling.data_ptr(), scaling_t.data_ptr(), rotation.data_ptr(),
                   rotation_r.data_ptr(), t.data_ptr(), idx.data_ptr(), d2.data_ptr(), velocity.data_ptr(), g.data_ptr(), 1.0,
                   *[o.data_ptr() for o in outs], ctx.scratch.data_ptr())
        return outs[0], outs[1], outs[2], outs[3], None, None, None


def rigid_motion_loss(pc, k: int = 20):
    """``(L_rigid, L_motion)`` of the reference trainer (train.py:130-159), both differentiable, on the GPU.

    ``pc``: anything with the reference model's attribute names (``_xyz``, ``_scaling``, ``_scaling_t``, ``_rotation``,
    ``_rotation_r``, ``_t``, ``rot_4d``, ``gaussian_dim``): ``GaussianParams``, ``ReferenceStyleModel`` or the reference's own
    ``GaussianModel``.  The velocity is the 4D conditional mean shift over dt = (t + 0.1) - t; L_rigid uses the k nearest means
    (``fdgs.knn.knn``, itself included at distance 0):  sum exp(-100 d2) |v_nbr - v_i| / k / P;  L_motion = mean |v|.
    Gradients reach ``_scaling / _scaling_t / _rotation / _rotation_r``; the means, t and the neighbour search get none, as in the
    reference.  Needs ``rot_4d`` and ``gaussian_dim == 4`` (the reference has no velocity otherwise)."""
    if not getattr(pc, "rot_4d", False) or int(getattr(pc, "gaussian_dim", 3)) != 4:
        raise ValueError("fdgs: rigid_motion_loss needs a rot_4d model with gaussian_dim == 4 (the velocity is the 4D conditional "
                         "mean shift); got rot_4d=%s, gaussian_dim=%s" % (getattr(pc, "rot_4d", None), getattr(pc, "gaussian_dim", None)))
    xyz = pc.get_xyz
    if not xyz.is_cuda:
        raise RuntimeError("fdgs: rigid_motion_loss needs GPU tensors; there is no CPU path")
    if int(xyz.shape[0]) == 0:
        raise ValueError("fdgs: rigid_motion_loss of a model without Gaussians")
    l_rigid, l_motion, _ = _RigidMotion.apply(pc._scaling, pc._scaling_t, pc._rotation, pc._rotation_r, pc.get_t, xyz, int(k))
    return l_rigid, l_motion


class _OpaMask(torch.autograd.Function):
    """Value and d L / d alpha in ONE pass in the forward (the gradient is linear in the upstream scalar: the backward scales it)."""

    @staticmethod
    def forward(ctx, alpha, mask):
        if not alpha.is_cuda or not mask.is_cuda:
            raise RuntimeError("fdgs: opa_mask_loss needs GPU tensors; there is no CPU path")
        if alpha.numel() != mask.numel() or alpha.shape[-2:] != mask.shape[-2:]:
            raise ValueError("fdgs: opa_mask_loss expects alpha and gt_alpha_mask of one [1, H, W] shape; got %s and %s"
                             % (tuple(alpha.shape), tuple(mask.shape)))
        a, m = alpha.detach().contiguous().float(), mask.detach().contiguous().float()
        H, W, dev = int(alpha.shape[-2]), int(alpha.shape[-1]), alpha.device
        parts = torch.empty(max(1, _capi.lib.fdgs_opa_mask_num_partials(H, W)), dtype=torch.float32, device=dev)
        out = torch.empty(1, dtype=torch.float32, device=dev)
        g = torch.empty_like(a) if alpha.requires_grad else None
        _capi.call("fdgs_opa_mask_loss", dev, H, W, a.data_ptr(), 0, m.data_ptr(), None, 1.0, _capi._ptr(g), 0, parts.data_ptr(), out.data_ptr())
        ctx.save_for_backward(g)
        ctx.shape = alpha.shape
        return out[0]

    @staticmethod
    def backward(ctx, grad_out):
        g, = ctx.saved_tensors
        return (g * grad_out.float()).view(ctx.shape), None


def opa_mask_loss(alpha: torch.Tensor, gt_alpha_mask: torch.Tensor) -> torch.Tensor:
    """The reference trainer's opacity-mask loss (train.py:120-128), one kernel each way:
    ``o = alpha.clamp(1e-6, 1 - 1e-6); mean(-(1 - gt_alpha_mask) * log(1 - o))``.  ``alpha``: ``render()``'s ``"alpha"`` [1, H, W];
    its gradient flows back through the rasterizer's alpha path.  The mask is a constant."""
    return _OpaMask.apply(alpha, gt_alpha_mask)
