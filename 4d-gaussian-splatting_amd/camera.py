"""Cameras under optimisation: ``LearnableCamera`` refines a view's pose and time offset through the rasterizer.

Multi-view video rigs come with poses that are a fraction of a pixel off and per-camera clocks that are a fraction of a frame off; a 4D
model turns both into blur.  ``LearnableCamera(base_cam)`` wraps any camera object ``render()`` / ``render_raw()`` take and exposes
``world_view_transform``, ``full_proj_transform``, ``camera_center`` and ``timestamp`` as differentiable torch expressions of two
parameters; the rasterizer returns dL/d(those tensors) (fdgs_camera_backward, csrc/camera_bwd.hip) and autograd chains them to

  ``pose_delta`` [6] = (omega, u): an se(3) twist, applied on the left of the world-to-view transform, V' = exp(xi) V;
  ``time_offset`` [1]: added to the base camera's timestamp.

Matrices are held as the reference holds them (scene/cameras.py:65-71): transposed, row-vector convention -- ``world_view_transform`` =
V^T, ``full_proj_transform`` = V^T P^T.  Every property is the base camera's tensor plus a correction that is exactly zero at zero
delta, so an unrefined LearnableCamera renders what its base camera renders, bit for bit.
"""
import torch
import torch.nn as nn


def _hat(w):
    z = torch.zeros((), dtype=w.dtype, device=w.device)
    return torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])


def se3_exp_minus_identity(xi):
    """exp(xi) - I of the twist xi = (omega, u) as (R - I [3,3], t [3]):  R = I + A K + B K^2,  t = (I + B K + C K^2) u  with K = hat(omega),
    A = sin th / th, B = (1 - cos th) / th^2, C = (th - sin th) / th^3.  Near th = 0 the coefficients come from their series in th^2 --
    polynomials in omega, so the gradient at zero is finite and exact; R - I is formed without subtracting the identity."""
    w, u = xi[:3], xi[3:]
    th2 = (w * w).sum()
    small = th2 < (1e-6 if xi.dtype == torch.float32 else 1e-8)
    th2s = torch.where(small, torch.ones_like(th2), th2)   # the closed forms are evaluated away from 0 (their branch is masked there)
    th = torch.sqrt(th2s)
    A = torch.where(small, 1.0 - th2 / 6.0 + th2 * th2 / 120.0, torch.sin(th) / th)
    B = torch.where(small, 0.5 - th2 / 24.0 + th2 * th2 / 720.0, (1.0 - torch.cos(th)) / th2s)
    Cc = torch.where(small, 1.0 / 6.0 - th2 / 120.0 + th2 * th2 / 5040.0, (th - torch.sin(th)) / (th2s * th))
    K = _hat(w)
    K2 = K @ K
    return A * K + B * K2, u + B * (K @ u) + Cc * (K2 @ u)


def apply_twist(world_view_transform, xi):
    """(exp(xi) V)^T for V^T = ``world_view_transform``, as V^T + V^T (exp(xi)^T - I): equal to V^T bit for bit at xi = 0."""
    dR, t = se3_exp_minus_identity(xi)
    D = torch.cat([torch.cat([dR.T, torch.zeros(3, 1, dtype=xi.dtype, device=xi.device)], dim=1),
                   torch.cat([t, torch.zeros(1, dtype=xi.dtype, device=xi.device)]).reshape(1, 4)], dim=0)
    return world_view_transform + world_view_transform @ D


def centre_of(world_view_transform):
    """The camera centre -R^T t of a world-to-view transform held transposed (rows 0-2: R^T, row 3: t): no inverse()."""
    return -(world_view_transform[:3, :3] @ world_view_transform[3, :3])


class LearnableCamera(nn.Module):
    """``base_cam`` with a refinable pose and time offset; everything else (image size, field of view, image, ...) is the base camera's."""

    def __init__(self, base_cam):
        super().__init__()
        object.__setattr__(self, "_base", base_cam)   # not a submodule, not in the state dict
        V = base_cam.world_view_transform
        self.pose_delta = nn.Parameter(torch.zeros(6, dtype=V.dtype, device=V.device))
        self.time_offset = nn.Parameter(torch.zeros(1, dtype=V.dtype, device=V.device))
        # the base projection P^T (transposed layout) with V^T P^T = full_proj_transform: the base camera's own where it has one
        # (scene/cameras.py:66-68), otherwise solved for in double
        proj = getattr(base_cam, "projection_matrix", None)
        if proj is None:
            proj = torch.linalg.solve(V.detach().double(), base_cam.full_proj_transform.detach().double()).to(V.dtype)
        self.register_buffer("_proj", proj.detach().clone(), persistent=False)

    @property
    def base(self):
        return self._base

    @property
    def world_view_transform(self):
        return apply_twist(self._base.world_view_transform.detach(), self.pose_delta)

    @property
    def full_proj_transform(self):
        V = self._base.world_view_transform.detach()
        return self._base.full_proj_transform.detach() + (self.world_view_transform - V) @ self._proj

    @property
    def camera_center(self):
        V = self._base.world_view_transform.detach()
        return self._base.camera_center.detach() + (centre_of(self.world_view_transform) - centre_of(V))

    @property
    def timestamp(self):
        """0-d tensor: base timestamp + time_offset."""
        t = self._base.timestamp
        t = t.detach().to(self.time_offset) if isinstance(t, torch.Tensor) else torch.as_tensor(float(t), dtype=self.time_offset.dtype, device=self.time_offset.device)
        return (t + self.time_offset).reshape(())

    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            return getattr(object.__getattribute__(self, "_base"), name)
