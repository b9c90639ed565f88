"""float64 torch statement of the environment-map composite (gaussian_renderer/__init__.py:165-177, scene/cameras.py:75-82):
rays, sphere intersection, texture coordinates, the bilinear zero-padded lookup written out by hand (not F.grid_sample: the host
tests compare the two), the composite and -- through autograd -- its gradients.  One deliberate difference from the reference:
z / R is clamped to [-1, 1] before the acos (csrc/envmap.hip takes the equal atan2(sqrt(x^2 + y^2), z), which cannot leave [0, pi])."""
import math

import torch

F64 = torch.float64


def rays(world_view_transform, camera_center, fl_x, fl_y, cx, cy, H, W):
    """(origin [3], unit directions [H, W, 3]) of the pixel centres, as Camera.get_rays."""
    vm = torch.as_tensor(world_view_transform).to(F64).cpu()
    o = torch.as_tensor(camera_center).to(F64).cpu().reshape(3)
    j, i = torch.meshgrid(torch.arange(H, dtype=F64) + 0.5, torch.arange(W, dtype=F64) + 0.5, indexing="ij")
    one = torch.ones_like(i)
    pts = torch.stack([(i - cx) / fl_x, (j - cy) / fl_y, one, one], -1)
    c2w = torch.linalg.inv(vm.transpose(0, 1))
    d = (pts @ c2w.T)[..., :3] - o
    return o, d / torch.norm(d, dim=-1, keepdim=True)


def intersect(o, d, R=60.0):
    """The point where the ray leaves the sphere, with the reference's operator precedence."""
    od, dd, oo = (o * d).sum(-1), (d * d).sum(-1), (o * o).sum(-1)
    delta = od ** 2 - dd * (oo - R ** 2)
    t = -od + torch.sqrt(delta) / dd
    return o + d * t.unsqueeze(-1)


def texcoord(x, R=60.0):
    """(u, v) in [0, 1]: u = atan2(y, x) / 2pi + 0.5, v = acos(clamp(z / R)) / pi."""
    u = torch.atan2(x[..., 1], x[..., 0]) / (2 * math.pi) + 0.5
    v = torch.acos((x[..., 2] / R).clamp(-1.0, 1.0)) / math.pi
    return u, v


def bilinear(env, u, v):
    """grid_sample(env[None], grid = (u, v) * 2 - 1, bilinear, zeros, align_corners=False)[0], written out: [3, H, W]."""
    C, eh, ew = env.shape
    ix = ((u * 2 - 1 + 1) * ew - 1) / 2
    iy = ((v * 2 - 1 + 1) * eh - 1) / 2
    x0, y0 = torch.floor(ix), torch.floor(iy)
    out = torch.zeros((C,) + tuple(u.shape), dtype=env.dtype)
    flat = env.reshape(C, -1)
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        xk, yk = x0 + dx, y0 + dy
        w = (1 - (ix - xk).abs()) * (1 - (iy - yk).abs())
        ok = (xk >= 0) & (xk < ew) & (yk >= 0) & (yk < eh)
        idx = (yk.clamp(0, eh - 1) * ew + xk.clamp(0, ew - 1)).long()
        out = out + torch.where(ok, w, torch.zeros_like(w)) * flat[:, idx.reshape(-1)].reshape((C,) + tuple(u.shape))
    return out


def cam_rays(cam, H, W):
    return rays(cam.world_view_transform, cam.camera_center, float(cam.fl_x), float(cam.fl_y), float(cam.cx), float(cam.cy), H, W)


def lookup(cam, env, H, W, R=60.0):
    """env(ray) [3, H, W] and the flags of the pixels within 1e-4 R of the seam or 1e-3 R of the pole axis [H, W]."""
    o, d = cam_rays(cam, H, W)
    x = intersect(o, d, R)
    u, v = texcoord(x, R)
    seam = (x[..., 1].abs() < 1e-4 * R) & (x[..., 0] < 0)
    pole = torch.sqrt(x[..., 0] ** 2 + x[..., 1] ** 2) < 1e-3 * R
    return bilinear(env, u, v), seam | pole


def composite(colour, alpha, env, cam, R=60.0):
    """colour + (1 - alpha) * env(ray), float64, differentiable in colour, alpha and env.  Returns (image, flags)."""
    H, W = colour.shape[-2:]
    e, flags = lookup(cam, env, H, W, R)
    return colour + (1 - alpha) * e, flags


def composite_grads(colour, alpha, env, cam, g, R=60.0):
    """(d <g, composite> / d alpha, d / d env) in float64 through autograd."""
    a = alpha.detach().to(F64).cpu().requires_grad_(True)
    e = env.detach().to(F64).cpu().requires_grad_(True)
    out, _ = composite(colour.detach().to(F64).cpu(), a, e, cam, R)
    (out * g.detach().to(F64).cpu()).sum().backward()
    return a.grad, e.grad


class PlainCamera:
    """What the composite reads of a camera: world_view_transform, camera_center, fl_x, fl_y, cx, cy."""

    def __init__(self, world_view_transform, camera_center, fl_x, fl_y, cx, cy):
        self.world_view_transform, self.camera_center = world_view_transform, camera_center
        self.fl_x, self.fl_y, self.cx, self.cy = fl_x, fl_y, cx, cy

    def to(self, dev):
        return PlainCamera(self.world_view_transform.to(dev), self.camera_center.to(dev), self.fl_x, self.fl_y, self.cx, self.cy)


def camera(pose, W, H):
    """A PlainCamera of fdgs.synth.camera_for(pose) with its pinhole intrinsics (centre-shift principal point where the pose has one)."""
    from fdgs import synth
    kw = dict(synth.POSES[pose] if isinstance(pose, str) else pose)
    off = kw.pop("principal_off", None)
    c = synth.camera_for(pose, W, H)
    focal = W / (2.0 * c["tanfovx"])
    cx, cy = (0.5 * W, 0.5 * H) if off is None else (0.5 * W + off[0], 0.5 * H + off[1])
    return PlainCamera(c["world_view_transform"], c["camera_center"], focal, focal, cx, cy)


# the poses of the tests: "axis" looks at the +z pole and crosses the atan2 seam; the DyNeRF-like rigs; one looking along the
# equator (+y); one with the seam (direction -x) in mid-image
POSES = {
    "axis": "axis",
    "rig1": "rig1",
    "rig2": "rig2",
    "equator": dict(pitch=-math.pi / 2, shift=(0.3, -0.2, 4.0)),
    "seam": dict(yaw=-math.pi / 2, pitch=-math.pi / 2, shift=(0.2, 0.1, 4.0), principal_off=(7.5, -3.25)),
}
