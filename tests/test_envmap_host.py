"""CPU: the float64 statement of the environment-map composite (tests/envmap_oracle.py) against the reference's own rays
(tests/golden/envmap/rays.npz, from scene/cameras.py's get_rays) and against F.grid_sample."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import envmap_oracle as eo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "envmap", "rays.npz")


@pytest.mark.parametrize("name", ["front", "rig", "equator"])
def test_rays_match_the_reference_camera(name):
    z = np.load(GOLDEN)
    dirs = z[name + "_dirs"]
    H, W = dirs.shape[:2]
    fx, fy, cx, cy = z[name + "_intrinsics"]
    o, d = eo.rays(torch.from_numpy(z[name + "_world_view_transform"]), torch.from_numpy(z[name + "_camera_center"]), fx, fy, cx, cy, H, W)
    assert np.abs(o.numpy() - z[name + "_origin"]).max() <= 1e-6
    err = np.abs(d.numpy() - dirs).max()
    assert err <= 2e-6, err
    # the rays fan out over the image: a transposed or mirrored convention would not match at the corners
    assert np.abs(dirs[0, 0] - dirs[-1, -1]).max() > 0.5


def _grid(u, v):
    return torch.stack([u, v], -1) * 2 - 1


@pytest.mark.parametrize("shape", [(3, 40, 72), (3, 17, 31), (3, 64, 64)])
def test_bilinear_is_grid_sample(shape):
    g = torch.Generator().manual_seed(shape[1])
    env = torch.rand(shape, generator=g, dtype=torch.float64)
    # the whole range and a margin beyond it (zero padding), and the edges exactly
    u = torch.cat([torch.rand(3000, generator=g, dtype=torch.float64) * 1.2 - 0.1, torch.tensor([0.0, 1.0, 0.5, 1e-9, 1 - 1e-9], dtype=torch.float64)])
    v = torch.cat([torch.rand(3000, generator=g, dtype=torch.float64) * 1.2 - 0.1, torch.tensor([0.0, 1.0, 1e-9, 0.5, 1.0], dtype=torch.float64)])
    want = F.grid_sample(env[None], _grid(u, v)[None, None], mode="bilinear", padding_mode="zeros", align_corners=False)[0][:, 0]
    got = eo.bilinear(env, u, v)
    assert torch.allclose(got, want, atol=1e-12, rtol=0)


def test_bilinear_gradient_is_grid_sample_gradient():
    g = torch.Generator().manual_seed(5)
    env = torch.rand(3, 40, 72, generator=g, dtype=torch.float64)
    u, v = torch.rand(500, generator=g, dtype=torch.float64), torch.rand(500, generator=g, dtype=torch.float64)
    w = torch.randn(3, 500, generator=g, dtype=torch.float64)
    e1 = env.clone().requires_grad_(True)
    (eo.bilinear(e1, u, v) * w).sum().backward()
    e2 = env.clone().requires_grad_(True)
    (F.grid_sample(e2[None], _grid(u, v)[None, None], align_corners=False)[0][:, 0] * w).sum().backward()
    assert torch.allclose(e1.grad, e2.grad, atol=1e-12, rtol=0)


def test_seam_does_not_wrap():
    """u = 0 and u = 1 (atan2 = -pi / +pi) sample half of the first / last column and half of the zero padding, not the other side."""
    env = torch.zeros(3, 8, 16, dtype=torch.float64)
    env[:, :, 0] = 1.0
    env[:, :, -1] = 2.0
    v = torch.full((2,), (3 + 0.5) / 8, dtype=torch.float64)   # a texel-row centre
    got = eo.bilinear(env, torch.tensor([0.0, 1.0], dtype=torch.float64), v)
    assert torch.allclose(got, torch.tensor([[0.5, 1.0]] * 3, dtype=torch.float64))


def test_pole_clamp_and_intersection():
    """Looking straight up the z axis from the centre: z / R can round above 1; the clamp keeps v = 0 finite.  Off-centre origins:
    the intersection lies on the sphere."""
    x = torch.tensor([[0.0, 0.0, 60.0 * (1 + 1e-15)]], dtype=torch.float64)
    u, v = eo.texcoord(x)
    assert torch.isfinite(v).all() and float(v) == 0.0
    g = torch.Generator().manual_seed(1)
    o = torch.tensor([0.7, -0.45, -4.3], dtype=torch.float64)
    d = torch.randn(200, 3, generator=g, dtype=torch.float64)
    d = d / d.norm(dim=-1, keepdim=True)
    p = eo.intersect(o, d)
    assert torch.allclose(p.norm(dim=-1), torch.full((200,), 60.0, dtype=torch.float64), atol=1e-9)
    assert ((p - o) * d).sum(-1).min() > 0      # in front of the camera


def test_composite_gradients():
    """d / d alpha = -<g, env>, d / d env = the transposed lookup of g (1 - alpha): the autograd gradients of the oracle."""
    W, H = 24, 16
    cam = eo.PlainCamera(torch.eye(4), torch.zeros(3), 20.0, 20.0, 12.0, 8.0)
    g = torch.Generator().manual_seed(2)
    env = torch.rand(3, 10, 20, generator=g, dtype=torch.float64)
    colour = torch.rand(3, H, W, generator=g, dtype=torch.float64)
    alpha = torch.rand(1, H, W, generator=g, dtype=torch.float64)
    up = torch.randn(3, H, W, generator=g, dtype=torch.float64)
    ga, ge = eo.composite_grads(colour, alpha, env, cam, up)
    e, _ = eo.lookup(cam, env, H, W)
    assert torch.allclose(ga, -(up * e).sum(0, keepdim=True))
    e2 = env.clone().requires_grad_(True)
    o, d = eo.cam_rays(cam, H, W)
    u, v = eo.texcoord(eo.intersect(o, d))
    (F.grid_sample(e2[None], _grid(u, v)[None], align_corners=False)[0] * (1 - alpha) * up).sum().backward()
    assert torch.allclose(ge, e2.grad, atol=1e-12)
