"""GPU: the environment-map composite (csrc/envmap.hip through fdgs.envmap) against the float64 statement of
tests/envmap_oracle.py, and render_raw with pipe.env_map_res against the drop-in render()."""
import math

import numpy as np
import pytest
import torch

import envmap_oracle as eo
from util import synth

pytestmark = pytest.mark.gpu


def smooth_env(eh, ew, seed, dev):
    """A smooth map (a few low harmonics in both texel directions): the bars below bound the arithmetic, not fp32's rounding of
    the texture coordinate times the texel-to-texel jumps of a noise map."""
    g = torch.Generator().manual_seed(seed)
    y = (torch.arange(eh, dtype=torch.float64) + 0.5) / eh
    x = (torch.arange(ew, dtype=torch.float64) + 0.5) / ew
    env = torch.empty(3, eh, ew, dtype=torch.float64)
    for c in range(3):
        a = torch.rand(4, generator=g, dtype=torch.float64)
        env[c] = 0.5 + 0.2 * a[0] * torch.sin(2 * math.pi * (x[None, :] + a[1])) + 0.2 * a[2] * torch.cos(math.pi * (2 * y[:, None] + a[3]))
    return env.float().to(dev)


def _case(dev, pose, W, H, eh, ew, seed=0):
    cam = eo.camera(eo.POSES[pose], W, H).to(dev)
    g = torch.Generator().manual_seed(seed + 11)
    colour = torch.rand(3, H, W, generator=g).to(dev)
    alpha = (torch.rand(1, H, W, generator=g) * 0.9).to(dev)
    up = torch.randn(3, H, W, generator=g).to(dev)
    return cam, colour, alpha, up, smooth_env(eh, ew, seed, dev)


def _check(dev, pose, W, H, eh, ew):
    from fdgs.envmap import env_composite
    cam, colour, alpha, up, env = _case(dev, pose, W, H, eh, ew)
    c = colour.clone().requires_grad_(True)
    a = alpha.clone().requires_grad_(True)
    e = env.clone().requires_grad_(True)
    out = env_composite(c, a, e, cam)
    want, flags = eo.composite(colour.double().cpu(), alpha.double().cpu(), env.double().cpu(), cam)
    assert torch.isfinite(out).all()
    ok = ~flags
    assert flags.float().mean().item() <= 0.01, flags.float().mean().item()
    err = (out.detach().double().cpu() - want).abs()[:, ok]
    assert err.max().item() <= 1e-5, (pose, err.max().item())
    assert ((1 - alpha.cpu()) * (want - colour.double().cpu())).abs().max() > 0.05   # the map is visible
    # gradients: the upstream gradient is zero on flagged pixels (a tap across the seam moves the contribution to the far side)
    upm = up * ok.to(dev)
    (out * upm).sum().backward()
    ga, ge = eo.composite_grads(colour, alpha, env, cam, upm.cpu())
    assert torch.isfinite(a.grad).all() and torch.isfinite(e.grad).all()
    assert torch.equal(c.grad, upm)
    gerr = (a.grad.double().cpu() - ga).abs().max().item()
    assert gerr <= 1e-5 * ga.abs().max().item(), (pose, gerr, ga.abs().max().item())
    eerr = (e.grad.double().cpu() - ge).abs().max().item()
    assert eerr <= 1e-4 * ge.abs().max().item(), (pose, eerr, ge.abs().max().item())
    return cam, env


@pytest.mark.parametrize("pose", list(eo.POSES))
@pytest.mark.parametrize("size", [(40, 72), (500, 500)], ids=["40x72", "500x500"])
def test_composite_matches_float64(gpu_device, pose, size):
    _check(gpu_device, pose, 208, 160, *size)


@pytest.mark.parametrize("pose", ["axis", "equator"])
def test_composite_full_size(gpu_device, pose):
    """C3's image (1352 x 1014, focal 0.9 W) with a 500^2 map: the pole-facing rig puts hundreds of longitude texels under the
    central tiles (the wide-window fall-back), the equator-facing one a few texels under every tile."""
    _check(gpu_device, pose, 1352, 1014, 500, 500)


def test_accumulate_and_partial_outputs(gpu_device):
    """fdgs_env_composite_backward: g_alpha / g_env added with accumulate_*, either one alone, colour_out aliasing colour_in."""
    from fdgs import envmap
    cam, colour, alpha, up, env = _case(gpu_device, "rig2", 96, 80, 40, 72)
    T = (1 - alpha).contiguous()
    ga, ge = torch.empty_like(alpha), torch.empty_like(env)
    envmap.composite_backward(T, up, env, cam, ga, False, ge, False)
    ga2, ge2 = torch.full_like(alpha, 0.5), torch.full_like(env, 0.25)
    envmap.composite_backward(T, up, env, cam, ga2, True, None, False)
    envmap.composite_backward(T, up, env, cam, None, False, ge2, True)
    torch.cuda.synchronize()
    assert torch.allclose(ga2, ga + 0.5, atol=1e-6) and torch.allclose(ge2, ge + 0.25, atol=1e-5)
    c = colour.clone()
    out = envmap.composite_(c, T, env, cam)
    assert out.data_ptr() == c.data_ptr()
    want = envmap.composite_(colour, T, env, cam, out=torch.empty_like(colour))
    assert torch.equal(c, want)


def test_camera_outside_the_sphere(gpu_device):
    from fdgs.envmap import env_composite
    cam = eo.camera(dict(shift=(0.0, 0.0, 70.0)), 64, 48).to(gpu_device)
    env = smooth_env(8, 16, 0, gpu_device)
    with pytest.raises(ValueError, match="inside its sphere"):
        env_composite(torch.zeros(3, 48, 64, device=gpu_device), torch.zeros(1, 48, 64, device=gpu_device), env, cam)


class _EnvPipe:
    compute_cov3D_python = False
    convert_SHs_python = False
    debug = False
    env_map_res = 40


@pytest.mark.parametrize("pose", ["axis", "rig2"])
def test_render_raw_with_env_map_matches_render(gpu_device, pose):
    """render_raw with pipe.env_map_res (black background, HIP composite) against the drop-in render()'s own composite
    (gaussian_renderer._finish: grid_sample through autograd) applied to render_raw's image over black: image, raw-parameter gradients
    (test_gpu_api's 1e-4 of the tensor scale) and the map's gradient.  (The same rasterization on both sides: render() itself takes
    torch's activations, which move a few pixels by more than the bars; test_gpu_render_branches pins its composite.)"""
    from fdgs import train_host
    from fdgs.fused import render_raw
    from fdgs.gaussian_renderer import _finish
    cfg = synth.SceneConfig("env", 4000, 208, 160, 3, 2, 0.03, 10.0, True, 4, False)
    scene = synth.make_scene(cfg, seed=6, pose=pose)
    bg = torch.tensor([0.9, 0.8, 0.7], device=gpu_device)        # ignored by the environment-map path
    cam = train_host.SyntheticCamera(scene, gpu_device)
    model = train_host.GaussianParams(scene, gpu_device)
    model.env_map = smooth_env(40, 72, 3, gpu_device).requires_grad_(True)
    # the drop-in's fp32 acos(z / R) loses ~sqrt(eps) of v near the pole (the HIP path works in float64 there): the pixels within
    # 0.05 R of the pole axis are left out of the comparison (no upstream gradient, image not compared)
    o, d = eo.cam_rays(cam, scene["H"], scene["W"])
    x = eo.intersect(o, d)
    far = (torch.sqrt(x[..., 0] ** 2 + x[..., 1] ** 2) >= 0.05 * 60.0).to(gpu_device)
    assert far.float().mean().item() >= 0.95
    up = torch.randn(3, scene["H"], scene["W"], generator=torch.Generator().manual_seed(2)).to(gpu_device) * 1e-2 * far
    runs = {}
    for name in ("torch", "raw"):
        model.zero_grad()
        model.env_map.grad = None
        if name == "raw":
            img = render_raw(cam, model, _EnvPipe(), bg)["render"]
        else:
            out = render_raw(cam, model, train_host.PipelineFlags(), torch.zeros(3, device=gpu_device))
            black = out["render"].detach().clone()
            img = _finish(cam, model, _EnvPipe(), out["viewspace_points"], out["render"], out["radii"], out["depth"], out["alpha"],
                          out["flow"], None)["render"]
        (img * up).sum().backward()
        torch.cuda.synchronize()
        runs[name] = (img.detach().clone(), model.flat_grad.clone(), model.env_map.grad.clone())
    img_err = (runs["raw"][0] - runs["torch"][0]).abs()[:, far].max().item()
    assert img_err <= 1e-5, img_err
    assert (runs["torch"][0] - black).abs().max() > 0.05, "the environment is invisible: the case does not test it"
    for n in model.NAMES:
        b, e = model.offsets[n]
        g, w = runs["raw"][1][b:e], runs["torch"][1][b:e]
        scale = max(1.0, w.abs().max().item())
        assert (g - w).abs().max().item() <= 1e-4 * scale, (n, (g - w).abs().max().item(), scale)
    ge, we = runs["raw"][2], runs["torch"][2]
    assert (ge - we).abs().max().item() <= 1e-4 * we.abs().max().item()
