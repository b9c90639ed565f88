"""GPU: StepPipeline with the environment map (pipe.env_map_res > 0) against a reference-style loop -- the drop-in render() (its
PyTorch composite), fused_l1_ssim, autograd, the model's Adam and torch.optim.Adam on the map (train.py:71-77, 250-252) -- and
harness.train learning a map."""
import numpy as np
import pytest
import torch

from util import synth
from test_gpu_envmap import smooth_env

pytestmark = pytest.mark.gpu
ENV = (24, 48)


class EnvPipe:
    compute_cov3D_python = False
    convert_SHs_python = False
    debug = False

    def __init__(self, res):
        self.env_map_res = res


def _setup(dev, B, P=6000, seed=4):
    from fdgs import train_host
    cfg = synth.SceneConfig("envpipe", P, 208, 160, 3, 2, 0.03, 10.0, True, 4, False)
    scene = synth.make_scene(cfg, seed=seed)
    cams = [train_host.SyntheticCamera(scene, dev, timestamp=(b + 0.5) / B * scene["time_duration"]) for b in range(B)]
    gen = torch.Generator(device="cpu").manual_seed(7)
    gts = [torch.rand(3, scene["H"], scene["W"], generator=gen).to(dev) for _ in range(B)]
    masks = [(torch.rand(1, scene["H"], scene["W"], generator=gen) > 0.5).float().to(dev) for _ in range(B)]
    return scene, cams, gts, masks, torch.tensor([0.1, 0.2, 0.3], device=dev)


def _model(scene, dev):
    from fdgs import train_host
    m = train_host.GaussianParams(scene, dev)
    m.env_map = smooth_env(*ENV, 9, dev).requires_grad_(True)
    return m


def _reference(scene, cams, gts, masks, bg, steps=2, lam_opa=0.0):
    from fdgs import train_host
    from fdgs.gaussian_renderer import render
    from fdgs.loss import fused_l1_ssim, opa_mask_loss
    dev = bg.device
    B = len(cams)
    ma = _model(scene, dev)
    oa = train_host.make_optimizer(ma)
    oe = torch.optim.Adam([ma.env_map], lr=2.5e-3, eps=1e-15)
    losses = []
    for _ in range(steps):
        ma.zero_grad()
        for b in range(B):
            pkg = render(cams[b], ma, EnvPipe(ENV[0]), bg)
            l1s = fused_l1_ssim(pkg["render"], gts[b], 0.2)
            loss = l1s + (lam_opa * opa_mask_loss(pkg["alpha"], masks[b]) if lam_opa > 0 else 0.0)
            (loss / B).backward()
            losses.append(float(l1s))
        oa.step()
        oe.step()
        oe.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    return ma, losses


def _pipeline(scene, cams, gts, masks, bg, steps=2, res=ENV[0], mods=None, optimize_env=True, **kw):
    from fdgs import train_host
    from fdgs.pipeline import StepPipeline
    mp = _model(scene, bg.device)
    sp = StepPipeline(mp, train_host.make_optimizer(mp), world_size=1, lambda_dssim=0.2, **kw)
    losses, renders = [], []
    for s in range(steps):
        res_, ls = sp.step(cams, gts, EnvPipe(res), bg, scaling_modifier=1.0 if mods is None else mods[s],
                           alpha_masks=masks if kw.get("lambda_opa_mask", 0) > 0 else None, optimize_env=optimize_env)
        losses += [float(l) for l in ls]
        renders.append([r["render"].clone() for r in res_])
    torch.cuda.synchronize()
    return mp, sp, losses, renders


def _close_params(mp, ma):
    perr = (mp.flat - ma.flat).abs()
    assert (perr > 2e-3).float().mean().item() <= 2e-3 and perr.max().item() <= 0.25, ((perr > 2e-3).float().mean().item(), perr.max().item())
    # the map: Adam moves every texel by ~lr per step whatever its gradient; where the gradient is float-atomics noise its sign may differ
    eerr = (mp.env_map.detach() - ma.env_map.detach()).abs()
    assert (eerr > 1e-3).float().mean().item() <= 0.01 and eerr.max().item() <= 2 * 2.5e-3 * 2 + 1e-6, ((eerr > 1e-3).float().mean().item(), eerr.max().item())


@pytest.mark.parametrize("overlap,fuse,B,group", [(True, True, 3, 1), (False, True, 3, 1), (True, False, 3, 1), (True, True, 1, 1),
                                                  (True, True, 3, 2), (True, False, 3, 2)])
def test_pipeline_with_env_map_matches_autograd(gpu_device, overlap, fuse, B, group):
    scene, cams, gts, masks, bg = _setup(gpu_device, B)
    ma, ref_losses = _reference(scene, cams, gts, masks, bg)
    mp, sp, got_losses, renders = _pipeline(scene, cams, gts, masks, bg, overlap=overlap, fuse_sh_adam=fuse, sh_group=group)
    np.testing.assert_allclose(got_losses, ref_losses, rtol=3e-5, atol=1e-6)
    assert sp.env_opt.step_count == 2
    _close_params(mp, ma)


def test_pipeline_with_env_map_and_opacity_mask(gpu_device):
    """The opacity-mask term and the composite both feed the views' alpha gradient: they add up."""
    B = 3
    scene, cams, gts, masks, bg = _setup(gpu_device, B)
    ma, ref_losses = _reference(scene, cams, gts, masks, bg, lam_opa=0.3)
    mp, _sp, got_losses, _r = _pipeline(scene, cams, gts, masks, bg, lambda_opa_mask=0.3)
    np.testing.assert_allclose(got_losses, ref_losses, rtol=3e-5, atol=1e-6)
    _close_params(mp, ma)


def test_pipeline_with_env_map_overlap_steps(gpu_device):
    B = 3
    scene, cams, gts, masks, bg = _setup(gpu_device, B)
    plain = _pipeline(scene, cams, gts, masks, bg, steps=4)
    over = _pipeline(scene, cams, gts, masks, bg, steps=4, overlap_steps=True)
    assert over[1].overlap_steps and over[1].steps_carried == 3
    np.testing.assert_allclose(over[2], plain[2], rtol=1e-4, atol=1e-6)
    perr = (over[0].flat - plain[0].flat).abs()
    assert (perr > 2e-3).float().mean().item() <= 2e-3 and perr.max().item() <= 0.25
    eerr = (over[0].env_map.detach() - plain[0].env_map.detach()).abs()
    assert (eerr > 1e-3).float().mean().item() <= 0.01


def test_pipeline_with_env_map_lazy_redo(gpu_device):
    """A lazy step redone (scaling_modifier 2.6 after two steps at 1.0) overwrites the map's gradient like the bucket: it equals the
    waiting pipeline."""
    B = 3
    scene, cams, gts, masks, bg = _setup(gpu_device, B, P=6007)
    runs = {lazy: _pipeline(scene, cams, gts, masks, bg, steps=4, mods=(1.0, 1.0, 2.6, 2.6), lazy=lazy) for lazy in (False, True)}
    assert runs[False][1].lazy_redone == 0 and runs[True][1].lazy_redone == 1
    np.testing.assert_allclose(runs[True][2], runs[False][2], rtol=3e-5, atol=1e-6)
    perr = (runs[True][0].flat - runs[False][0].flat).abs()
    assert (perr > 2e-3).float().mean().item() <= 2e-3 and perr.max().item() <= 0.25
    eerr = (runs[True][0].env_map.detach() - runs[False][0].env_map.detach()).abs()
    assert (eerr > 1e-3).float().mean().item() <= 0.01


def test_optimize_env_false_keeps_the_map(gpu_device):
    B = 3
    scene, cams, gts, masks, bg = _setup(gpu_device, B)
    mp, sp, _l, renders = _pipeline(scene, cams, gts, masks, bg, steps=2, optimize_env=False)
    want = smooth_env(*ENV, 9, gpu_device)
    assert torch.equal(mp.env_map.detach(), want) and sp.env_opt.step_count == 0
    start = _model(scene, gpu_device)
    assert (mp.flat - start.flat).abs().max().item() > 1e-4          # the Gaussians moved
    # ... and saw the map: the rendered image is not the one over black
    from fdgs.fused import render_raw
    from fdgs import train_host
    black = render_raw(cams[0], start, train_host.PipelineFlags(), torch.zeros(3, device=gpu_device))["render"]
    assert (renders[0][0] - black).abs().max().item() > 0.05


def test_env_map_res_zero_is_the_plain_pipeline(gpu_device):
    """pipe.env_map_res = 0 (a model that has a map, an optimizer handed in): nothing of the map runs -- the first step is
    bit-identical to a pipeline built without the new arguments."""
    from fdgs import train_host
    from fdgs.envmap import EnvMapAdam
    from fdgs.pipeline import StepPipeline
    B = 3
    scene, cams, gts, _masks, bg = _setup(gpu_device, B)
    outs = {}
    for mode in ("plain", "env0"):
        mp = _model(scene, gpu_device)
        kw = dict(env_optimizer=EnvMapAdam(mp.env_map)) if mode == "env0" else {}
        sp = StepPipeline(mp, train_host.make_optimizer(mp), world_size=1, lambda_dssim=0.2, **kw)
        res, ls = sp.step(cams, gts, train_host.PipelineFlags(), bg, **({"optimize_env": True} if mode == "env0" else {}))
        torch.cuda.synchronize()
        outs[mode] = ([r["render"].clone() for r in res], torch.stack(ls).clone(), mp.flat.clone(), mp.env_map.detach().clone())
    for a, b in zip(outs["plain"][0], outs["env0"][0]):
        assert torch.equal(a, b)
    assert torch.equal(outs["plain"][1], outs["env0"][1])
    # (the parameters after the step: within the float-atomics noise of the blend backward; the map untouched)
    perr = (outs["plain"][2] - outs["env0"][2]).abs()
    assert (perr > 2e-3).float().mean().item() <= 2e-3
    assert torch.equal(outs["env0"][3], smooth_env(*ENV, 9, gpu_device))


def test_env_map_refusals(gpu_device):
    from fdgs import train_host
    from fdgs.pipeline import StepPipeline
    scene, cams, gts, _masks, bg = _setup(gpu_device, 1, P=500)
    mp = train_host.GaussianParams(scene, gpu_device)      # no env_map
    sp = StepPipeline(mp, train_host.make_optimizer(mp), world_size=1)
    with pytest.raises(ValueError, match="env_map"):
        sp.step(cams, gts, EnvPipe(8), bg)
    sp2 = StepPipeline(mp, train_host.make_optimizer(mp), world_size=2)
    with pytest.raises(NotImplementedError):
        sp2.step(cams, gts, EnvPipe(8), bg)


def test_harness_train_learns_the_env_map(gpu_device):
    """Ground truth rendered over a known smooth environment; training starts from a zero map (train.py:71-77).  After 200 steps the
    PSNR clears a bar and the map's error on the texels the cameras see has fallen; env_optimize_until = 1 keeps the map at zero."""
    from fdgs import harness, train_host
    from fdgs.fused import render_raw
    cfg = synth.SceneConfig("envtrain", 2000, 160, 128, 2, 1, 0.03, 10.0, True, 4, False)
    R = 32
    V = 8
    runs = {}
    for until in (10 ** 9, 1):
        scene = synth.make_scene(cfg, seed=5)
        bg = torch.zeros(3, device=gpu_device)
        target = train_host.GaussianParams(scene, gpu_device)
        truth = smooth_env(R, R, 4, gpu_device)
        target.env_map = truth
        cams = [train_host.SyntheticCamera(scene, gpu_device, timestamp=(v + 0.5) / V * scene["time_duration"]) for v in range(V)]
        with torch.no_grad():
            gts = [render_raw(c, target, EnvPipe(R), bg)["render"].clone() for c in cams]
            # the texels the cameras see: the map's gradient of a unit upstream is non-zero there
            seen = torch.zeros(3, R, R, device=gpu_device)
            from fdgs.envmap import composite_backward
            for c in cams:
                T = torch.ones(scene["H"], scene["W"], device=gpu_device)
                composite_backward(T, torch.ones(3, scene["H"], scene["W"], device=gpu_device), truth, c, g_env=seen, accumulate_env=True)
            seen = seen > 1.0
        student = train_host.GaussianParams(scene, gpu_device)
        g = torch.Generator(device="cpu").manual_seed(0)
        with torch.no_grad():
            student.params["_features"].add_(0.2 * torch.randn(student.params["_features"].shape, generator=g).to(gpu_device))
        opt = train_host.make_optimizer(student)
        hist = harness.train(student, opt, cams, gts, EnvPipe(R), bg, iterations=200, batch_size=4, log_every=50, log=lambda s: None,
                             densify_until_iter=0, env_lr=2e-2, env_optimize_until=until)
        torch.cuda.synchronize()
        err0 = (truth[seen]).abs().mean().item()
        err = (student.env_map.detach() - truth)[seen].abs().mean().item()
        runs[until] = (hist, err0, err, student.env_map.detach().clone(), int(seen.sum()))
    hist, err0, err, _m, nseen = runs[10 ** 9]
    assert nseen > 50
    assert hist["psnr"][-1] > 25.0, hist
    assert err < 0.3 * err0, (err, err0)
    assert torch.count_nonzero(runs[1][3]) == 0
