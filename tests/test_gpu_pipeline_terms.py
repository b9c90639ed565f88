"""GPU: StepPipeline with the reference trainer's rigid, motion and opacity-mask terms (lambda_rigid / lambda_motion /
lambda_opa_mask) against render_raw + fused_l1_ssim + the torch oracle terms (tests/regularizer_oracle.py) + autograd + Adam,
and harness.train with lego's lambda_rigid = 1."""
import numpy as np
import pytest
import torch

from util import synth
import regularizer_oracle as ro

pytestmark = pytest.mark.gpu
LAM = dict(lambda_rigid=1.0, lambda_motion=0.5, lambda_opa_mask=0.3)


def _setup(dev, B, P=6000, seed=4):
    from fdgs import train_host
    cfg = synth.SceneConfig("terms", P, 208, 160, 3, 2, 0.03, 10.0, True, 4, False)
    scene = synth.make_scene(cfg, seed=seed)
    cams = [train_host.SyntheticCamera(scene, dev, timestamp=(b + 0.5) / B * scene["time_duration"]) for b in range(B)]
    gen = torch.Generator(device="cpu").manual_seed(7)
    gts = [torch.rand(3, scene["H"], scene["W"], generator=gen).to(dev) for _ in range(B)]
    masks = [(torch.rand(1, scene["H"], scene["W"], generator=gen) > 0.5).float().to(dev) for _ in range(B)]
    return scene, cams, gts, masks, train_host.PipelineFlags(), torch.tensor([0.1, 0.2, 0.3], device=dev)


def _reference(scene, cams, gts, masks, pipe, bg, steps=2, k=20):
    """render_raw + fused_l1_ssim + the torch terms per view (train.py:115-162), autograd, Adam.  The rigid / motion terms do not
    depend on the view: B views x (1 / B) = their gradient once per step, taken in a backward of its own (the raster backward of
    view 0 WRITES the bucket, and autograd does not order it against the accumulation of another branch)."""
    from fdgs import train_host
    from fdgs.fused import render_raw
    from fdgs.knn import knn
    from fdgs.loss import fused_l1_ssim
    dev = bg.device
    B = len(cams)
    ma = train_host.GaussianParams(scene, dev)
    oa = train_host.make_optimizer(ma)
    sink = ma.grad_sink()
    losses, terms = [], []
    for _ in range(steps):
        opa = []
        for b in range(B):
            pkg = render_raw(cams[b], ma, pipe, bg, grad_sink=sink, accumulate=b > 0)
            l1s = fused_l1_ssim(pkg["render"], gts[b], 0.2)
            lo = ro.opa_mask(pkg["alpha"], masks[b])
            ((l1s + LAM["lambda_opa_mask"] * lo) / B).backward()
            losses.append(float(l1s))
            opa.append(float(lo))
        idx, d2 = knn(ma._xyz.detach()[None], ma._xyz.detach()[None], k)
        v = ro.velocity(ma._scaling, ma._scaling_t, ma._rotation, ma._rotation_r, ma._t, torch.float32)
        lr, lm = ro.rigid(v, idx[0], d2[0]), ro.motion(v)
        (LAM["lambda_rigid"] * lr + LAM["lambda_motion"] * lm).backward()
        terms.append((float(lr), float(lm), opa))
        oa.step()
    torch.cuda.synchronize()
    return ma, losses, terms


def _pipeline(scene, cams, gts, masks, pipe, bg, steps=2, mods=None, **kw):
    from fdgs import train_host
    from fdgs.pipeline import StepPipeline
    mp = train_host.GaussianParams(scene, bg.device)
    sp = StepPipeline(mp, train_host.make_optimizer(mp), world_size=1, lambda_dssim=0.2, **kw)
    losses, terms = [], []
    for s in range(steps):
        _res, ls = sp.step(cams, gts, pipe, bg, scaling_modifier=1.0 if mods is None else mods[s],
                           alpha_masks=masks if kw.get("lambda_opa_mask", 0) > 0 else None)
        losses += [float(l) for l in ls]
        t = sp.last_terms
        terms.append((float(t["rigid"]), float(t["motion"]), t["opa_mask"].tolist()) if t else None)
    torch.cuda.synchronize()
    return mp, sp, losses, terms


def _close(mp, ma, fuse, got_losses, ref_losses, got_terms, ref_terms, reg=None):
    np.testing.assert_allclose(got_losses, ref_losses, rtol=3e-5, atol=1e-6)
    for (gr, gm, go), (wr, wm, wo) in zip(got_terms, ref_terms):
        np.testing.assert_allclose([gr, gm], [wr, wm], rtol=3e-5)
        np.testing.assert_allclose(go, wo, rtol=3e-5, atol=1e-6)
    # the bars of tests/test_gpu_api.py::test_step_pipeline_matches_autograd_step (float atomics in the blend backward)
    n_cmp = mp.offsets["_features"][0] if fuse else mp.flat.numel()
    gerr = (mp.flat_grad[:n_cmp] - ma.flat_grad[:n_cmp]).abs()
    gscale = max(1e-6, ma.flat_grad.abs().max().item())
    assert gerr.max().item() <= 1e-3 * gscale, (gerr.max().item(), gscale)
    perr = (mp.flat - ma.flat).abs()
    assert (perr > 2e-3).float().mean().item() <= 2e-3 and perr.max().item() <= 0.25, ((perr > 2e-3).float().mean().item(), perr.max().item())
    # the bar above is relative to the bucket's largest entry, a rasteriser gradient orders of magnitude above the regularisers': their
    # part of the step's gradient is held to the float64 oracle relative to its own size
    for n, (got, spread, bar) in (reg or {}).items():
        ratio = bar.ratio(got)
        print("pipeline regulariser part %-12s max|ref| %.2e raster noise %.2e grad_bar %.2e err %.2e err/unit %.2f"
              % (n, bar.ref_max, spread, bar.bar, bar.err(got), ratio))
        if n in REG_HELD:
            assert bar.err(got) <= 4 * spread + bar.bar, (n, bar.err(got), spread, bar.bar, bar.ref_max)


# the tensors on which the rasteriser's atomic-order noise does not swamp the regularisers' gradient ("Regulariser gradients"):
# 4 x noise is 1 .. 6 % of max|ref| on these.  On _scaling_t the noise (7e-9 .. 3e-8) is above the whole gradient (max|ref| 5.9e-9): printed only
REG_HELD = ("_scaling", "_rotation", "_rotation_r")
_REG_BARS = {}


def _regulariser_part(scene, cams, gts, masks, pipe, bg, **kw):
    """Per raw tensor: (the first step's gradient with lambda_rigid / lambda_motion on minus the same step with both off -- the
    opacity-mask term stays on in both, it reaches these tensors through the rasteriser --, the spread of that difference over two
    identical repeats: the float-atomics noise of two rasteriser backwards, the oracle's bar of lambda_rigid L_rigid + lambda_motion L_motion)."""
    from fdgs import train_host
    from fdgs.knn import knn
    from fdgs.pipeline import StepPipeline

    def first_step(lam):
        mp = train_host.GaussianParams(scene, bg.device)
        StepPipeline(mp, train_host.make_optimizer(mp), world_size=1, lambda_dssim=0.2, **kw, **lam).step(cams, gts, pipe, bg, alpha_masks=masks)
        torch.cuda.synchronize()
        return mp
    off = dict(LAM, lambda_rigid=0.0, lambda_motion=0.0)
    diffs = []
    for _ in range(2):
        on_, off_ = first_step(LAM), first_step(off)
        diffs.append((on_.flat_grad - off_.flat_grad).cpu())
        offsets = on_.offsets
    key = len(cams)
    if key not in _REG_BARS:
        m = train_host.GaussianParams(scene, bg.device)
        idx, d2 = knn(m._xyz.detach()[None], m._xyz.detach()[None], 20)
        params = {n: getattr(m, n).detach().cpu() for n in ro.NAMES4 + ("_t",)}
        _REG_BARS[key] = ro.grad_bar(params, idx[0].cpu(), d2[0].cpu(), LAM["lambda_rigid"], LAM["lambda_motion"])
    out = {}
    for n, bar in _REG_BARS[key].items():
        b, e = offsets[n]
        out[n] = (diffs[0][b:e].view(bar.ref.shape), float((diffs[0][b:e] - diffs[1][b:e]).abs().max()), bar)
    return out


@pytest.mark.parametrize("overlap,fuse,B", [(True, True, 3), (False, True, 3), (True, False, 3), (True, True, 1), (True, False, 1)])
@pytest.mark.parametrize("group", [1, 2], ids=["per-view", "sh-pairs"])
def test_pipeline_with_terms_matches_autograd_step(gpu_device, overlap, fuse, B, group):
    scene, cams, gts, masks, pipe, bg = _setup(gpu_device, B)
    ma, ref_losses, ref_terms = _reference(scene, cams, gts, masks, pipe, bg)
    mp, _sp, got_losses, got_terms = _pipeline(scene, cams, gts, masks, pipe, bg, overlap=overlap, fuse_sh_adam=fuse, sh_group=group, **LAM)
    reg = _regulariser_part(scene, cams, gts, masks, pipe, bg, overlap=overlap, fuse_sh_adam=fuse, sh_group=group)
    _close(mp, ma, fuse, got_losses, ref_losses, got_terms, ref_terms, reg)


def test_pipeline_with_terms_lazy_redo(gpu_device):
    """A lazy step that outgrows its run-ahead buffers (scaling_modifier 2.6 after two steps at 1.0, as in tests/test_gpu_api.py) is redone with the terms re-enqueued, and equals
    the waiting pipeline."""
    B = 3
    scene, cams, gts, masks, pipe, bg = _setup(gpu_device, B, P=6007)
    runs = {}
    for lazy in (False, True):
        runs[lazy] = _pipeline(scene, cams, gts, masks, pipe, bg, steps=4, mods=(1.0, 1.0, 2.6, 2.6), lazy=lazy, **LAM)
    assert runs[False][1].lazy_redone == 0 and runs[True][1].lazy_redone == 1
    np.testing.assert_allclose(runs[True][2], runs[False][2], rtol=3e-5, atol=1e-6)
    for a, b in zip(runs[True][3], runs[False][3]):
        np.testing.assert_allclose(a[:2], b[:2], rtol=3e-5)
        np.testing.assert_allclose(a[2], b[2], rtol=3e-5, atol=1e-6)
    perr = (runs[True][0].flat - runs[False][0].flat).abs()
    assert (perr > 2e-3).float().mean().item() <= 2e-3 and perr.max().item() <= 0.25


def test_pipeline_with_zero_lambdas_is_the_plain_pipeline(gpu_device):
    """All lambdas 0: nothing of the terms runs -- the first step (identical inputs) is bit-identical to a pipeline built without the
    arguments, later steps within the float-atomics noise two runs of one pipeline differ by; no terms reported."""
    from fdgs import train_host
    from fdgs.pipeline import StepPipeline
    B = 3
    scene, cams, gts, _masks, pipe, bg = _setup(gpu_device, B)
    outs = {}
    for mode in ("plain", "zeros"):
        mp = train_host.GaussianParams(scene, gpu_device)
        kw = dict(lambda_rigid=0.0, lambda_motion=0.0, lambda_opa_mask=0.0, rigid_k=20) if mode == "zeros" else {}
        sp = StepPipeline(mp, train_host.make_optimizer(mp), world_size=1, lambda_dssim=0.2, **kw)
        res, ls = sp.step(cams, gts, pipe, bg)
        first = ([r["render"].clone() for r in res], torch.stack(ls).clone())
        _res, ls2 = sp.step(cams, gts, pipe, bg)
        torch.cuda.synchronize()
        outs[mode] = (first, [float(l) for l in ls2], mp.flat.clone(), sp.last_terms)
    for a, b in zip(outs["plain"][0][0], outs["zeros"][0][0]):
        assert torch.equal(a, b)
    assert torch.equal(outs["plain"][0][1], outs["zeros"][0][1])
    assert outs["zeros"][3] == {}
    np.testing.assert_allclose(outs["zeros"][1], outs["plain"][1], rtol=3e-5, atol=1e-6)
    perr = (outs["zeros"][2] - outs["plain"][2]).abs()
    assert (perr > 2e-3).float().mean().item() <= 2e-3


def test_pipeline_with_terms_overlap_steps_equals_plain(gpu_device):
    B = 3
    scene, cams, gts, masks, pipe, bg = _setup(gpu_device, B)
    plain = _pipeline(scene, cams, gts, masks, pipe, bg, steps=4, **LAM)
    over = _pipeline(scene, cams, gts, masks, pipe, bg, steps=4, overlap_steps=True, **LAM)
    assert over[1].overlap_steps and over[1].steps_carried == 3
    np.testing.assert_allclose(over[2][:B], plain[2][:B], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(over[2], plain[2], rtol=1e-4, atol=1e-6)
    for a, b in zip(over[3], plain[3]):
        np.testing.assert_allclose(a[:2], b[:2], rtol=1e-4)
    perr = (over[0].flat - plain[0].flat).abs()
    assert (perr > 2e-3).float().mean().item() <= 2e-3 and perr.max().item() <= 0.25


def test_pipeline_terms_refusals(gpu_device):
    from fdgs import train_host
    from fdgs.pipeline import StepPipeline
    scene, cams, gts, _masks, pipe, bg = _setup(gpu_device, 1, P=500)
    mp = train_host.GaussianParams(scene, gpu_device)
    with pytest.raises(NotImplementedError):
        StepPipeline(mp, train_host.make_optimizer(mp), world_size=2, lambda_rigid=1.0)
    sp = StepPipeline(mp, train_host.make_optimizer(mp), world_size=1, lambda_opa_mask=0.1)
    with pytest.raises(ValueError, match="alpha mask"):
        sp.step(cams, gts, pipe, bg)


def test_harness_train_with_lego_rigid_weight(gpu_device):
    """harness.train, 300 steps with clones and splits inside the run (densification from iteration 100 every 100): finite losses, and
    lambda_rigid = 1 (configs/dnerf/lego.yaml) ends with a lower L_rigid than the same run without it."""
    from fdgs import harness, train_host
    from fdgs.fused import render_raw
    from fdgs.loss import rigid_motion_loss
    cfg = synth.SceneConfig("lego", 3000, 160, 128, 2, 1, 0.04, 10.0, True, 4, False)
    scene = synth.make_scene(cfg, seed=6)
    pipe = train_host.PipelineFlags()
    bg = torch.zeros(3, device=gpu_device)
    target = train_host.GaussianParams(scene, gpu_device)
    V = 8
    cams = [train_host.SyntheticCamera(scene, gpu_device, timestamp=(v + 0.5) / V * scene["time_duration"]) for v in range(V)]
    with torch.no_grad():
        gts = [render_raw(c, target, pipe, bg)["render"].clone() for c in cams]
    final = {}
    for lam in (0.0, 1.0):
        student = train_host.GaussianParams(scene, gpu_device)
        g = torch.Generator(device="cpu").manual_seed(0)
        with torch.no_grad():
            student.params["_features"].add_(0.3 * torch.randn(student.params["_features"].shape, generator=g).to(gpu_device))
            student.params["_xyz"].add_(0.01 * torch.randn(student.params["_xyz"].shape, generator=g).to(gpu_device))
        opt = train_host.make_optimizer(student)
        lines = []
        hist = harness.train(student, opt, cams, gts, pipe, bg, iterations=300, batch_size=4, log_every=30, log=lines.append,
                             densify_from_iter=100, densification_interval=100, densify_until_iter=250, opacity_reset_interval=10 ** 6,
                             densify_grad_threshold=5e-4, cameras_extent=2.0, lambda_rigid=lam)
        torch.cuda.synchronize()
        assert any("densify" in l for l in lines), lines
        assert np.isfinite(hist["loss"]).all() and torch.isfinite(student.flat).all()
        with torch.no_grad():
            final[lam] = float(rigid_motion_loss(student)[0])
    assert final[1.0] < final[0.0], final
