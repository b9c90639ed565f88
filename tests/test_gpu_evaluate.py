"""GPU: fdgs.metrics.evaluate (training_report's inner loop on the fast path) against a per-view loop of the drop-in render() +
clamp + the float64 oracle, and the evaluation hook of harness.train."""
import numpy as np
import pytest
import torch

import metrics_oracle as mo
from util import synth

pytestmark = pytest.mark.gpu
BARS = (2e-6, 1e-4, 2e-6, 1e-5)
REF_BARS = (1e-5, 1e-3, 2e-5, 1e-4)   # against render()'s image: the bars above plus what the two paths' pixels may differ by


class EnvPipe:
    compute_cov3D_python = False
    convert_SHs_python = False
    debug = False

    def __init__(self, res):
        self.env_map_res = res


def _scene(dev, V, seed=3):
    from fdgs import train_host
    cfg = synth.SceneConfig("evalC1", 10_000, 400, 400, 3, 1, 0.03, 1.0, True, 4, False)   # C1 size, rot_4d, SH 3 + time 1
    scene = synth.make_scene(cfg, seed=seed)
    cams = [train_host.SyntheticCamera(scene, dev, timestamp=(v + 0.5) / V * scene["time_duration"]) for v in range(V)]
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(3, 52, 52, generator=g)
    gts = [torch.nn.functional.interpolate(base[None], size=(400, 400), mode="bilinear", align_corners=False)[0].roll(17 * v, -1).to(dev)
           for v in range(V)]
    return scene, cams, gts


def _compare(model, cams, gts, pipe, bg):
    from fdgs.fused import render_raw
    from fdgs.gaussian_renderer import render
    from fdgs.metrics import evaluate
    ev = evaluate(model, cams, gts, pipe, bg)
    rows = ev["rows"]
    assert rows.shape == (len(cams), 4) and ev["views"] == len(cams)
    sums = np.zeros(4)
    for v, (cam, gt) in enumerate(zip(cams, gts)):
        with torch.no_grad():
            fast = render_raw(cam, model, pipe, bg)["render"]
            ref = render(cam, model, pipe, bg)["render"]
        # the two render paths (activations in the kernels vs in PyTorch): the pixel tolerance of the render-branch tests
        d = (fast - ref).abs()
        scale = max(1.0, float(ref.abs().max()))
        assert float((d > 1e-4 * scale).float().mean()) <= 2e-3 and float(d.max()) <= 5e-2 * scale, float(d.max())
        want_fast = mo.metrics(fast.cpu(), gt.cpu())
        want_ref = mo.metrics(ref.cpu(), gt.cpu())
        for k in range(4):
            assert abs(float(rows[v, k]) - want_fast[k]) <= BARS[k], (v, k, float(rows[v, k]), want_fast[k])
            assert abs(float(rows[v, k]) - want_ref[k]) <= REF_BARS[k], (v, k, float(rows[v, k]), want_ref[k])
        sums += np.array(want_ref)
    for k, name in enumerate(("l1", "psnr", "ssim", "msssim")):
        assert abs(ev[name] - sums[k] / len(cams)) <= REF_BARS[k], (name, ev[name], sums[k] / len(cams))
        assert abs(ev[name] - float(rows[:, k].double().mean())) <= 1e-12
    return ev


def test_evaluate_matches_render_and_oracle(gpu_device):
    from fdgs import train_host
    scene, cams, gts = _scene(gpu_device, 5)
    model = train_host.GaussianParams(scene, gpu_device)
    ev = _compare(model, cams, gts, train_host.PipelineFlags(), torch.tensor([0.1, 0.2, 0.3], device=gpu_device))
    assert 0.0 < ev["msssim"] < 1.0 and np.isfinite(ev["psnr"])


def test_evaluate_with_environment_map(gpu_device):
    from fdgs import train_host
    from test_gpu_envmap import smooth_env
    scene, cams, gts = _scene(gpu_device, 3, seed=4)
    model = train_host.GaussianParams(scene, gpu_device)
    model.env_map = smooth_env(64, 64, 9, gpu_device)
    _compare(model, cams, gts, EnvPipe(64), torch.zeros(3, device=gpu_device))


def test_first_view_renders_few_gaussians(gpu_device):
    """The first view looks past the scene's edge and sees a few hundred Gaussians, the others all 10 000: every row still equals
    the metrics of that view rendered on its own."""
    from fdgs import train_host
    from fdgs.fused import render_raw
    from fdgs.metrics import evaluate, image_metrics
    scene, cams, gts = _scene(gpu_device, 4, seed=5)
    aside = dict(scene)
    aside.update(synth.make_camera(scene["W"], scene["H"], yaw=0.85))
    cams[0] = train_host.SyntheticCamera(aside, gpu_device, timestamp=0.5)
    model = train_host.GaussianParams(scene, gpu_device)
    pipe, bg = train_host.PipelineFlags(), torch.tensor([0.1, 0.2, 0.3], device=gpu_device)
    with torch.no_grad():
        r0 = render_raw(cams[0], model, pipe, bg)
        r1 = render_raw(cams[1], model, pipe, bg)
    assert 0 < int((r0["radii"] > 0).sum()) * 10 < int((r1["radii"] > 0).sum())
    ev = evaluate(model, cams, gts, pipe, bg)
    for v in range(4):
        with torch.no_grad():
            want = image_metrics(render_raw(cams[v], model, pipe, bg)["render"], gts[v]).cpu()
        assert torch.equal(ev["rows"][v], want), (v, ev["rows"][v], want)


def _train_setup(dev, V=12, T=4):
    from fdgs import train_host
    from fdgs.fused import render_raw
    scene = synth.make_scene(synth.CONFIGS["C1"], seed=0)
    pipe, bg = train_host.PipelineFlags(), scene["bg"].to(dev)
    target = train_host.GaussianParams(scene, dev)
    cams = [train_host.SyntheticCamera(scene, dev, timestamp=(v + 0.5) / V * scene["time_duration"]) for v in range(V)]
    tcams = [train_host.SyntheticCamera(scene, dev, timestamp=(v + 0.25) / T * scene["time_duration"]) for v in range(T)]
    with torch.no_grad():
        gts = [render_raw(c, target, pipe, bg)["render"].clone() for c in cams]
        tgts = [render_raw(c, target, pipe, bg)["render"].clone() for c in tcams]
    student = train_host.GaussianParams(scene, dev)
    g = torch.Generator(device="cpu").manual_seed(1)
    with torch.no_grad():
        student.params["_features"].add_(0.3 * torch.randn(student.params["_features"].shape, generator=g).to(dev))
        student.params["_opacity"].add_(0.5 * torch.randn(student.params["_opacity"].shape, generator=g).to(dev))
    return student, train_host.make_optimizer(student), cams, gts, tcams, tgts, pipe, bg


def test_harness_train_evaluates(gpu_device):
    from fdgs import harness
    student, opt, cams, gts, tcams, tgts, pipe, bg = _train_setup(gpu_device)
    calls = []
    hist = harness.train(student, opt, cams, gts, pipe, bg, iterations=100, batch_size=4, test_cameras=tcams, test_gts=tgts,
                         test_iterations=[50, 100], on_evaluate=lambda it, name, m: calls.append((it, name, m)))
    ev = hist["eval"]
    assert [(e["iteration"], e["set"]) for e in ev] == [(50, "train"), (50, "test"), (100, "train"), (100, "test")]
    assert [(c[0], c[1]) for c in calls] == [(e["iteration"], e["set"]) for e in ev]
    for e in ev:
        assert set(("l1", "psnr", "ssim", "msssim")) <= set(e) and all(np.isfinite(e[k]) for k in ("l1", "psnr", "ssim", "msssim"))
    test = [e for e in ev if e["set"] == "test"]
    assert test[1]["psnr"] > test[0]["psnr"], test
    assert test[0]["views"] == len(tcams) and [e for e in ev if e["set"] == "train"][0]["views"] == 5


def test_harness_train_without_evaluation_keeps_its_keys(gpu_device):
    from fdgs import harness
    student, opt, cams, gts, _tc, _tg, pipe, bg = _train_setup(gpu_device)
    hist = harness.train(student, opt, cams, gts, pipe, bg, iterations=10, batch_size=4, log_every=5, log=lambda s: None)
    assert set(hist) == {"iteration", "loss", "psnr"}
