"""GPU: fdgs.playback.render_path (a time sweep of a small rot_4d scene out as 8-bit frames, with alpha, grey depth and the
environment map) and fdgs.checkpoint on the device (a saved run renders and trains on after loading)."""
import math

import pytest
import torch

from test_gpu_frame_encode import cpu_encode, cpu_gray
from util import synth

pytestmark = pytest.mark.gpu
CFG = synth.SceneConfig("path", 4000, 200, 176, 3, 1, 0.03, 10.0, True, 4, False)   # rot_4d, SH 3 + time 1


class Pipe:
    compute_cov3D_python = False
    convert_SHs_python = False
    debug = False

    def __init__(self, res=0):
        self.env_map_res = res


def _model(dev, seed=3, pose="rig1"):
    from fdgs import train_host
    scene = synth.make_scene(CFG, seed=seed, pose=pose, alloc=(3, 2))
    return scene, train_host.GaussianParams(scene, dev), train_host.SyntheticCamera(scene, dev)


def test_time_sweep_helpers(gpu_device):
    from fdgs import playback
    scene, _, cam = _model(gpu_device)
    c = playback.with_timestamp(cam, 2.5)
    assert c is not cam and c.timestamp == 2.5 and cam.timestamp == scene["timestamp"]
    assert c.world_view_transform is cam.world_view_transform and c.image_width == cam.image_width
    sweep = playback.time_sweep(cam, 1.0, 9.0, 5)
    assert [s.timestamp for s in sweep] == [1.0, 3.0, 5.0, 7.0, 9.0]
    assert [s.timestamp for s in playback.time_sweep(cam, 4.0, 9.0, 1)] == [4.0]
    with pytest.raises(ValueError):
        playback.time_sweep(cam, 0.0, 1.0, 0)


@pytest.mark.parametrize("mode", ["rgb-host", "rgb-device", "rgba-depth-host", "env-rgba-depth-device"])
def test_render_path(mode, gpu_device):
    from fdgs import playback
    from fdgs.frames import FrameStore
    from fdgs.fused import render_raw
    from fdgs.metrics import evaluate
    dev = gpu_device
    scene, model, cam = _model(dev)
    env = mode.startswith("env")
    alpha, depth = "rgba" in mode, "depth" in mode
    residency = "host" if mode.endswith("host") else "device"
    pipe = Pipe(32 if env else 0)
    if env:
        from test_gpu_envmap import smooth_env
        model.env_map = smooth_env(32, 32, 5, dev)
    bg = torch.zeros(3, device=dev) if env else torch.tensor([0.1, 0.2, 0.3], device=dev)
    cams = playback.time_sweep(cam, 0.5, 9.5, 6)
    seen = []

    def on_render(i, results):
        assert i == len(seen) and set(results) >= {"render", "alpha", "depth", "radii"}
        seen.append({k: results[k].detach().clone() for k in ("render", "alpha", "depth")})

    res = playback.render_path(model, cams, pipe, bg, alpha=alpha, depth=depth, residency=residency, on_render=on_render)
    N, H, W, C = 6, CFG.H, CFG.W, 4 if alpha else 3
    frames = res["frames"]
    assert res["views"] == N == len(seen) and tuple(frames.shape) == (N, H, W, C) and frames.dtype == torch.uint8
    assert frames.is_pinned() if residency == "host" else frames.is_cuda
    assert ("depth" in res) == depth
    got = frames.cpu()
    for i, s in enumerate(seen):
        img = s["render"].cpu()
        assert float(img.std()) > 1e-3, "view %d is empty" % i
        # the bytes are the CPU expression of the float image the hook saw, exactly
        want = cpu_encode(torch.cat((img, s["alpha"].cpu()), 0) if alpha else img).permute(1, 2, 0)
        diff = int((got[i] != want).sum())
        assert diff == 0, (i, diff)
        # the rule's own bound: half a quantisation step plus the rounding of one fp32 division
        back = got[i][..., :3].permute(2, 0, 1).float() / 255.0
        err = float((back - img.clamp(0, 1)).abs().max())
        assert err <= 0.5 / 255 + 1e-6, (i, err)
        if depth:
            dd = int((res["depth"][i].cpu() != cpu_gray(s["depth"].cpu()[None])[0]).sum())
            assert dd == 0, (i, dd)
    if depth:
        assert tuple(res["depth"].shape) == (N, H, W, 1) and int(res["depth"].max()) == 255 and int(res["depth"].min()) == 0
    # against a separate render_raw call per camera: no byte differs by more than 1
    with torch.no_grad():
        for i, c in enumerate(cams):
            again = cpu_encode(render_raw(c, model, pipe, bg)["render"]).permute(1, 2, 0)
            d = (got[i][..., :3].int() - again.int()).abs()
            assert int(d.max()) <= 1, "view %d: %d bytes differ, the largest difference is %d" % (i, int((d > 0).sum()), int(d.max()))
    # the sweep moves
    assert int((got[0] != got[5]).sum()) > 100
    if not alpha:
        # what came out is what a FrameStore takes: the decoded frames against the same cameras' renders
        store = FrameStore(frames, residency=residency, device=dev)
        ev = evaluate(model, cams, store, pipe, bg, msssim=False)
        floor = 20 * math.log10(510.0) - 0.01      # mean squared error <= (0.5 / 255)^2
        assert ev["psnr"] >= floor and float(ev["rows"][:, 1].min()) >= floor, (ev["psnr"], floor)


def test_render_path_arguments(gpu_device):
    from fdgs import playback, train_host
    from fdgs.frames import FrameWriter
    dev = gpu_device
    scene, model, cam = _model(dev)
    other = train_host.SyntheticCamera(synth.make_scene(CFG, seed=3, W=160, H=112), dev)
    bg = torch.zeros(3, device=dev)
    with pytest.raises(ValueError, match="one image size"):
        playback.render_path(model, [cam, other], Pipe(), bg)
    with pytest.raises(ValueError, match="no cameras"):
        playback.render_path(model, [], Pipe(), bg)
    with pytest.raises(ValueError, match="FrameWriter of 2 frames"):
        playback.render_path(model, [cam, cam], Pipe(), bg, out=FrameWriter(3, CFG.H, CFG.W, device=dev))
    # a writer of the caller's own is written through and reused
    w = FrameWriter(2, CFG.H, CFG.W, residency="device", device=dev)
    a = playback.render_path(model, [cam, playback.with_timestamp(cam, 1.0)], Pipe(), bg, out=w)["frames"]
    assert a is w.frames
    first = a.clone()
    b = playback.render_path(model, [cam, playback.with_timestamp(cam, 1.0)], Pipe(), bg, out=w, scaling_modifier=0.5)["frames"]
    assert b is a and int((b != first).sum()) > 0


def test_checkpoint_on_the_device(gpu_device, tmp_path):
    """save after three StepPipeline steps, load onto the GPU: the loaded model renders bit for bit what the live one renders (the
    forward has no atomics and a fixed order of operations), and trains on."""
    from fdgs import checkpoint, playback, train_host
    from fdgs.fused import render_raw
    from fdgs.pipeline import StepPipeline
    dev = gpu_device
    scene, model, cam = _model(dev, seed=9)
    opt = train_host.FlatAdam(model)
    cams = playback.time_sweep(cam, 1.0, 9.0, 4)
    g = torch.Generator().manual_seed(1)
    gts = [torch.rand(3, CFG.H, CFG.W, generator=g).to(dev) for _ in cams]
    pipe, bg = Pipe(), torch.tensor([0.1, 0.2, 0.3], device=dev)
    sp = StepPipeline(model, opt)
    for k in range(3):
        _, losses = sp.step(cams[:2] if k % 2 == 0 else cams[2:], gts[:2] if k % 2 == 0 else gts[2:], pipe, bg)
    torch.cuda.synchronize()
    assert opt.step_count == 3
    path = str(tmp_path / "chkpnt3.pth")
    checkpoint.save(path, model, opt, 3)
    m2, o2, st2, it = checkpoint.load(path, dev, sh_degree=3, sh_degree_t=2, time_duration=[0.0, CFG.duration])
    assert it == 3 and o2.step_count == 3 and m2.flat.is_cuda and st2.denom.is_cuda
    assert (m2.active_sh_degree, m2.active_sh_degree_t, m2.rot_4d, m2.gaussian_dim) == (3, 1, True, 4)
    assert torch.equal(m2.flat, model.flat) and torch.equal(o2.exp_avg, opt.exp_avg) and torch.equal(o2.exp_avg_sq, opt.exp_avg_sq)
    with torch.no_grad():
        for c in (cams[0], cams[3]):
            live, loaded = render_raw(c, model, pipe, bg), render_raw(c, m2, pipe, bg)
            for k in ("render", "depth", "alpha", "radii"):
                assert torch.equal(live[k], loaded[k]), k
    # one further step on the loaded model, next to the same step on the live one
    before = m2.flat.detach().clone()
    _, la = StepPipeline(m2, o2).step(cams[:2], gts[:2], pipe, bg)
    _, lb = sp.step(cams[:2], gts[:2], pipe, bg)
    torch.cuda.synchronize()
    assert o2.step_count == 4 and all(math.isfinite(float(x)) for x in la)
    assert [float(x) for x in la] == [float(x) for x in lb], "the loaded model's losses differ from the live model's"
    assert bool(torch.isfinite(m2.flat).all()) and not torch.equal(m2.flat, before)
