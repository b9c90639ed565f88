"""Per-camera colour correction: a synthetic rot_4d scene whose ground-truth frames carry a known gain and offset per camera, trained
with and without fdgs.exposure.ExposureModel in the StepPipeline.

    python examples/train_with_exposure.py --iterations 400
    python examples/train_with_exposure.py --bench       # the kernels at 1352 x 1014 next to PyTorch, and the step rate on and off

Prints the held-out PSNR, raw and after the closed-form colour alignment (``_cc``), and the recovered rows next to the true ones.  A
transform shared by every camera cannot be told from the scene's own colours, so the rows are compared after dividing out camera 0's.
"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

TRAIN_POSES, TEST_POSE = ("rig0", "rig1", "rig3"), "rig2"
GAINS = ((1.0, 1.0, 1.0), (0.7, 0.75, 0.8), (1.3, 1.2, 1.25))      # per camera and channel
OFFSETS = (0.0, 0.03, -0.02)


def _camera(scene, pose, dev, timestamp, uid):
    from fdgs import synth, train_host
    cam = train_host.SyntheticCamera(dict(scene, **synth.camera_for(pose, scene["W"], scene["H"])), dev, timestamp=timestamp)
    cam.uid = uid
    return cam


def run(dev, iterations=400, P=3000, W=200, H=152, views=4, seed=0, log=print):
    from fdgs import exposure, synth, train_host
    from fdgs.fused import render_raw
    from fdgs.pipeline import StepPipeline
    scene = synth.make_scene(synth.SceneConfig("exposure", P, W, H, 2, 1, 0.05, 1.0, True, 4, False), seed=seed)
    pipe, bg = train_host.PipelineFlags(), torch.zeros(3, device=dev)
    target = train_host.GaussianParams(scene, dev)
    times = [(k + 0.5) / views * scene["time_duration"] for k in range(views)]
    cams = [_camera(scene, p, dev, t, uid) for uid, p in enumerate(TRAIN_POSES) for t in times]
    tcams = [_camera(scene, TEST_POSE, dev, t, 0) for t in times]
    truth = torch.zeros((len(TRAIN_POSES), 12))
    for k, (g, o) in enumerate(zip(GAINS, OFFSETS)):
        truth[k] = torch.tensor([g[0], 0, 0, o, 0, g[1], 0, o, 0, 0, g[2], o])
    with torch.no_grad():
        gts = [exposure.apply_(render_raw(c, target, pipe, bg)["render"].contiguous().clone(), truth.to(dev), c.uid) for c in cams]
        tgts = [render_raw(c, target, pipe, bg)["render"].clone() for c in tcams]
    out = {}
    for mode in ("without", "with"):
        g = torch.Generator().manual_seed(seed + 1)
        raw = {n: p.detach().clone() for n, p in target.params.items()}
        raw["_features"] += 0.3 * torch.randn(raw["_features"].shape, generator=g).to(dev)
        student = train_host.GaussianParams.from_raw(raw, dev, **target.settings())
        ex = exposure.ExposureModel(len(TRAIN_POSES), dev, lr=2e-3) if mode == "with" else None
        sp = StepPipeline(student, train_host.make_optimizer(student), world_size=1, lambda_dssim=0.2, exposure=ex)
        B = 3
        for it in range(iterations):
            ix = [b * views + it % views for b in range(B)]      # one view of every camera per step
            sp.step([cams[i] for i in ix], [gts[i] for i in ix], pipe, bg)
        res = exposure.evaluate_corrected(student, tcams, tgts, pipe, bg, msssim=False)
        log("%s the exposure model: held-out PSNR %.2f dB, after colour alignment (psnr_cc) %.2f dB" % (mode, res["psnr"], res["psnr_cc"]))
        out[mode] = (res, ex)
    ex = out["with"][1]
    got = ex.table.cpu().double().reshape(-1, 3, 4)
    want = truth.double().reshape(-1, 3, 4)
    log("rows relative to camera 0's diagonal (recovered | true):")
    for k in range(len(TRAIN_POSES)):
        rel = torch.stack([got[k, i, i] / got[0, i, i] for i in range(3)])
        rel_true = torch.stack([want[k, i, i] / want[0, i, i] for i in range(3)])
        log("  camera %d: gains %s | %s   offsets %s | %s" % (k, [round(float(x), 3) for x in rel], [round(float(x), 3) for x in rel_true],
                                                             [round(float(x), 3) for x in got[k, :, 3]], [round(float(x), 3) for x in want[k, :, 3]]))
    return out


def _timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def bench(dev, W=1352, H=1014, steps=30, log=print):
    """The three image kernels at ``W`` x ``H`` next to their PyTorch formulation, and StepPipeline images/s on the C3 scene with the
    exposure model on and off."""
    from fdgs import exposure, synth, train_host
    from fdgs.pipeline import StepPipeline
    g = torch.Generator().manual_seed(0)
    img, gt, up = (torch.rand(3, H, W, generator=g).to(dev) for _ in range(3))
    ex = exposure.ExposureModel(4, dev)
    ex.table.add_(0.1 * torch.randn(4, 12, generator=g).to(dev))
    out, gi, slot = torch.empty_like(img), torch.empty_like(img), torch.empty(12, device=dev)
    A = ex.table[1].reshape(3, 4)
    n = H * W

    def report(name, ms, nbytes, ms_t):
        log("%-28s %8.1f us  %7.0f GB/s of the %d B/pixel it must move   PyTorch %8.1f us" % (name, ms * 1e3, nbytes / ms * 1e-6, nbytes // n, ms_t * 1e3))
    report("apply", _timed(lambda: exposure.apply_(img, ex, 1, out=out), 50), 24 * n,
           _timed(lambda: torch.addmm(A[:, 3:], A[:, :3], img.view(3, -1)), 20))

    def backward_torch():
        g2 = up.view(3, -1)
        return A[:, :3].t() @ g2, g2.double() @ torch.cat([img.view(3, -1), torch.ones(1, n, device=dev)]).double().t()
    report("backward (one pass + finish)", _timed(lambda: exposure.backward_(up, img, ex, 1, slot, out=gi), 50), 36 * n, _timed(backward_torch, 10))

    def moments_torch():
        c1 = torch.cat([img.view(3, -1).clamp(0, 1), torch.ones(1, n, device=dev)]).double()
        return c1 @ c1.t(), gt.view(3, -1).double() @ c1.t()
    report("fit moments (+ finish)", _timed(lambda: exposure.fit_moments(img, gt), 50), 24 * n, _timed(moments_torch, 10))
    slots = torch.randn(4, 12, generator=g).to(dev)
    log("%-28s %8.1f us" % ("table Adam, 4 views", _timed(lambda: ex.step([0, 1, 2, 3], slots), 50) * 1e3))

    scene = synth.make_scene(synth.CONFIGS["C3"], seed=0)
    B = 4
    cams = [train_host.SyntheticCamera(scene, dev, timestamp=(b + 0.5) / B * scene["time_duration"]) for b in range(B)]
    for b, c in enumerate(cams):
        c.uid = b
    gts = [torch.rand(3, scene["H"], scene["W"], generator=g).to(dev) for _ in range(B)]
    pipe, bg = train_host.PipelineFlags(), torch.zeros(3, device=dev)
    for mode in ("off", "on", "off", "on"):
        m = train_host.GaussianParams(scene, dev)
        model = exposure.ExposureModel(B, dev) if mode == "on" else None
        sp = StepPipeline(m, train_host.make_optimizer(m), world_size=1, lambda_dssim=0.2, exposure=model)
        ms = _timed(lambda: sp.step(cams, gts, pipe, bg), steps)
        log("StepPipeline, C3 (%d Gaussians, %d x %d), %d views per step, exposure %-3s: %.3f ms per step, %.0f images/s"
            % (m.P, scene["W"], scene["H"], B, mode, ms, B / ms * 1e3))
        del sp, m


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=400)
    ap.add_argument("--bench", action="store_true")
    a = ap.parse_args()
    device = torch.device("cuda:0")
    if a.bench:
        bench(device)
    else:
        run(device, a.iterations)
