"""Training to a fixed model size: a synthetic rot_4d scene trained with StepPipeline + fdgs.mcmc.MCMCStrategy (relocate the dead,
grow 5 % per refinement up to a cap, a noise step on the means after every optimizer step, L1 regularisers on opacity and scale).

    python examples/train_mcmc.py --iterations 600 --cap 3000
    python examples/train_mcmc.py --bench            # refine() and the noise step at 2 M Gaussians next to their PyTorch formulation

Prints the held-out PSNR and the number of Gaussians over time.  No gradient statistics, no opacity reset, and the step's buffers are
re-laid out only while the model still grows.
"""
import argparse, math, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

TRAIN_POSES, TEST_POSE = ("rig0", "rig1", "rig3"), "rig2"


def _camera(scene, pose, dev, timestamp):
    from fdgs import synth, train_host
    return train_host.SyntheticCamera(dict(scene, **synth.camera_for(pose, scene["W"], scene["H"])), dev, timestamp=timestamp)


def run(dev, iterations=600, P=4000, start=2000, cap=6000, refine_every=50, W=200, H=152, views=4, seed=0, log=print):
    """The student starts as ``start`` perturbed Gaussians of a ``P``-Gaussian scene and is trained to ``cap``."""
    from fdgs import mcmc, synth, train_host
    from fdgs.fused import render_raw
    from fdgs.pipeline import StepPipeline
    scene = synth.make_scene(synth.SceneConfig("mcmc", P, W, H, 2, 1, 0.05, 1.0, True, 4, False), seed=seed)
    pipe, bg = train_host.PipelineFlags(), torch.zeros(3, device=dev)
    target = train_host.GaussianParams(scene, dev)
    times = [(k + 0.5) / views * scene["time_duration"] for k in range(views)]
    cams = [_camera(scene, p, dev, t) for p in TRAIN_POSES for t in times]
    tcams = [_camera(scene, TEST_POSE, dev, t) for t in times]
    with torch.no_grad():
        gts = [render_raw(c, target, pipe, bg)["render"].clone() for c in cams]
        tgts = [render_raw(c, target, pipe, bg)["render"].clone() for c in tcams]
    g = torch.Generator().manual_seed(seed + 1)
    keep = torch.randperm(P, generator=g)[:start].to(dev)
    raw = {n: p.detach()[keep].clone() for n, p in target.params.items()}
    raw["_xyz"] += 0.03 * torch.randn(raw["_xyz"].shape, generator=g).to(dev)
    raw["_features"] += 0.3 * torch.randn(raw["_features"].shape, generator=g).to(dev)
    student = train_host.GaussianParams.from_raw(raw, dev, **target.settings())
    del target
    opt = train_host.make_optimizer(student)
    strategy = mcmc.MCMCStrategy(student, opt, cap=cap, seed=seed)
    sp = StepPipeline(student, opt, world_size=1, lambda_dssim=0.2, grad_terms=[strategy.add_regularizer_grads])

    def psnr():
        with torch.no_grad():
            mse = [float(((render_raw(c, student, pipe, bg)["render"] - gt) ** 2).mean()) for c, gt in zip(tcams, tgts)]
        return sum(-10.0 * math.log10(max(m, 1e-12)) for m in mse) / len(mse)
    history = [(0, student.P, psnr())]
    log("iteration %5d  P %6d  held-out PSNR %.2f dB" % history[-1])
    B = 2
    for it in range(1, iterations + 1):
        ix = [((it - 1) * B + b) % len(cams) for b in range(B)]
        sp.step([cams[i] for i in ix], [gts[i] for i in ix], pipe, bg)
        strategy.after_step()
        if it % refine_every == 0:
            out = strategy.refine()
            history.append((it, student.P, psnr()))
            log("iteration %5d  P %6d  held-out PSNR %.2f dB   relocated %d, added %d" % (history[-1] + (out["relocated"], out["added"])))
    return history


def _timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def bench(dev, P=2_000_000, M=16, log=print):
    """refine() and the noise step at ``P`` rot_4d Gaussians, next to the same operations written in PyTorch."""
    from fdgs import mcmc, train_host
    g = torch.Generator().manual_seed(0)
    raw = {"_xyz": torch.randn(P, 3, generator=g), "_opacity": torch.randn(P, 1, generator=g) * 3 - 1, "_scaling": torch.rand(P, 3, generator=g) * 3 - 5,
           "_rotation": torch.randn(P, 4, generator=g), "_t": torch.rand(P, 1, generator=g), "_scaling_t": torch.rand(P, 1, generator=g) * 3 - 5,
           "_rotation_r": torch.randn(P, 4, generator=g), "_features": torch.randn(P, M, 3, generator=g)}
    model = train_host.GaussianParams.from_raw(raw, dev, max_sh_degree=3, gaussian_dim=4, rot_4d=True)
    opt = train_host.make_optimizer(model)
    snapshot = model.flat.clone()
    calls = [0]

    def noise():
        calls[0] += 1
        mcmc.noise_step(model, 1.6e-4, 5e5, seed=1, call=calls[0])

    def noise_torch():
        from fdgs.train_host import scaling_rotation_4d
        with torch.no_grad():
            L = scaling_rotation_4d(torch.exp(torch.cat([model._scaling, model._scaling_t], 1)), model._rotation, model._rotation_r)
            sigma = L @ L.transpose(1, 2)
            o = torch.sigmoid(model._opacity)
            d = (sigma @ torch.randn(P, 4, 1, device=dev)).squeeze(-1) * torch.sigmoid(100.0 * ((1 - o) - 0.995)) * 80.0
            model._xyz.add_(d[:, :3])
            model._t.add_(d[:, 3:])
    ms, ms_t = _timed(noise, 20), _timed(noise_torch, 5)
    nbytes = P * (13 + 4 + 4) * 4          # 13 floats read, xyz + t read and written
    log("noise step, %d Gaussians: %.3f ms (%.0f GB/s of the %d MB it must move), PyTorch %.3f ms" % (P, ms, nbytes / ms * 1e-6, nbytes >> 20, ms_t))

    def refine():
        model.flat.copy_(snapshot)
        calls[0] += 1
        return mcmc.relocate(model, opt, seed=1, call=calls[0])

    def refine_torch():
        with torch.no_grad():
            model.flat.copy_(snapshot)
            o = torch.sigmoid(model._opacity).flatten()
            dead = torch.nonzero(o <= 0.005).flatten()
            src = torch.multinomial(torch.where(o > 0.005, o, torch.zeros_like(o)), dead.numel(), replacement=True)
            for p in model.params.values():
                p[dead] = p[src]
            n = torch.bincount(src, minlength=P).clamp(max=50)[src] + 1
            model._opacity[dead] = torch.logit((1 - (1 - o[src]) ** (1.0 / n)).clamp(0.005, 1 - 2 ** -23)).unsqueeze(1)
    out = refine()
    ms, ms_t = _timed(refine, 5), _timed(refine_torch, 3)
    log("relocate, %d Gaussians (%d dead, %d sources): %.3f ms including the bucket restore; PyTorch (copy + opacity only, no scale "
        "ratio, no moments) %.3f ms" % (P, out["dead"], out["sources"], ms, ms_t))
    ms_copy = _timed(lambda: model.flat.copy_(snapshot), 5)
    log("  (the bucket restore alone: %.3f ms)" % ms_copy)
    sink = model.grad_sink()
    strat = mcmc.MCMCStrategy(model, opt, cap=P)
    log("regularisers: %.3f ms" % _timed(lambda: strat.add_regularizer_grads(sink), 20))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=600)
    ap.add_argument("--cap", type=int, default=3000)
    ap.add_argument("--start", type=int, default=2000)
    ap.add_argument("--refine-every", type=int, default=50)
    ap.add_argument("--bench", action="store_true")
    a = ap.parse_args()
    device = torch.device("cuda:0")
    if a.bench:
        bench(device)
    else:
        run(device, a.iterations, start=a.start, cap=a.cap, refine_every=a.refine_every)
