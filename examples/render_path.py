"""A camera path out of a model as 8-bit frames: trains a synthetic 4D scene for a few iterations (or loads a checkpoint), renders
a fixed-camera time sweep with fdgs.playback.render_path and writes the frames as a .npy array [N, H, W, 3] (no image codec needed:
numpy.load + any viewer, or ffmpeg -f rawvideo).

    python examples/render_path.py --workload C2 --iterations 100 --views 60 --out sweep.npy
    python examples/render_path.py --workload C2 --checkpoint chkpnt100.pth --views 60 --out sweep.npy      (saved with --save)
    python examples/render_path.py --bench      frames/s of render_path against the loop one writes without it, and the encode kernel

--bench (C3 size: 300 k Gaussians, 1352 x 1014, 120 views): every figure is timed with events on the stream over at least one second
of work after a warm-up, three times; the median and the range are printed.
"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def timed(fn, min_seconds=1.0, repeats=3):
    """Seconds per call of ``fn`` (which enqueues work and may read results back): events around enough calls for ``min_seconds``."""
    fn(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); torch.cuda.synchronize()
    n = max(1, int(min_seconds / max(a.elapsed_time(b) * 1e-3, 1e-6)) + 1)
    out = []
    for _ in range(repeats):
        a.record()
        for _ in range(n):
            fn()
        b.record(); torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e-3 / n)
    return sorted(out)


def bench(dev, views):
    from fdgs import playback, synth, train_host
    from fdgs.frames import FrameWriter, encode_frames
    from fdgs.fused import render_raw
    scene = synth.make_scene(synth.CONFIGS["C3"], seed=0)
    model, pipe, bg = train_host.GaussianParams(scene, dev), train_host.PipelineFlags(), scene["bg"].to(dev)
    train_host.spatial_sort(model)
    cam = train_host.SyntheticCamera(scene, dev)
    cams = playback.time_sweep(cam, 0.0, scene["time_duration"], views)
    H, W = scene["H"], scene["W"]
    writer = FrameWriter(views, H, W, residency="host", device=dev)

    def with_render_path():
        return playback.render_path(model, cams, pipe, bg, out=writer)["frames"]

    def by_hand():   # what a caller writes without it
        out = []
        with torch.no_grad():
            for c in cams:
                img = render_raw(c, model, pipe, bg)["render"]
                out.append(img.clamp(0, 1).mul(255).add(0.5).to(torch.uint8).permute(1, 2, 0).cpu())
        return out

    def render_only():
        with torch.no_grad():
            for c in cams:
                render_raw(c, model, pipe, bg)

    ta, tb, tr = timed(with_render_path), timed(by_hand), timed(render_only)
    # the encode kernel alone: a batch of 4 images into 4 frames (12 bytes in, 3 out per pixel)
    g = torch.Generator().manual_seed(0)
    images = torch.rand(4, 3, H, W, generator=g).to(dev)
    frames = torch.empty((4, H, W, 3), dtype=torch.uint8, device=dev)
    index = torch.arange(4, dtype=torch.int32, device=dev)
    te = timed(lambda: encode_frames(images, index, frames))
    nbytes = 4 * H * W * 15
    med = lambda t: t[len(t) // 2]   # noqa: E731
    res = {"workload": "C3", "views": views, "H": H, "W": W,
           "render_path_host_fps": views / med(ta), "render_path_host_fps_range": [views / ta[-1], views / ta[0]],
           "by_hand_fps": views / med(tb), "by_hand_fps_range": [views / tb[-1], views / tb[0]],
           "render_only_fps": views / med(tr),
           "encode_batch4_us": med(te) * 1e6, "encode_batch4_us_range": [te[0] * 1e6, te[-1] * 1e6],
           "encode_batch4_GBps": nbytes / med(te) * 1e-9, "encode_fraction_of_8TBps": nbytes / med(te) / 8e12}
    print(json.dumps(res))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2")
    ap.add_argument("--iterations", type=int, default=100, help="training iterations before the sweep (0: render the scene as generated)")
    ap.add_argument("--checkpoint", default=None, help="load this checkpoint (fdgs.checkpoint / the reference's layout) instead of training")
    ap.add_argument("--save", default=None, help="save a checkpoint of the trained model here")
    ap.add_argument("--views", type=int, default=None, help="frames of the sweep (default 60; --bench: 120)")
    ap.add_argument("--alpha", action="store_true", help="RGBA frames: the fourth byte is the rendered alpha")
    ap.add_argument("--depth", action="store_true", help="also write the grey depth frames (<out>.depth.npy)")
    ap.add_argument("--out", default="sweep.npy")
    ap.add_argument("--bench", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.bench:
        bench(dev, args.views or 120)
        return
    from fdgs import checkpoint, harness, playback, synth, train_host
    from fdgs.fused import render_raw
    cfg = synth.CONFIGS[args.workload]
    scene = synth.make_scene(cfg, seed=0)
    pipe, bg = train_host.PipelineFlags(), scene["bg"].to(dev)
    cam = train_host.SyntheticCamera(scene, dev)
    if args.checkpoint:
        model, opt, stats, it = checkpoint.load(args.checkpoint, dev, sh_degree=cfg.sh_degree, sh_degree_t=cfg.sh_degree_t,
                                                time_duration=[0.0, cfg.duration], force_sh_3d=cfg.force_sh_3d)
        print("loaded %s: %d Gaussians after %d iterations" % (args.checkpoint, model.P, it))
    else:
        target = train_host.GaussianParams(scene, dev)
        cams = [train_host.SyntheticCamera(scene, dev, timestamp=(v + 0.5) / 32 * scene["time_duration"]) for v in range(32)]
        with torch.no_grad():
            gts = [render_raw(c, target, pipe, bg)["render"].clone() for c in cams]
        model = train_host.GaussianParams(scene, dev)
        g = torch.Generator(device="cpu").manual_seed(1)
        with torch.no_grad():
            model.params["_features"].add_(0.3 * torch.randn(model.params["_features"].shape, generator=g).to(dev))
        opt = train_host.make_optimizer(model)
        on_save = (lambda it, m, o, st: checkpoint.save(args.save, m, o, it, st)) if args.save else None
        if args.iterations:
            harness.train(model, opt, cams, gts, pipe, bg, iterations=args.iterations, log_every=max(1, args.iterations // 4),
                          save_iterations=[args.iterations], on_save=on_save)
    path = playback.time_sweep(cam, 0.0, scene["time_duration"], args.views or 60)
    res = playback.render_path(model, path, pipe, bg, alpha=args.alpha, depth=args.depth)
    np.save(args.out, res["frames"].numpy())
    print("%s: %s uint8" % (args.out, tuple(res["frames"].shape)))
    if args.depth:
        np.save(args.out[:-4] + ".depth.npy", res["depth"].numpy())


if __name__ == "__main__":
    main()
