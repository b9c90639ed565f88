"""Times view evaluation at C3 (300 k Gaussians, 1352 x 1014): (a) fdgs_eval_metrics alone per image (L1, PSNR, SSIM, MS-SSIM of
one 3 x 1014 x 1352 pair), (b) fdgs.metrics.evaluate over 50 views with one synchronisation at the end, next to 50 forward-only
render_raw calls, and (c) the PyTorch statement of the reference's training_report loop (train.py:311-326): the drop-in render(),
torch psnr and the reference's ssim (five grouped convolutions) on the GPU, then MS-SSIM on the CPU in float32 as torchmetrics
computes it there (reflection padding, one grouped convolution of the five moment maps, crop; 16 threads).  Prints one JSON line
of medians in ms.

    python tools/metrics_cost.py [--reps 50] [--views 50] [--ref-views 5]
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from regularizer_cost import _median_ms  # noqa: E402

BETAS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def _window32(C):
    g = torch.exp(-((torch.arange(11, dtype=torch.float32) - 5.0) ** 2) / (2 * 1.5 ** 2))
    g = g / g.sum()
    return (g[:, None] * g[None, :]).expand(C, 1, 11, 11).contiguous()


def msssim_cpu32(x, y):
    """torchmetrics 0.11.4's MS-SSIM as the reference runs it: float32 on the CPU, [1, C, H, W] inputs."""
    C = x.shape[1]
    w = _window32(C)
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    vals = []
    for s in range(len(BETAS)):
        xp, yp = F.pad(x, (5, 5, 5, 5), mode="reflect"), F.pad(y, (5, 5, 5, 5), mode="reflect")
        out = F.conv2d(torch.cat([xp, yp, xp * xp, yp * yp, xp * yp]), w, groups=C)
        mu1, mu2, e11, e22, e12 = out.split(1)
        s11, s22, s12 = e11 - mu1 ** 2, e22 - mu2 ** 2, e12 - mu1 * mu2
        upper, lower = 2 * s12 + c2, s11 + s22 + c2
        ssim_map = ((2 * mu1 * mu2 + c1) * upper) / ((mu1 ** 2 + mu2 ** 2 + c1) * lower)
        cs_map = upper / lower
        sim = torch.relu(ssim_map[..., 5:-5, 5:-5].mean())
        cs = torch.relu(cs_map[..., 5:-5, 5:-5].mean())
        vals.append(sim if s == len(BETAS) - 1 else cs)
        x, y = F.avg_pool2d(x, 2), F.avg_pool2d(y, 2)
    return float(torch.prod(torch.stack(vals) ** torch.tensor(BETAS)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--views", type=int, default=50)
    ap.add_argument("--ref-views", type=int, default=5)
    ap.add_argument("--config", default="C3")
    args = ap.parse_args()
    torch.set_num_threads(int(os.environ.get("OMP_NUM_THREADS", "16")))
    from fdgs import synth, train_host
    from fdgs.fused import render_raw
    from fdgs.gaussian_renderer import render
    from fdgs.metrics import evaluate, image_metrics

    dev = torch.device("cuda:0")
    scene = synth.make_scene(synth.CONFIGS[args.config], seed=0)
    H, W = scene["H"], scene["W"]
    out = {"config": args.config, "image": [3, H, W], "views": args.views, "threads": torch.get_num_threads()}
    gen = torch.Generator(device="cpu").manual_seed(7)
    img = (1.1 * torch.rand(3, H, W, generator=gen) - 0.05).to(dev)
    gt = torch.rand(3, H, W, generator=gen).to(dev)

    # (a) the metrics alone: per call (event pair around one call), and 50 back-to-back calls per image (launch gaps hidden)
    row = torch.empty(4, device=dev)
    out["metrics_call_ms"] = _median_ms(lambda: image_metrics(img, gt, out=row), args.reps)
    rows = torch.empty((50, 4), device=dev)

    def fifty():
        for v in range(50):
            image_metrics(img, gt, out=rows[v])
    out["metrics_per_image_ms"] = _median_ms(fifty, max(5, args.reps // 10)) / 50
    out["metrics_no_msssim_per_image_ms"] = _median_ms(lambda: [image_metrics(img, gt, msssim=False, out=rows[v]) for v in range(50)],
                                                       max(5, args.reps // 10)) / 50

    # (b) evaluate over the views, next to the forward alone
    model = train_host.GaussianParams(scene, dev)
    pipe, bg = train_host.PipelineFlags(), torch.tensor([0.1, 0.2, 0.3], device=dev)
    cams = [train_host.SyntheticCamera(scene, dev, timestamp=(v + 0.5) / args.views * scene["time_duration"]) for v in range(args.views)]
    gts = [torch.rand(3, H, W, generator=gen).to(dev) for _ in range(args.views)]

    def wall(fn, reps):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        return ts[len(ts) // 2]

    def forwards():
        with torch.no_grad():
            for c in cams:
                render_raw(c, model, pipe, bg)

    reps_b = max(3, args.reps // 10)
    out["forward_only_per_view_ms"] = wall(forwards, reps_b) / args.views
    out["evaluate_per_view_ms"] = wall(lambda: evaluate(model, cams, gts, pipe, bg), reps_b) / args.views
    out["evaluate_minus_forward_per_view_ms"] = out["evaluate_per_view_ms"] - out["forward_only_per_view_ms"]

    # (c) the reference's statement: render(), GPU psnr / ssim, CPU float32 MS-SSIM
    def reference_loop():
        acc = 0.0
        for c, g in zip(cams[:args.ref_views], gts[:args.ref_views]):
            with torch.no_grad():
                image = torch.clamp(render(c, model, pipe, bg)["render"], 0.0, 1.0)
                acc += float(train_host.l1_loss(image, g).double())
                mse = ((image - g) ** 2).view(3, -1).mean(1, keepdim=True)
                acc += float((20 * torch.log10(1.0 / torch.sqrt(mse))).mean().double())
                acc += float(train_host.ssim(image, g).double())
            acc += msssim_cpu32(image[None].cpu(), g[None].cpu())
        return acc

    out["reference_per_view_ms"] = wall(reference_loop, 3) / args.ref_views
    xc, yc = img.clamp(0, 1)[None].cpu(), gt[None].cpu()
    t0 = time.perf_counter()
    for _ in range(3):
        msssim_cpu32(xc, yc)
    out["reference_cpu_msssim_ms"] = (time.perf_counter() - t0) * 1e3 / 3
    out["reference_gpu_ssim_ms"] = _median_ms(lambda: train_host.ssim(img, gt), args.reps)
    out["speedup_per_view"] = out["reference_per_view_ms"] / out["evaluate_per_view_ms"]
    print(json.dumps({kk: (round(v, 4) if isinstance(v, float) else v) for kk, v in out.items()}))


if __name__ == "__main__":
    main()
