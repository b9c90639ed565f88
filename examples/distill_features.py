"""Per-Gaussian labels in and out of a 4D model.  Builds a synthetic rot_4d scene whose Gaussians carry ground-truth labels (k clusters
by position, one-hot, C = k), renders the label maps over a camera rig x a time sweep (fdgs.features.render_features), recovers the
per-Gaussian features from zeros from those maps alone (fit_features) and prints the per-pixel argmax accuracy on HELD-OUT
timestamps, over the pixels with alpha > 0.5; writes a diagnostic render of a per-Gaussian scalar, the mean time ``_t``, as .npy.

    python examples/distill_features.py --workload C2 --clusters 6 --times 4 --iterations 300 --out mean_time.npy
    python examples/distill_features.py --bench

--bench (one C3 view; median of 3 measurements of 20 launches each, after a warm-up): the feature pass forward and backward at C = 3
and C = 16, next to blend_fwd for the same view and to the only route that exists without the pass: ceil(C / 3) calls of
render(override_color=...), forward and backward, each a full preprocess, binning, sort and blend, the backward with the whole
geometry chain.
"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from prune_model import median3, stage_median3

RIG = ("rig0", "rig1", "rig2", "rig3")


def bench(dev):
    from fdgs import features, synth, train_host
    from fdgs.fused import raw_forward, raw_settings
    from fdgs.gaussian_renderer import render
    scene = synth.make_scene(synth.CONFIGS["C3"], seed=0, pose="rig0")
    model, pipe, bg = train_host.GaussianParams(scene, dev), train_host.PipelineFlags(), scene["bg"].to(dev)
    cam = train_host.SyntheticCamera(scene, dev)
    P, W, H = model.P, int(scene["W"]), int(scene["H"])
    rs, (xyz, feats, opacity, ts, scaling, scaling_t, rotation, rotation_r, pv) = raw_settings(cam, model, pipe, bg)
    res = {"workload": "C3", "P": P, "W": W, "H": H}
    with torch.no_grad():
        fwd = lambda: raw_forward(rs, xyz, feats, opacity, ts, scaling, scaling_t, rotation, rotation_r, pv, tile_cull=True)  # noqa: E731
        (R, _c, _f, _d, _T, radii, geom, binb, img, _cov, _om) = fwd()
        t, rng = stage_median3(fwd, ["blend_fwd"])
        res["blend_fwd_us"], res["blend_fwd_us_range"], res["num_rendered"] = t * 1e6, [rng[0] * 1e6, rng[1] * 1e6], R
        visible = int((radii > 0).sum())
    g = torch.Generator().manual_seed(0)
    for Cn in (3, 16):
        F = (2.0 * torch.rand(P, Cn, generator=g) - 1.0).to(dev)
        G = torch.randn(Cn, H, W, generator=g).to(dev)
        out, dF = torch.empty((Cn, H, W), device=dev), torch.zeros((P, Cn), device=dev)
        t, rng = median3(lambda: features.blend_pass(P, W, H, geom, binb, img, R, F, out=out))
        res["feature_fwd_us_C%d" % Cn], res["feature_fwd_us_range_C%d" % Cn] = t * 1e6, [rng[0] * 1e6, rng[1] * 1e6]
        # compulsory traffic: the image written once, the visible Gaussians' rows and blend records (32 of 48 bytes) read once
        res["feature_fwd_GBps_C%d" % Cn] = (4.0 * Cn * W * H + visible * (4.0 * Cn + 32.0)) / t * 1e-9
        t, rng = median3(lambda: features.blend_backward_pass(P, W, H, geom, binb, img, R, G, dF))
        res["feature_bwd_us_C%d" % Cn], res["feature_bwd_us_range_C%d" % Cn] = t * 1e6, [rng[0] * 1e6, rng[1] * 1e6]
        # ... the gradient image read once, the visible rows read, added to and written back
        res["feature_bwd_GBps_C%d" % Cn] = (4.0 * Cn * W * H + visible * (8.0 * Cn + 32.0)) / t * 1e-9
        # the route that exists without the pass: three channels per render() call
        cols = [F[:, j:j + 3].contiguous() for j in range(0, Cn, 3)]
        cols = [torch.cat([c, c.new_zeros(P, 3 - c.shape[1])], 1).requires_grad_(True) for c in cols]
        ups = [G[j:j + 3] for j in range(0, Cn, 3)]

        def route(backward):
            for c, u in zip(cols, ups):
                img3 = render(cam, model, pipe, bg, override_color=c)["render"]
                if backward:
                    (img3[:u.shape[0]] * u).sum().backward()
        with torch.no_grad():
            t, rng = median3(lambda: route(False), launches=5)
        res["override_color_fwd_us_C%d" % Cn], res["override_color_calls_C%d" % Cn] = t * 1e6, len(cols)
        t, rng = median3(lambda: route(True), launches=5)
        res["override_color_fwd_bwd_us_C%d" % Cn] = t * 1e6
        res["feature_fwd_bwd_us_C%d" % Cn] = res["feature_fwd_us_C%d" % Cn] + res["feature_bwd_us_C%d" % Cn]
        # the two routes agree on what both deliver (the override route composites the background: black here)
        with torch.no_grad():
            img3 = render(cam, model, pipe, torch.zeros(3, device=dev), override_color=cols[0])["render"]
        res["fwd_max_abs_diff_C%d" % Cn] = float((img3[:min(3, Cn)] - out[:min(3, Cn)]).abs().max())
    print(json.dumps(res))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2")
    ap.add_argument("--clusters", type=int, default=6, help="k: label clusters by position (k-means on the means); C = k")
    ap.add_argument("--times", type=int, default=4, help="training timestamps of the sweep; held-out ones lie between them")
    ap.add_argument("--iterations", type=int, default=300)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--out", default="mean_time.npy")
    ap.add_argument("--bench", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.bench:
        bench(dev)
        return
    from fdgs import features, playback, synth, train_host
    cfg = synth.CONFIGS[args.workload]
    scenes = [synth.make_scene(cfg, seed=0, pose=p) for p in RIG]
    if not scenes[0]["rot_4d"]:
        raise SystemExit("distill_features: workload %s is not rot_4d" % args.workload)
    model, pipe = train_host.GaussianParams(scenes[0], dev), train_host.PipelineFlags()
    P, k, T = model.P, args.clusters, float(scenes[0]["time_duration"])
    # ground truth: k clusters by position (a few Lloyd iterations from k of the means), one-hot
    xyz = model.get_xyz.detach()
    centres = xyz[torch.randperm(P, generator=torch.Generator().manual_seed(0))[:k].to(dev)].clone()
    for _ in range(10):
        label = torch.cdist(xyz, centres).argmin(1)
        for j in range(k):
            if bool((label == j).any()):
                centres[j] = xyz[label == j].mean(0)
    truth = torch.nn.functional.one_hot(label, k).float()
    n = max(2, args.times)
    train_t = [T * i / (n - 1) for i in range(n)]
    held_t = [0.5 * (a + b) for a, b in zip(train_t[:-1], train_t[1:])]
    base = [train_host.SyntheticCamera(s, dev) for s in scenes]
    train_cams = [playback.with_timestamp(c, t) for c in base for t in train_t]
    held_cams = [playback.with_timestamp(c, t) for c in base for t in held_t]
    with torch.no_grad():
        targets = [features.render_features(c, model, pipe, truth)["features"] for c in train_cams]
    fitted, history = features.fit_features(model, train_cams, targets, pipe, iterations=args.iterations, lr=args.lr,
                                            on_step=lambda it, v: print("[it %4d] loss %.3e" % (it, v)) if it % max(1, args.iterations // 10) == 0 else None)
    print("%s: %d Gaussians, %d labels, %d training views; loss %.3e -> %.3e" % (args.workload, P, k, len(train_cams), history[0], history[-1]))
    hit = cnt = 0
    with torch.no_grad():
        for c in held_cams:
            want = features.render_features(c, model, pipe, truth)
            got = features.render_features(c, model, pipe, fitted)["features"]
            m = want["alpha"][0] > 0.5
            hit += int((got.argmax(0)[m] == want["features"].argmax(0)[m]).sum())
            cnt += int(m.sum())
        print("held-out timestamps %s: per-pixel argmax accuracy %.4f over %d pixels with alpha > 0.5 (%d views)" % (
            ["%.3g" % t for t in held_t], hit / max(1, cnt), cnt, len(held_cams)))
        # a diagnostic render of a per-Gaussian scalar: the mean time of what a pixel shows (sum of w * _t, over alpha)
        d = features.render_features(held_cams[0], model, pipe, model.get_t.detach().reshape(P).contiguous())
        mean_t = torch.where(d["alpha"] > 0, d["features"] / d["alpha"].clamp_min(1e-12), torch.full_like(d["alpha"], float("nan")))[0]
    np.save(args.out, mean_t.cpu().numpy())
    print("%s: %s float32, mean time of the visible pixels %.4f (the view's timestamp: %.4f)" % (
        args.out, tuple(mean_t.shape), float(torch.nanmean(mean_t)), float(held_cams[0].timestamp)))


if __name__ == "__main__":
    main()
