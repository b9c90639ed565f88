"""How small does a 4D model store, and what does that cost in the image?  Builds a synthetic rot_4d scene as the model (--prune F
first cuts it to the fraction F of its Gaussians by contribution), compresses it at several codebook sizes / bit settings
(fdgs.compress), writes each as .npz and prints the file size, its ratio to the float32 checkpoint of the same model, and the mean /
worst PSNR and mean SSIM of the decompressed model's renders against the uncompressed model's over a camera rig x a time sweep.

    python examples/compress_model.py --workload C3 --P 60000 --times 3 --codebooks 256 4096 --out /tmp/model
    python examples/compress_model.py --bench

--bench (C3-sized rows: N = 300 000, D = 141, K = 4096; the median and range of 3 event-timed measurements of several launches each,
after a warm-up): fdgs_kmeans_assign and its TFLOP/s counted as 2 N K D / t, the same assignment as a chunked torch.cdist + argmin,
fdgs_kmeans_update, and the decode of the SH segment in GB/s (bytes written + bytes read).
"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

RIG = ("rig0", "rig1", "rig2", "rig3")


def median3(fn, launches):
    """Seconds per launch of ``fn``: the median (and the range) of 3 event-timed runs of ``launches`` launches, after a warm-up."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record(); torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e-3 / launches)
    out.sort()
    return out[1], (out[0], out[2])


def cdist_argmin(x, c, chunk=16384):
    """The PyTorch route: an N x K distance matrix, materialised ``chunk`` rows at a time."""
    return torch.cat([torch.cdist(x[i:i + chunk], c).argmin(dim=1) for i in range(0, x.shape[0], chunk)])


def bench(dev, N=300_000, D=141, K=4096):
    from fdgs import _capi, compress
    g = torch.Generator().manual_seed(0)
    centres = torch.randn(K, D, generator=g)
    x = (centres[torch.randint(0, K, (N,), generator=g)] + 0.5 * torch.randn(N, D, generator=g)).to(dev)
    c = x[torch.randperm(N, generator=g)[:K].to(dev)].contiguous()
    w = torch.rand(N, generator=g).to(dev)
    scratch = _capi.scratch(_capi.lib.fdgs_kmeans_scratch_bytes(N, K), dev, floor=1)
    res = {"N": N, "D": D, "K": K, "runs": 3}
    t, rng = median3(lambda: compress.assign(x, c, scratch=scratch), 5)
    res["assign_ms"], res["assign_ms_range"], res["assign_tflops"] = t * 1e3, [rng[0] * 1e3, rng[1] * 1e3], 2.0 * N * K * D / t * 1e-12
    t, rng = median3(lambda: cdist_argmin(x, c), 3)
    res["cdist_argmin_ms"], res["cdist_argmin_ms_range"] = t * 1e3, [rng[0] * 1e3, rng[1] * 1e3]
    index, _ = compress.assign(x, c, scratch=scratch)
    ref = cdist_argmin(x, c)
    res["rows_differing_from_cdist"] = int((index.long() != ref).sum())
    cb = c.clone()
    t, rng = median3(lambda: compress.update(x, index, cb, weights=w, scratch=scratch), 5)
    res["update_ms"], res["update_ms_range"] = t * 1e3, [rng[0] * 1e3, rng[1] * 1e3]
    # decode of the SH segment: [N, 3 + D] floats written; a 16-bit DC triple, an index and (from cache) a codebook row read per Gaussian
    dc = torch.randint(0, 1 << 15, (N, 3), dtype=torch.int16, device=dev)
    out = torch.empty(N * (3 + D), dtype=torch.float32, device=dev)
    t, rng = median3(lambda: compress.decode_into(out, N, 3, 16, dc, [0, 0, 0], [1e-4] * 3, rows=c, index=index), 20)
    moved = N * ((3 + D) * 4 + 6 + 4) + K * D * 4
    res["decode_sh_us"], res["decode_sh_us_range"], res["decode_sh_gbs"] = t * 1e6, [rng[0] * 1e6, rng[1] * 1e6], moved / t * 1e-9
    print(json.dumps(res))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C3")
    ap.add_argument("--P", type=int, default=60000, help="Gaussians of the synthetic model")
    ap.add_argument("--size", type=int, nargs=2, default=[676, 507], help="W H of the renders")
    ap.add_argument("--times", type=int, default=3, help="timestamps of the sweep; every rig camera renders each")
    ap.add_argument("--codebooks", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--prune", type=float, default=0.0, help="keep this fraction of the Gaussians by contribution first (0: no pruning)")
    ap.add_argument("--out", default="compressed_model", help="prefix of the files written")
    ap.add_argument("--bench", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.bench:
        bench(dev)
        return
    from fdgs import checkpoint, compress, importance, metrics, playback, synth, train_host
    from fdgs.fused import render_raw
    cfg = synth.CONFIGS[args.workload]
    W, H = args.size
    scenes = [synth.make_scene(cfg, seed=0, P=args.P, W=W, H=H, pose=p) for p in RIG]
    if not scenes[0]["rot_4d"]:
        raise SystemExit("compress_model: workload %s is not rot_4d" % args.workload)
    pipe, bg = train_host.PipelineFlags(), scenes[0]["bg"].to(dev)
    cams = [c for s in scenes for c in playback.time_sweep(train_host.SyntheticCamera(s, dev), 0.0, s["time_duration"], max(1, args.times))]

    def renders(m):
        with torch.no_grad():
            return [render_raw(c, m, pipe, bg)["render"] for c in cams]

    model = train_host.GaussianParams(scenes[0], dev)
    stats = importance.accumulate(model, cams, pipe, bg)
    if args.prune > 0.0:
        rep = importance.prune_by_contribution(model, None, stats, keep_fraction=args.prune)
        print("pruned by contribution: P %d -> %d" % (rep["P_old"], rep["P_new"]))
    full = renders(model)
    ckpt = args.out + "_float32.pth"
    checkpoint.save(ckpt, model, None, 0)
    ckpt_bytes = os.path.getsize(ckpt)
    print("%s: %d Gaussians, M = %d, %d views of %d x %d; float32 checkpoint %d B (%d B per Gaussian)" % (
        args.workload, model.P, model.M, len(cams), W, H, ckpt_bytes, ckpt_bytes // max(model.P, 1)))
    settings = [("K=%d, default bits" % k, dict(codebook_size=k)) for k in args.codebooks]
    settings.append(("K=%d, contribution-weighted" % args.codebooks[-1], dict(codebook_size=args.codebooks[-1], weights=stats.weight_sum)))
    settings.append(("K=%d, 16-bit everywhere" % args.codebooks[-1],
                     dict(codebook_size=args.codebooks[-1], bits={"_opacity": 16, "_rotation": 16, "_rotation_r": 16})))
    settings.append(("no codebook, default bits", dict(codebook_size=None)))
    for i, (label, kw) in enumerate(settings):
        cm = compress.compress(model, iters=args.iters, **kw)
        path = "%s_%d.npz" % (args.out, i)
        compress.save(path, cm)
        back = compress.decompress(compress.load(path), dev)
        rows = torch.stack([metrics.image_metrics(a, b, msssim=False) for a, b in zip(renders(back), full)]).cpu().numpy()
        size = os.path.getsize(path)
        print("%-32s %10d B  1 / %5.2f of the checkpoint  (payload %d B)  PSNR mean %.2f worst %.2f dB  SSIM mean %.4f" % (
            label, size, ckpt_bytes / size, compress.nbytes(cm), float(rows[:, 1].mean()), float(rows[:, 1].min()), float(rows[:, 2].mean())))


if __name__ == "__main__":
    main()
