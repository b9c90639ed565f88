"""Full-size 8-bit frames to the training resolution on the GPU: what the reference's loader does per image on the host
(``loadCam`` -> ``PILtoTorch`` -> ``PIL.Image.resize``), byte for byte, as one kernel launch per chunk of frames.

    python examples/resize_frames.py                          synthetic 2704 x 2028 frames -> a half-size FrameStore (``-r 2``)
    python examples/resize_frames.py --frames 40 --rgba --background white --residency host
    python examples/resize_frames.py --bench                  kernel time per frame and GB/s, PIL on the host, resized_store frames/s

--bench (2704 x 2028 -> 1352 x 1014, RGB and RGBA): the kernel is timed with events on the stream over at least one second of work
after a warm-up, three times, in batches of 8 frames that rotate through 24 distinct source frames (395 / 526 MB: more than the
256 MB Infinity Cache, so the source comes from HBM); the median and the range are printed, for the fused kernel and for the
two-launch path in alternation.  GB/s = (bytes of the source frame + bytes of the result) / time; the share of peak is that over
the 8000 GB/s HBM peak bench.py uses.
"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

HBM_PEAK_GBS = 8000.0   # bench.py


def synthetic_frames(n, H, W, C, seed=0):
    """Smooth colour gradients with noise on top (and a soft round alpha mask): uint8 [n, H, W, C] on the host."""
    g = torch.Generator().manual_seed(seed)
    yy = torch.linspace(0, 1, H)[:, None].expand(H, W)
    xx = torch.linspace(0, 1, W)[None, :].expand(H, W)
    out = torch.empty((n, H, W, C), dtype=torch.uint8)
    for i in range(n):
        ph = i / max(n, 1)
        base = torch.stack([xx, yy, (xx + yy + ph) % 1.0], -1) * 200.0
        out[i, ..., :3] = (base + torch.randint(0, 56, (H, W, 3), generator=g)).to(torch.uint8)
        if C == 4:
            r2 = (xx - 0.5) ** 2 + (yy - 0.5) ** 2
            out[i, ..., 3] = ((1.0 - (r2 / 0.2).clamp(0, 1)) * 255.0).to(torch.uint8)
    return out


def timed(fns, min_seconds=1.0, repeats=3):
    """Seconds per call of each of ``fns``, alternating between them: events around enough calls for ``min_seconds``."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    counts = []
    for fn in fns:
        fn(); torch.cuda.synchronize()
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        counts.append(max(1, int(min_seconds / max(a.elapsed_time(b) * 1e-3, 1e-6)) + 1))
    out = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            a.record()
            for _ in range(counts[k]):
                fn()
            b.record(); torch.cuda.synchronize()
            out[k].append(a.elapsed_time(b) * 1e-3 / counts[k])
    return [sorted(o) for o in out]


def bench(dev):
    from fdgs import _capi
    from fdgs.resize import resize_frames, resized_store
    Hs, Ws, Hd, Wd, B, N = 2028, 2704, 1014, 1352, 8, 24
    result = {"device": torch.cuda.get_device_name(dev), "source": [Hs, Ws], "target": [Hd, Wd], "batch": B, "distinct_frames": N}
    for C, name in ((3, "rgb"), (4, "rgba")):
        host = synthetic_frames(4, Hs, Ws, C)
        src = host.repeat(N // 4, 1, 1, 1).to(dev)
        src += torch.arange(N, dtype=torch.uint8, device=dev)[:, None, None, None]      # 24 distinct frames
        if C == 4:
            src[..., 3] = host[0, ..., 3].to(dev)
        out = torch.empty((B, Hd, Wd, C), dtype=torch.uint8, device=dev)
        batches = [torch.arange(k * B, (k + 1) * B, dtype=torch.int32, device=dev) for k in range(N // B)]
        turn = [0]

        def fused():
            turn[0] += 1
            resize_frames(src, (Wd, Hd), batches[turn[0] % len(batches)], out)

        def two_launches():
            _capi.lib.fdgs_debug_frames_resize_path(1)
            try:
                fused()
            finally:
                _capi.lib.fdgs_debug_frames_resize_path(0)

        ref = resize_frames(src, (Wd, Hd), batches[0])
        _capi.lib.fdgs_debug_frames_resize_path(1)
        try:
            other = resize_frames(src, (Wd, Hd), batches[0])
        finally:
            _capi.lib.fdgs_debug_frames_resize_path(0)
        assert torch.equal(ref, other), "the two paths differ"
        del ref, other
        nbytes = (Hs * Ws + Hd * Wd) * C
        entry = {}
        for label, ts in zip(("fused", "two_launches"), timed([fused, two_launches])):
            per_frame = [t / B for t in ts]
            gbs = nbytes / per_frame[1] / 1e9
            entry[label] = {"us_per_frame": round(per_frame[1] * 1e6, 2), "us_range": [round(per_frame[0] * 1e6, 2), round(per_frame[-1] * 1e6, 2)],
                            "gb_per_s": round(gbs, 1), "frac_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4)}
        # PIL on the host, the code this replaces (single-threaded, one frame)
        try:
            from PIL import Image
            im = Image.fromarray(host[0].numpy(), "RGB" if C == 3 else "RGBA")
            im.resize((Wd, Hd))
            t0 = time.perf_counter()
            for _ in range(5):
                pil = im.resize((Wd, Hd))
            entry["pil_host_ms_per_frame"] = round((time.perf_counter() - t0) / 5 * 1e3, 2)
            got = resize_frames(host[:1].to(dev), (Wd, Hd))
            entry["equals_pil"] = bool(np.array_equal(got[0].cpu().numpy(), np.array(pil)))
        except ImportError:
            entry["pil_host_ms_per_frame"] = None
        # end to end: pinned full-size frames on the host -> a device-resident store
        pinned = synthetic_frames(16, Hs, Ws, C).pin_memory()
        resized_store(pinned, (Wd, Hd), chunk=8, device=dev); torch.cuda.synchronize()
        runs = []
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(4):
                resized_store(pinned, (Wd, Hd), chunk=8, device=dev)
            torch.cuda.synchronize()
            runs.append(4 * 16 / (time.perf_counter() - t0))
        runs.sort()
        entry["resized_store_frames_per_s"] = round(runs[1], 1)
        entry["resized_store_range"] = [round(runs[0], 1), round(runs[-1], 1)]
        entry["resized_store_host_gb_per_s"] = round(runs[1] * Hs * Ws * C / 1e9, 2)
        result[name] = entry
        del src, out, pinned
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--width", type=int, default=2704)
    ap.add_argument("--height", type=int, default=2028)
    ap.add_argument("--resolution", type=float, default=2, help="the reference's -r: 1, 2, 3, 4, 8, -1 or a target width")
    ap.add_argument("--rgba", action="store_true")
    ap.add_argument("--background", choices=("white", "black"), default=None, help="composite RGBA frames over it before the resize")
    ap.add_argument("--residency", choices=("device", "host"), default="device")
    ap.add_argument("--chunk", type=int, default=8)
    ap.add_argument("--bench", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resize_frames.py needs a GPU: the resize has no CPU path")
    dev = torch.device("cuda:0")
    if args.bench:
        return bench(dev)
    from fdgs.resize import resized_store, target_resolution
    res = int(args.resolution) if float(args.resolution).is_integer() else args.resolution
    fl = 0.54 * args.width
    size, scale, intr = target_resolution(args.width, args.height, res, cx=args.width / 2, cy=args.height / 2, fl_x=fl, fl_y=fl)
    frames = synthetic_frames(args.frames, args.height, args.width, 4 if (args.rgba or args.background) else 3)
    t0 = time.perf_counter()
    store = resized_store(frames, size, residency=args.residency, chunk=args.chunk, background=args.background, device=dev)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("source   %d frames %s uint8 (%.1f MB on the host)" % (len(frames), tuple(frames.shape[1:]), frames.numel() / 1e6))
    print("target   %d x %d (scale %.4g), intrinsics %s" % (size[0], size[1], scale, {k: round(v, 3) for k, v in intr.items()}))
    print("store    %d frames %s, residency %s, %.1f MB; built in %.3f s (%.0f frames/s, first call: includes start-up)" % (
        len(store), store.shape, store.residency, store.frames.numel() / 1e6, dt, len(frames) / dt))
    image = store[0]
    print("store[0] float32 %s, mean %.4f" % (tuple(image.shape), float(image.mean())))


if __name__ == "__main__":
    main()
