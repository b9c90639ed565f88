"""Times the 8-bit ground-truth path (fdgs.frames) at C3 (300 k Gaussians, 1352 x 1014, 4 views per step, bench.py's cameras):

* the decode launch alone for 4 RGB frames -- 16.5 MB read, 65.8 MB written -- as median time and GB/s, next to the HBM peak the
  bench's roofline uses;
* images/s of one StepPipeline loop fed from (a) resident float tensors, (b) a device-resident FrameStore, (c) a host-resident
  FrameStore with prefetch, (d) float tensors in pinned host memory uploaded per step as the reference does (train.py:106).
  (a) and (b) run three times each, alternating; ``margin`` is the range (max - min) of (a)'s three runs and ``b_within_margin`` says
  whether (b)'s median is no further below (a)'s than that; ``store_batch_ms`` is what ``store.batch`` puts in front of a step on the
  caller's stream (index upload + decode).  (c) and (d) once, with the bus bandwidth their rate implies.

Every leg starts from the same model and draws the same frames in the same order.  Prints one JSON line.

    python tools/frames_cost.py [--steps 600] [--warmup 20] [--reps 50] [--frames 16]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from regularizer_cost import _median_ms  # noqa: E402

HBM_PEAK_GBS = 8000.0   # bench.py's roofline peak (MI355X HBM3E)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--config", default="C3")
    args = ap.parse_args()
    from fdgs import synth, train_host
    from fdgs.frames import FrameStore, decode_frames
    from fdgs.pipeline import StepPipeline

    dev = torch.device("cuda:0")
    scene = synth.make_scene(synth.CONFIGS[args.config], seed=0)
    H, W, B, N = scene["H"], scene["W"], 4, max(8, args.frames)
    out = {"config": args.config, "image": [3, H, W], "views_per_step": B, "frames": N, "steps": args.steps}
    u8 = torch.randint(0, 256, (N, H, W, 3), generator=torch.Generator().manual_seed(1234), dtype=torch.uint8)
    u8_dev = u8.to(dev)

    # the decode launch alone
    dst = torch.empty((B, 3, H, W), device=dev)
    index = torch.tensor([5, 2, 7, 0], dtype=torch.int32, device=dev)
    moved = B * H * W * 3 * (1 + 4)
    ms = _median_ms(lambda: decode_frames(u8_dev, index, dst), args.reps)
    out["decode_ms"], out["decode_bytes"] = ms, moved
    out["decode_gbs"] = moved / (ms * 1e-3) / 1e9
    out["hbm_peak_gbs"], out["decode_frac_of_hbm_peak"] = HBM_PEAK_GBS, moved / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS
    ten = _median_ms(lambda: [decode_frames(u8_dev, index, dst) for _ in range(10)], max(5, args.reps // 5)) / 10
    out["decode_back_to_back_ms"], out["decode_back_to_back_gbs"] = ten, moved / (ten * 1e-3) / 1e9

    # what a step pays in front of it: store.batch = the 16-byte index upload + the decode, on the caller's stream
    probe = FrameStore(u8_dev, slots=2 * B)
    out["store_batch_ms"] = _median_ms(lambda: probe.batch([5, 2, 7, 0]), args.reps)
    del probe

    # the step loop
    q = (u8_dev.float() / torch.tensor(255.0, device=dev)).permute(0, 3, 1, 2).contiguous()      # [N, 3, H, W] resident floats
    q_host = q.cpu().pin_memory()
    cams = [train_host.SyntheticCamera(dict(scene, **synth.camera_for("rig%d" % (b % 4), W, H)), dev,
                                       timestamp=(b + 0.5) / B * scene["time_duration"]) for b in range(B)]   # bench.py's views
    pipe, bg = train_host.PipelineFlags(), scene["bg"].to(dev)
    batches = [[(B * k + j) % N for j in range(B)] for k in range(args.warmup + args.steps + 1)]

    def leg(kind):
        model = train_host.GaussianParams(scene, dev)
        opt = train_host.make_optimizer(model)
        train_host.spatial_sort(model, opt)
        sp = StepPipeline(model, opt, world_size=1, lambda_dssim=0.2)
        store = None
        if kind in ("device", "host"):
            store = FrameStore(u8, residency=kind, device=dev)
            store.reserve(B)

        def step(k):
            idx = batches[k]
            if kind == "float":
                gts = [q[i] for i in idx]
            elif kind == "pinned_float":
                gts = [q_host[i].to(dev, non_blocking=True) for i in idx]
            else:
                gts = store.batch(idx)
                store.prefetch(batches[k + 1])
            sp.step(cams, gts, pipe, bg)
        if store is not None:
            store.prefetch(batches[0])
        for k in range(args.warmup):
            step(k)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(args.warmup, args.warmup + args.steps):
            step(k)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        del sp, opt, model, store
        return args.steps * B / dt, dt

    a, b = [], []
    for _ in range(3):
        a.append(leg("float")[0])
        b.append(leg("device")[0])
    c, c_dt = leg("host")
    d, _ = leg("pinned_float")
    med = lambda v: sorted(v)[len(v) // 2]
    out["a_float_resident_ips"], out["b_store_device_ips"] = a, b
    out["a_median_ips"], out["b_median_ips"] = med(a), med(b)
    out["margin_ips"] = max(a) - min(a)
    out["b_minus_a_ips"] = med(b) - med(a)
    out["b_within_margin"] = bool(med(b) >= med(a) - (max(a) - min(a)))
    out["timed_seconds_per_leg"] = c_dt
    out["c_store_host_prefetch_ips"], out["c_bus_gbs"] = c, c * H * W * 3 / 1e9
    out["d_pinned_float_upload_ips"], out["d_bus_gbs"] = d, d * H * W * 3 * 4 / 1e9
    print(json.dumps({k: ([round(x, 1) for x in v] if isinstance(v, list) and v and isinstance(v[0], float)
                          else round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}))


if __name__ == "__main__":
    main()
