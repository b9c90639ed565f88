"""Optical-flow maps of a 4D model: renders a synthetic rot_4d scene over a fixed-camera time sweep with ``flow_to`` set to the next
frame and writes the flow maps as a .npy array [N - 1, 2, H, W] (pixels of motion to the next frame, blended: sum_i flow_i alpha_i T_i;
--normalise divides by the rendered alpha).

    python examples/render_flow.py --workload C2 --views 30 --out flow.npy
    python examples/render_flow.py --bench     the two flow kernels' time and GB/s next to the PyTorch operations they replace

--bench (C3 size: 300 k Gaussians): events on the stream over at least one second of work after a warm-up, three times; the median
and the range are printed.  Bytes per Gaussian: the forward reads 17 floats and writes 2 (76 B); the backward reads 19 and reads and
writes 16 (204 B).
"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def timed(fn, min_seconds=1.0, repeats=3):
    """Seconds per call of ``fn``: events around enough calls for ``min_seconds``."""
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


def torch_flow(cam, cam_to, model, W, H):
    """The PyTorch operations the forward kernel replaces: the 4D covariance as the reference's
    get_current_covariance_and_mean_offset builds it, two projections, a subtraction (raw parameters, float32, on the device)."""
    s4 = torch.exp(torch.cat([model._scaling, model._scaling_t], dim=1))
    ql, qr = torch.nn.functional.normalize(model._rotation), torch.nn.functional.normalize(model._rotation_r)
    a, b, c, d = ql.unbind(-1)
    p, q, r, s = qr.unbind(-1)
    Ml = torch.stack([a, -b, -c, -d, b, a, -d, c, c, d, a, -b, d, -c, b, a], dim=1).view(-1, 4, 4)
    Mr = torch.stack([p, q, r, s, -q, p, -s, r, -r, s, p, -q, -s, -r, q, p], dim=1).view(-1, 4, 4)
    L = (Ml @ Mr).flip(1, 2) * s4.unsqueeze(1)
    sig = L @ L.transpose(1, 2)
    w = sig[:, 0:3, 3] / sig[:, 3, 3:4]
    wh = torch.tensor([float(W), float(H)], device=w.device)
    pix, z = [], []
    for cm in (cam, cam_to):
        mean = model._xyz + w * (float(cm.timestamp) - model._t)
        hom = torch.cat([mean, torch.ones_like(mean[:, :1])], dim=1)
        h = hom @ cm.full_proj_transform
        z.append((hom @ cm.world_view_transform)[:, 2])
        pix.append(((h[:, 0:2] / (h[:, 3:4] + 1e-7) + 1.0) * wh - 1.0) * 0.5)
    ok = (z[0] > 0.2) & (z[1] > 0.2)
    return torch.where(ok.unsqueeze(1), pix[1] - pix[0], torch.zeros_like(pix[0]))


def bench(dev):
    from fdgs import playback, synth, train_host
    from fdgs.flow import model_flow
    scene = synth.make_scene(synth.CONFIGS["C3"], seed=0)
    model = train_host.GaussianParams(scene, dev)
    cam = train_host.SyntheticCamera(scene, dev)
    cam_to = playback.with_timestamp(cam, cam.timestamp + 0.1)
    P, H, W = int(scene["P"]), scene["H"], scene["W"]
    g = torch.randn(P, 2, generator=torch.Generator().manual_seed(0)).to(dev)

    def hip_fwd():
        with torch.no_grad():
            return model_flow(cam, cam_to, model, raw=True)

    def hip_fwd_bwd():
        model_flow(cam, cam_to, model, raw=True).backward(g)

    def torch_fwd():
        with torch.no_grad():
            return torch_flow(cam, cam_to, model, W, H)

    def torch_fwd_bwd():
        torch_flow(cam, cam_to, model, W, H).backward(g)

    diff = float((hip_fwd() - torch_fwd()).abs().max())
    t = {k: timed(f) for k, f in (("hip_forward", hip_fwd), ("hip_forward_backward", hip_fwd_bwd), ("torch_forward", torch_fwd),
                                  ("torch_forward_backward", torch_fwd_bwd))}
    med = lambda v: v[len(v) // 2]   # noqa: E731
    fwd_bytes, bwd_bytes = P * 76, P * 204
    res = {"workload": "C3", "P": P, "max_abs_diff_px": diff}
    for k, v in t.items():
        res[k + "_us"] = med(v) * 1e6
        res[k + "_us_range"] = [v[0] * 1e6, v[-1] * 1e6]
    bwd = max(med(t["hip_forward_backward"]) - med(t["hip_forward"]), 1e-9)
    res.update(hip_forward_GBps=fwd_bytes / med(t["hip_forward"]) * 1e-9, hip_backward_us=bwd * 1e6, hip_backward_GBps=bwd_bytes / bwd * 1e-9,
               forward_speedup=med(t["torch_forward"]) / med(t["hip_forward"]),
               forward_backward_speedup=med(t["torch_forward_backward"]) / med(t["hip_forward_backward"]))
    print(json.dumps(res))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2")
    ap.add_argument("--views", type=int, default=30, help="frames of the sweep: views - 1 flow maps")
    ap.add_argument("--normalise", action="store_true", help="divide the blended flow by the rendered alpha (where alpha > 1e-3)")
    ap.add_argument("--out", default="flow.npy")
    ap.add_argument("--bench", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.bench:
        bench(dev)
        return
    from fdgs import playback, synth, train_host
    from fdgs.fused import render_raw
    scene = synth.make_scene(synth.CONFIGS[args.workload], seed=0, rot_sigma=0.3)
    if not scene["rot_4d"]:
        raise SystemExit("render_flow: workload %s is not rot_4d: its Gaussians do not move" % args.workload)
    model, pipe, bg = train_host.GaussianParams(scene, dev), train_host.PipelineFlags(), scene["bg"].to(dev)
    cam = train_host.SyntheticCamera(scene, dev)
    path = playback.time_sweep(cam, 0.0, scene["time_duration"], max(2, args.views))
    maps = []
    with torch.no_grad():
        for here, there in zip(path[:-1], path[1:]):
            pkg = render_raw(here, model, pipe, bg, flow_to=there)
            flow = pkg["flow"]
            if args.normalise:
                flow = torch.where(pkg["alpha"] > 1e-3, flow / pkg["alpha"].clamp_min(1e-3), torch.zeros_like(flow))
            maps.append(flow.cpu())
    out = torch.stack(maps).numpy()
    np.save(args.out, out)
    print("%s: %s float32, max |flow| %.2f px" % (args.out, out.shape, float(np.abs(out).max())))


if __name__ == "__main__":
    main()
