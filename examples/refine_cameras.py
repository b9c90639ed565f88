"""Refine camera poses and per-camera time offsets through the rasterizer (fdgs.camera.LearnableCamera, fdgs_camera_backward).

A synthetic rot_4d scene stands in for a trained model: its Gaussians are frozen, the "ground truth" frames are rendered from the
true rig.  Every camera of the rig is then perturbed by an se(3) twist and a time offset, and ``torch.optim.Adam`` refines them on
the fused L1 + SSIM loss.  Printed: the pose error (|twist|) and the time error before and after.

    python examples/refine_cameras.py --cameras 4 --steps 150
    python examples/refine_cameras.py --bench     the camera kernels' time next to preprocess_bwd for the same view and P

--bench (C3: 300 k Gaussians, 1352 x 1014): per-stage HIP events (fdgs_profile_*) over repeated backward passes of one view.
Bytes per Gaussian of the camera pass: the accumulator record (48 of its 64 B), two of the three blend-record words (32 B), radii (4),
out_means3D (12), cov3D (24), the clamp byte, and for rot_4d ts / scales / scales_t / rotations / rotations_r (52); the SH row is read
only by the visible ones (12 M bytes each).
"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def bench(dev, repeats=30):
    from fdgs import _capi, synth, train_host
    from fdgs.camera import LearnableCamera
    from fdgs.fused import render_raw
    scene = synth.make_scene(synth.CONFIGS["C3"], seed=0, pose="rig0")
    model, pipe, bg = train_host.GaussianParams(scene, dev), train_host.PipelineFlags(), scene["bg"].to(dev)
    cam = LearnableCamera(train_host.SyntheticCamera(scene, dev))
    g = torch.randn(3, scene["H"], scene["W"], generator=torch.Generator().manual_seed(0)).to(dev) * 1e-2

    def step():
        pkg = render_raw(cam, model, pipe, bg)
        pkg["render"].backward(g)
        return pkg
    for _ in range(3):
        pkg = step()
    torch.cuda.synchronize()
    _capi.profile_reset()
    _capi.profile_enable(True, stages=("camera_bwd", "preprocess_bwd", "sh_bwd", "blend_bwd"))
    for _ in range(repeats):
        step()
    torch.cuda.synchronize()
    _capi.profile_enable(False)
    prof = _capi.profile_read()
    P, M = int(scene["P"]), int(scene["M"])
    vis = int((pkg["radii"] > 0).sum())
    us = {k: 1e3 * ms / max(n, 1) for k, (ms, n) in prof.items() if n}
    cam_bytes = P * (48 + 32 + 4 + 12 + 24 + 1 + 52) + vis * 12 * M
    res = {"workload": "C3", "P": P, "visible": vis, "camera_bwd_us": us["camera_bwd"], "preprocess_bwd_us": us["preprocess_bwd"],
           "sh_bwd_us": us.get("sh_bwd"), "blend_bwd_us": us.get("blend_bwd"),
           "camera_over_preprocess_bwd": us["camera_bwd"] / us["preprocess_bwd"], "camera_bytes": cam_bytes,
           "camera_GBps": cam_bytes / (us["camera_bwd"] * 1e-6) * 1e-9}
    print(json.dumps(res))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2")
    ap.add_argument("--gaussians", type=int, default=20000)
    ap.add_argument("--size", type=int, nargs=2, default=(400, 300), metavar=("W", "H"))
    ap.add_argument("--cameras", type=int, default=4)
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--twist", type=float, default=0.01, help="perturbation: rotation (rad); the translation is twice it (world units)")
    ap.add_argument("--time", type=float, default=0.02, help="perturbation of the timestamps, as a fraction of the duration")
    ap.add_argument("--bench", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.bench:
        bench(dev)
        return
    from fdgs import synth, train_host
    from fdgs.camera import LearnableCamera
    from fdgs.fused import render_raw
    from fdgs.loss import fused_l1_ssim
    cfg = synth.CONFIGS[args.workload]._replace(P=args.gaussians, W=args.size[0], H=args.size[1], sh_degree=3, sh_degree_t=1, s0=0.04, duration=6.0,
                                                rot_4d=True, gaussian_dim=4, force_sh_3d=False)
    poses = ["rig0", "rig1", "rig2", "rig3"]
    gen = torch.Generator().manual_seed(1)
    pipe = train_host.PipelineFlags()
    model, bg, rig = None, None, []
    for c in range(args.cameras):
        scene = synth.make_scene(cfg, seed=0, pose=poses[c % 4], timestamp_frac=0.3 + 0.4 * c / max(1, args.cameras - 1), rot_sigma=0.3)
        if model is None:
            model, bg = train_host.GaussianParams(scene, dev), scene["bg"].to(dev)
        true_cam = train_host.SyntheticCamera(scene, dev)
        with torch.no_grad():
            gt = render_raw(true_cam, model, pipe, bg)["render"].clone()
        cam = LearnableCamera(true_cam)
        d = torch.randn(6, generator=gen)
        with torch.no_grad():
            cam.pose_delta.copy_(torch.cat([args.twist * d[:3] / d[:3].norm(), 2 * args.twist * d[3:] / d[3:].norm()]).to(dev))
            cam.time_offset.fill_(args.time * cfg.duration * (1 if c % 2 == 0 else -1))
        rig.append((cam, gt))
    # frozen Gaussians: nothing of the model is handed to an optimizer; only the cameras' 7 numbers each move
    opt = torch.optim.Adam([{"params": [cam.pose_delta for cam, _ in rig], "lr": 5e-4},
                            {"params": [cam.time_offset for cam, _ in rig], "lr": args.time * cfg.duration / 30}])

    def errors():
        return (sum(float(cam.pose_delta.detach().norm()) for cam, _ in rig) / len(rig),
                sum(float(cam.time_offset.detach().abs()) for cam, _ in rig) / len(rig))
    pose0, time0 = errors()
    first = last = None
    for it in range(args.steps):
        opt.zero_grad(set_to_none=True)
        total = 0.0
        for cam, gt in rig:
            loss = fused_l1_ssim(render_raw(cam, model, pipe, bg)["render"], gt)
            loss.backward()
            total += float(loss.detach())
        opt.step()
        first = total / len(rig) if first is None else first
        last = total / len(rig)
        if it % 25 == 0 or it == args.steps - 1:
            p, t = errors()
            print("step %4d  loss %.5f  pose error %.5f  time error %.5f" % (it, last, p, t))
    pose1, time1 = errors()
    print("pose error %.5f -> %.5f, time error %.5f -> %.5f, loss %.5f -> %.5f" % (pose0, pose1, time0, time1, first, last))


if __name__ == "__main__":
    main()
