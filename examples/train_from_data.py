"""Training from a dataset folder: fdgs.scene reads it, fdgs.seed thins its point cloud and writes the initial model.

    python examples/train_from_data.py --steps 300          # writes a tiny dataset first, then trains from it
    python examples/train_from_data.py --data /path/to/folder --steps 3000
    python examples/train_from_data.py --bench              # thinning + init at 2 M points next to numpy / PyTorch

Without ``--data`` the dataset is made here from a fdgs.synth scene, in the layout of a converted DyNeRF / D-NeRF folder: PNG frames,
``transforms_train.json`` / ``transforms_test.json`` (OpenGL camera-to-world matrices, ``camera_angle_x``, a ``time`` per frame) and a
``points3d.ply`` with a ``time`` column.  Everything after that only sees the folder.
"""
import argparse, json, math, os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def write_dataset(folder, dev, views=8, test_views=2, width=64, height=48, cloud_points=600, seed=0):
    """A synthetic 4D scene rendered from ``views`` + ``test_views`` cameras on an arc around it, one timestamp each, as a dataset folder.
    Returns the scene's time span."""
    from PIL import Image
    from fdgs import seed as seed_mod, synth, train_host
    from fdgs.fused import render_raw
    cfg = synth.SceneConfig("tiny", max(1500, cloud_points), width, height, 3, 0, 0.05, 1.0, True, 4, True)
    scene = synth.make_scene(cfg, seed=seed)
    target = train_host.GaussianParams(scene, dev)
    pipe, bg = train_host.PipelineFlags(), torch.zeros(3, device=dev)
    os.makedirs(folder, exist_ok=True)
    n = views + test_views
    test_at = set(int(round((k + 0.5) * n / test_views)) % n for k in range(test_views)) if test_views else set()
    splits = {"train": [], "test": []}
    for v in range(n):
        a = (v / max(n - 1, 1) - 0.5) * 1.2                                  # +-0.6 rad around the subject, 4 units away, looking at it
        cam = synth.make_camera(width, height, yaw=-a, shift=(4.0 * math.sin(a), 0.3 * math.sin(3.0 * a), 4.0 - 4.0 * math.cos(a)))
        stamp = (v + 0.5) / n * cfg.duration
        view = train_host.SyntheticCamera(dict(scene, **cam, H=height, W=width), dev, timestamp=stamp)
        with torch.no_grad():
            img = render_raw(view, target, pipe, bg)["render"]
        split = "test" if v in test_at else "train"
        name = "%s/r_%03d" % (split, len(splits[split]))
        os.makedirs(os.path.join(folder, split), exist_ok=True)
        Image.fromarray((img.clamp(0, 1) * 255 + 0.5).to(torch.uint8).permute(1, 2, 0).cpu().numpy(), "RGB").save(os.path.join(folder, name + ".png"))
        c2w = np.linalg.inv(cam["world_view_transform"].double().numpy().T)   # COLMAP axes ...
        c2w[:3, 1:3] *= -1                                                   # ... to the OpenGL axes the files use
        splits[split].append({"file_path": name, "time": stamp, "transform_matrix": c2w.tolist()})
    for split, frames in splits.items():
        with open(os.path.join(folder, "transforms_%s.json" % split), "w") as f:
            json.dump({"camera_angle_x": cam["FoVx"], "frames": frames}, f)
    # the cloud: some of the scene's own Gaussians (a COLMAP reconstruction per frame would give such points), jittered
    g = torch.Generator().manual_seed(seed + 1)
    pick = torch.randperm(scene["means3D"].shape[0], generator=g)[:cloud_points]
    xyz = scene["means3D"][pick] + 0.01 * torch.randn((len(pick), 3), generator=g)
    rgb = (0.5 + seed_mod.C0 * scene["shs"][pick, 0, :]).clamp(0, 1)
    seed_mod.save_ply(os.path.join(folder, "points3d.ply"), seed_mod.PointCloud(xyz, rgb, scene["ts"][pick].reshape(-1)))
    return (0.0, float(cfg.duration))


def run(folder, dev, views=8, test_views=2, width=64, height=48, cloud_points=600, num_pts=400, steps=300, batch_size=4, data=None, log=print):
    from fdgs import metrics, scene as scene_mod, train_host
    from fdgs.harness import FrameShard
    from fdgs.pipeline import StepPipeline
    if data is None:
        time_duration = write_dataset(folder, dev, views, test_views, width, height, cloud_points)
    else:
        folder, time_duration = data, (0.0, 1.0)
    sc = scene_mod.Scene(folder, white_background=False, eval=True, time_duration=time_duration, num_pts=num_pts)
    cams, store = sc.cameras("train", dev), sc.frames("train", device=dev)
    tcams, tstore = sc.cameras("test", dev), (sc.frames("test", device=dev) if sc.test_infos else None)
    model = sc.create_model(sh_degree=3, gaussian_dim=4, rot_4d=True, force_sh_3d=True, device=dev)
    thinned = model.P
    log("%d train / %d test views at %dx%d, cloud %d -> %d points, cameras_extent %.3f" % (
        len(cams), len(tcams), cams[0].image_width, cams[0].image_height, 0 if sc.cloud is None else len(sc.cloud), thinned, sc.cameras_extent))
    pipe, bg = train_host.PipelineFlags(), torch.zeros(3, device=dev)
    held_cams, held = (tcams, tstore) if tcams else (cams, store)
    before = metrics.evaluate(model, held_cams, held, pipe, bg, msssim=False)["psnr"]
    opt = train_host.make_optimizer(model)
    sp = StepPipeline(model, opt)
    batch_size = min(batch_size, len(cams))
    store.reserve(batch_size)
    shard = iter(FrameShard(len(cams), batch_size))
    first = last = None
    torch.cuda.synchronize(dev); t0 = time.time()
    for k in range(steps):
        idx = next(shard)
        _, losses = sp.step([cams[i] for i in idx], store.batch(idx), pipe, bg)
        if k == 0 or k == steps - 1 or (k + 1) % max(1, steps // 5) == 0:
            last = float(torch.stack(losses).mean())
            first = last if first is None else first
            log("[step %4d] loss %.5f" % (k + 1, last))
    torch.cuda.synchronize(dev)
    after = metrics.evaluate(model, held_cams, held, pipe, bg, msssim=False)["psnr"]
    log("%d steps in %.2f s; held-out PSNR %.2f dB -> %.2f dB" % (steps, time.time() - t0, before, after))
    return dict(train_views=len(cams), test_views=len(tcams), image_size=(cams[0].image_width, cams[0].image_height),
                cloud_points=0 if sc.cloud is None else len(sc.cloud), thinned_points=thinned, model_rows=model.P, first_loss=first,
                last_loss=last, psnr_untrained=before, psnr_trained=after)


def bench(dev, N=2_000_000, num_pts=100_000, repeats=5, log=print):
    """Thinning and initialisation at N points: HIP against the numpy / PyTorch formulation of the same steps.  Bytes: what each
    step has to move once (inputs read + outputs written), over the measured time."""
    from fdgs import seed
    from fdgs.knn import distCUDA2
    g = torch.Generator().manual_seed(0)
    cloud = seed.PointCloud(torch.rand((N, 3), generator=g) * 2.6 - 1.3, torch.rand((N, 3), generator=g), torch.rand(N, generator=g)).to(dev)

    def timed(fn):
        fn(); torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(repeats):
            out = fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / repeats, out
    t_to, th = timed(lambda: seed.thin_to(cloud, num_pts))
    t_thin, th = timed(lambda: seed.thin(cloud, th.cell, th.cell_t))
    M = len(th.cloud)
    d2 = distCUDA2(th.cloud.xyz)
    kw = dict(sh_degree=3, gaussian_dim=4, rot_4d=True, force_sh_3d=True, time_duration=(0.0, 1.0), dist2=d2)
    t_init, model = timed(lambda: seed.create_from_pcd(th.cloud, **kw))
    thin_bytes = N * 28 + M * (28 + 16)
    init_bytes = M * (28 + 4) + model.flat.numel() * 4

    def torch_init():
        P = len(th.cloud)
        feats = torch.zeros((P, 16, 3), device=dev)
        feats[:, 0, :] = (th.cloud.rgb - 0.5) / seed.C0
        sc = torch.log(torch.sqrt(torch.clamp_min(d2, 1e-7)))[..., None].repeat(1, 3)
        rot = torch.zeros((P, 4), device=dev); rot[:, 0] = 1
        return dict(_xyz=th.cloud.xyz, _features=feats, _scaling=sc, _rotation=rot, _opacity=torch.full((P, 1), -2.1972246, device=dev),
                    _t=th.cloud.t[:, None], _scaling_t=torch.full((P, 1), -0.804719, device=dev), _rotation_r=rot.clone())
    from fdgs.train_host import GaussianParams
    t_torch, _ = timed(lambda: GaussianParams.from_raw(torch_init(), dev, max_sh_degree=3, gaussian_dim=4, rot_4d=True, force_sh_3d=True))
    xyz = cloud.xyz.cpu().numpy()
    t0 = time.perf_counter()
    mask = np.random.default_rng(0).integers(0, N, num_pts)      # the reference's draw with replacement (plus the three gathers)
    _ = xyz[mask], cloud.rgb.cpu().numpy()[mask], cloud.t.cpu().numpy()[mask]
    t_np = time.perf_counter() - t0
    out = dict(N=N, num_pts=num_pts, thinned=M, thin_ms=t_thin * 1e3, thin_gbps=thin_bytes / t_thin * 1e-9, thin_to_ms=t_to * 1e3,
               init_ms=t_init * 1e3, init_gbps=init_bytes / t_init * 1e-9, torch_init_ms=t_torch * 1e3, numpy_randint_ms=t_np * 1e3)
    log(json.dumps(out))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", default=None, help="a dataset folder (transforms_train.json ...); default: write a tiny synthetic one")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--test-views", type=int, default=4)
    ap.add_argument("--size", type=int, nargs=2, default=(160, 120), metavar=("W", "H"))
    ap.add_argument("--cloud-points", type=int, default=3000)
    ap.add_argument("--num-pts", type=int, default=1500)
    ap.add_argument("--batch-size", type=int, default=4)
    ap.add_argument("--bench", action="store_true", help="time thinning + init at 2 M points next to the numpy / PyTorch formulation")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.bench:
        bench(dev)
        return
    with tempfile.TemporaryDirectory() as tmp:
        run(os.path.join(tmp, "dataset"), dev, args.views, args.test_views, args.size[0], args.size[1], args.cloud_points, args.num_pts,
            args.steps, args.batch_size, data=args.data)


if __name__ == "__main__":
    main()
