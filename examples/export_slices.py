"""Freeze frames of a 4D model: N timestamps of a checkpoint or of a synthetic scene, each as an ordinary 3D Gaussian scene in the
common 3DGS PLY layout (fdgs.slice.time_slice + save_ply), which any 3DGS viewer opens.

    python examples/export_slices.py --workload C2 --frames 8 --out frames/slice
    python examples/export_slices.py --workload C2 --checkpoint chkpnt100.pth --frames 8 --out frames/slice
    python examples/export_slices.py --bench      the slice kernels, the PyTorch operations they replace, render_slice against render()

--bench (C3 size: 300 k Gaussians, SH 3 + time 2, 1352 x 1014): every figure is timed with events on the stream over at least one
second of work after a warm-up, three times; the median and the range are printed.
"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from render_path import timed


def bench(dev):
    from fdgs import slice as fs, synth, train_host
    from fdgs.fused import render_raw
    scene = synth.make_scene(synth.CONFIGS["C3"], seed=0)
    model, pipe, bg = train_host.GaussianParams(scene, dev), train_host.PipelineFlags(), scene["bg"].to(dev)
    train_host.spatial_sort(model)
    t = scene["timestamp"]
    P, M = model.P, model.M
    sl = fs.time_slice(model, t)
    n = sl.n
    nblocks = 1 + min(model.active_sh_degree_t, 2) if (model.active_sh_degree > 2 and not model.force_sh_3d) else 1
    # what has to move: the 17 geometry floats of every Gaussian once; per live Gaussian its active SH blocks in, 48 floats of row, 10 of
    # geometry and the index out.  (The kernels read the geometry twice -- flags, then write: the second pass is in `slice_bytes_moved`.)
    must = P * 68 + n * (nblocks * 192 + 192 + 44)
    moved = must + P * 68
    outs = {k: torch.empty_like(getattr(sl, k)) for k in ("index", "xyz", "cov3D", "opacity", "shs")}
    n_live = torch.empty(1, dtype=torch.int32, device=dev)
    inputs = (model._xyz.detach(), model.get_features.detach(), model._opacity.detach(), model._t.detach(), model._scaling.detach(),
              model._scaling_t.detach(), model._rotation.detach(), model._rotation_r.detach() if model.rot_4d else None)
    settings = (model.active_sh_degree, model.active_sh_degree_t, 1.0, model.prefilter_var if model.prefilter_var > 0 else -1.0, t,
                model.time_duration[1] - model.time_duration[0], model.rot_4d, model.force_sh_3d)

    def kernels_only():   # the three launches, no host read
        fs._enqueue(inputs, settings, n, (outs["index"], outs["xyz"], outs["cov3D"], outs["opacity"], outs["shs"], None, None), n_live)

    # the PyTorch operations of render()'s compute_cov3D_python branch on the reference-style model: covariance, mean offset, marginal,
    # opacity, the boolean-mask gather of every tensor the rasterizer then takes (colour and SH left unfolded, as that branch leaves them)
    ref = train_host.ReferenceStyleModel(scene, dev)

    def torch_ops():
        with torch.no_grad():
            cov, delta = ref.get_current_covariance_and_mean_offset(1.0, t)
            means = ref.get_xyz + delta
            marginal = ref.get_marginal_t(t)
            opacity = ref.get_opacity * marginal
            mask = marginal[:, 0] > 0.05
            return means[mask], cov[mask], opacity[mask], ref.get_features[mask], ref.get_t[mask]

    cams = []
    for k, pose in enumerate(("axis", "rig0", "rig1", "rig2", "rig3", "axis", "rig0", "rig1")):
        sc = dict(scene)
        sc.update(synth.camera_for(pose, scene["W"], scene["H"]))
        cams.append(train_host.SyntheticCamera(sc, dev, timestamp=t))

    def eight_renders():
        with torch.no_grad():
            for c in cams:
                render_raw(c, model, pipe, bg)

    def slice_and_eight():
        s = fs.time_slice(model, t)
        for c in cams:
            fs.render_slice(s, c, bg)

    def eight_of_a_slice():
        for c in cams:
            fs.render_slice(sl, c, bg)

    tk, tc, tp = timed(kernels_only), timed(lambda: fs.time_slice(model, t)), timed(torch_ops)
    tr, ts_, t8 = timed(eight_renders), timed(slice_and_eight), timed(eight_of_a_slice)
    med = lambda v: v[len(v) // 2]   # noqa: E731
    rng = lambda v, f=1e6: [round(v[0] * f, 2), round(v[-1] * f, 2)]   # noqa: E731
    res = {"workload": "C3", "P": P, "M": M, "n_live": n, "live_fraction": round(n / P, 4),
           "slice_kernels_us": round(med(tk) * 1e6, 2), "slice_kernels_us_range": rng(tk),
           "slice_bytes_must_move": must, "slice_GBps_of_must_move": round(must / med(tk) * 1e-9, 1),
           "slice_bytes_moved": moved, "slice_GBps_of_moved": round(moved / med(tk) * 1e-9, 1),
           "time_slice_call_us": round(med(tc) * 1e6, 2), "time_slice_call_us_range": rng(tc),
           "torch_ops_us": round(med(tp) * 1e6, 2), "torch_ops_us_range": rng(tp),
           "render_x8_fps": round(8 / med(tr), 1), "render_x8_fps_range": [round(8 / tr[-1], 1), round(8 / tr[0], 1)],
           "slice_plus_render_slice_x8_fps": round(8 / med(ts_), 1), "slice_plus_render_slice_x8_fps_range": [round(8 / ts_[-1], 1), round(8 / ts_[0], 1)],
           "render_slice_x8_fps": round(8 / med(t8), 1), "render_slice_x8_fps_range": [round(8 / t8[-1], 1), round(8 / t8[0], 1)]}
    print(json.dumps(res))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2")
    ap.add_argument("--checkpoint", default=None, help="a checkpoint (fdgs.checkpoint / the reference's layout) instead of the synthetic scene")
    ap.add_argument("--frames", type=int, default=8, help="timestamps, evenly spaced over the model's duration")
    ap.add_argument("--scaling-modifier", type=float, default=1.0)
    ap.add_argument("--out", default="slice", help="prefix: <out>_0000.ply ...")
    ap.add_argument("--bench", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.bench:
        bench(dev)
        return
    from fdgs import checkpoint, synth, train_host
    from fdgs.slice import save_ply, time_slice
    cfg = synth.CONFIGS[args.workload]
    if args.checkpoint:
        model, _opt, _stats, it = checkpoint.load(args.checkpoint, dev, sh_degree=cfg.sh_degree, sh_degree_t=cfg.sh_degree_t,
                                                  time_duration=[0.0, cfg.duration], force_sh_3d=cfg.force_sh_3d)
        print("loaded %s: %d Gaussians after %d iterations" % (args.checkpoint, model.P, it))
    else:
        model = train_host.GaussianParams(synth.make_scene(cfg, seed=0), dev)
    t0, t1 = model.time_duration
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for k in range(args.frames):
        t = t0 + (t1 - t0) * (k + 0.5) / args.frames
        sl = time_slice(model, t, args.scaling_modifier, decompose=True)
        path = "%s_%04d.ply" % (args.out, k)
        save_ply(path, sl)
        print("%s: t = %.4f, %d of %d Gaussians" % (path, t, sl.n, model.P))


if __name__ == "__main__":
    main()
