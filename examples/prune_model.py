"""How far can a 4D model be cut before its renders change?  Loads a synthetic rot_4d scene as the model (--train N fine-tunes it
for N iterations on its own renders first), accumulates every Gaussian's blending weight over a camera rig x a time sweep
(fdgs.importance.accumulate), prunes copies of the model at several keep fractions (prune_by_contribution) and prints the number of
Gaussians left and the PSNR of the pruned renders against the unpruned model's renders; writes the ID map of the first view as .npy.

    python examples/prune_model.py --workload C2 --times 5 --keep 0.9 0.75 0.5 0.25 --out id_map.npy
    python examples/prune_model.py --bench

--bench (one C3 view; median of 3 measurements of 20 launches each, after a warm-up): the statistics pass, next to blend_fwd for the
same view and to the only route to a per-Gaussian weight sum without it -- a backward with a unit colour gradient (blend backward +
geometry backward), which yields weight_sum alone (no maximum, no counts, no ID map).
"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

RIG = ("rig0", "rig1", "rig2", "rig3")


def median3(fn, launches=20):
    """Seconds per launch of ``fn``: the median (and the range) of 3 event-timed runs of ``launches`` launches, after a warm-up."""
    for _ in range(3):
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


def stage_median3(fn, stages, launches=20):
    """Seconds per launch spent in the library's ``stages`` (HIP events around each stage's launch), median of 3 runs of ``launches``."""
    from fdgs import _capi
    out = []
    _capi.profile_enable(True, stages=stages)
    try:
        for _ in range(3):
            fn()
        for _ in range(3):
            torch.cuda.synchronize(); _capi.profile_reset()
            for _ in range(launches):
                fn()
            torch.cuda.synchronize()
            r = _capi.profile_read()
            out.append(sum(r[s][0] for s in stages) * 1e-3 / launches)
    finally:
        _capi.profile_enable(False)
    out.sort()
    return out[1], (out[0], out[2])


def bench(dev):
    from fdgs import importance, synth, train_host
    from fdgs.fused import raw_backward, raw_forward, raw_settings
    scene = synth.make_scene(synth.CONFIGS["C3"], seed=0, pose="rig0")
    model, pipe, bg = train_host.GaussianParams(scene, dev), train_host.PipelineFlags(), scene["bg"].to(dev)
    cam = train_host.SyntheticCamera(scene, dev)
    P, W, H = model.P, int(scene["W"]), int(scene["H"])
    rs, (xyz, feats, opacity, ts, scaling, scaling_t, rotation, rotation_r, pv) = raw_settings(cam, model, pipe, bg)
    res = {"workload": "C3", "P": P, "W": W, "H": H}
    with torch.no_grad():
        for tile_cull in (True, False):
            tag = "_tile_cull" if tile_cull else ""
            fwd = lambda: raw_forward(rs, xyz, feats, opacity, ts, scaling, scaling_t, rotation, rotation_r, pv, tile_cull=tile_cull)  # noqa: E731
            out = fwd()
            (R, _c, _f, _d, _T, radii, geom, binb, img, _cov, om) = out
            st = importance.ContributionStats(P, dev)
            ids = torch.empty((H, W), dtype=torch.int32, device=dev)
            all_out = dict(weight_sum=st.weight_sum, weight_max=st.weight_max, hits=st.hits, dominant=st.dominant, dominant_id=ids)
            t, rng = median3(lambda: importance.contribution_pass(P, W, H, geom, binb, img, R, **all_out))
            res["stats_pass_us" + tag], res["stats_pass_us_range" + tag] = t * 1e6, [rng[0] * 1e6, rng[1] * 1e6]
            t, _ = median3(lambda: importance.contribution_pass(P, W, H, geom, binb, img, R, weight_sum=st.weight_sum))
            res["stats_pass_sum_only_us" + tag] = t * 1e6
            t, _ = median3(lambda: importance.contribution_pass(P, W, H, geom, binb, img, R, dominant_id=ids))
            res["id_map_only_us" + tag] = t * 1e6
            t, rng = stage_median3(fwd, ["blend_fwd"])
            res["blend_fwd_us" + tag], res["blend_fwd_us_range" + tag] = t * 1e6, [rng[0] * 1e6, rng[1] * 1e6]
            # the route that exists without the pass: weight_sum = dL_dcolor[:, 0] of a backward with a unit colour gradient
            ones = torch.ones((3, H, W), dtype=torch.float32, device=dev)
            bwd = lambda: raw_backward(rs, xyz, om, radii, feats, opacity, ts, scaling, scaling_t, rotation, rotation_r, pv, geom, R, binb, img,  # noqa: E731
                                       ones, None, None, None, None, False)
            t, rng = median3(bwd)
            res["backward_call_us" + tag], res["backward_call_us_range" + tag] = t * 1e6, [rng[0] * 1e6, rng[1] * 1e6]
            t, rng = stage_median3(bwd, ["blend_bwd", "preprocess_bwd"])
            res["blend_bwd_plus_preprocess_bwd_us" + tag] = t * 1e6
            res["num_rendered" + tag] = R
            # the two routes agree on what both deliver
            st.zero_()
            importance.contribution_pass(P, W, H, geom, binb, img, R, weight_sum=st.weight_sum)
            d_colors = bwd()[1][:, 0]
            res["weight_sum_max_abs_diff" + tag] = float((st.weight_sum - d_colors).abs().max())
            res["weight_sum_max" + tag] = float(d_colors.abs().max())
    print(json.dumps(res))
    return res


def psnr(a, b):
    mse = float(((a - b) ** 2).mean())
    return float("inf") if mse == 0.0 else 10.0 * np.log10(1.0 / mse)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2")
    ap.add_argument("--times", type=int, default=5, help="timestamps of the sweep; every rig camera renders each")
    ap.add_argument("--keep", type=float, nargs="+", default=[0.9, 0.75, 0.5, 0.25])
    ap.add_argument("--train", type=int, default=0, help="fine-tune for this many iterations on the model's own renders first")
    ap.add_argument("--out", default="id_map.npy")
    ap.add_argument("--bench", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.bench:
        bench(dev)
        return
    from fdgs import harness, importance, layout, playback, synth, train_host
    from fdgs.fused import render_raw
    cfg = synth.CONFIGS[args.workload]
    scenes = [synth.make_scene(cfg, seed=0, pose=p) for p in RIG]
    if not scenes[0]["rot_4d"]:
        raise SystemExit("prune_model: workload %s is not rot_4d" % args.workload)
    pipe, bg = train_host.PipelineFlags(), scenes[0]["bg"].to(dev)
    cams = [c for s in scenes for c in playback.time_sweep(train_host.SyntheticCamera(s, dev), 0.0, s["time_duration"], max(1, args.times))]

    def renders(m):
        with torch.no_grad():
            return [render_raw(c, m, pipe, bg)["render"] for c in cams]

    model = train_host.GaussianParams(scenes[0], dev)
    if args.train > 0:
        opt = train_host.make_optimizer(model)
        harness.train(model, opt, cams, renders(model), pipe, bg, iterations=args.train, batch_size=min(4, len(cams)), densify_until_iter=0,
                      log_every=max(1, args.train // 5))
    full = renders(model)
    stats = importance.accumulate(model, cams, pipe, bg)
    torch.cuda.synchronize()
    P = model.P
    print("%s: %d Gaussians, %d views; never contributing: %d, never dominant: %d" % (
        args.workload, P, stats.views, int((stats.hits == 0).sum()), int((stats.dominant == 0).sum())))
    geo = (stats.weight_sum.clone(), stats.weight_max.clone(), stats.hits.clone(), stats.dominant.clone())
    for frac in args.keep:
        m = train_host.GaussianParams.from_raw(layout.raw_of(model), dev, **model.settings())   # a copy to cut down
        st = importance.ContributionStats(P, dev)
        st.weight_sum, st.weight_max, st.hits, st.dominant = (t.clone() for t in geo)
        rep = importance.prune_by_contribution(m, None, st, keep_fraction=frac)
        worst = min(psnr(a, b) for a, b in zip(full, renders(m)))
        print("keep %.2f: P %d -> %d, worst-view PSNR against the unpruned renders %.2f dB" % (frac, rep["P_old"], rep["P_new"], worst))
    ids = importance.id_map(model, cams[0], pipe, bg).cpu().numpy()
    np.save(args.out, ids)
    print("%s: %s int32, %d pixels without a contributor, %d distinct Gaussians" % (args.out, ids.shape, int((ids < 0).sum()), np.unique(ids[ids >= 0]).size))


if __name__ == "__main__":
    main()
