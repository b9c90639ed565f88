"""Two 4D scenes in one: scene B is cut out with a box mask, placed into scene A at half size, rotated, and retimed to start mid-way
(fdgs.edit: extract, Similarity, transform, merge); the merged model is rendered over a time sweep and the frames are written as .npy.

    python examples/compose_scenes.py --frames 16 --out frames/composed
    python examples/compose_scenes.py --bench      the two kernels of fdgs_model_transform, a torch copy of the same bytes, the torch formulation

--bench (C3 size: 300 k Gaussians, 48 SH coefficients, rot_4d, the closed-form path s == a): every figure is timed with events on the
stream over at least one second of work after a warm-up, three times; the median and the range are printed.  The SH kernel's time is
the call with SH rows minus the call without them (the C entry always runs the geometry pass); the argument structs are built once,
outside the timed loop.
"""
import argparse, ctypes, json, math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from render_path import timed


def rot_axis(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def bench(dev):
    from fdgs import _capi, edit, synth, train_host
    scene = synth.make_scene(synth.CONFIGS["C3"], seed=0)
    model = train_host.GaussianParams(scene, dev)
    P, M = model.P, model.M
    sim = edit.Similarity(rot_axis((0.3, -0.5, 0.8), 1.1), (0.4, -0.25, 0.6), 0.5, 0.5, 0.25)
    names = ("_xyz", "_t", "_scaling", "_scaling_t", "_rotation", "_rotation_r", "_features")
    src = [getattr(model, n).detach() for n in names]
    dst = [torch.empty_like(t) for t in src]
    # 16 geometry floats (opacity stays) and 3 M SH floats, read and written.  At this size the geometry pass's 38 MB stay in the
    # last-level cache between back-to-back calls: its figure is a launch rate, not an HBM bandwidth; the SH rows (346 MB) do not fit.
    geom_bytes, sh_bytes = 2 * 4 * 16 * P, 2 * 12 * M * P

    # the argument structs once: what is timed is the C call (two launches), not the float64 host set-up of the matrices
    args_geometry = [ctypes.byref(a) for a in edit._arguments(sim, 4, True, M, src[:6] + [None], dst[:6] + [None])]
    args_both = [ctypes.byref(a) for a in edit._arguments(sim, 4, True, M, src, dst)]

    def geometry():
        _capi.call("fdgs_model_transform", dev, *args_geometry)

    def both():
        _capi.call("fdgs_model_transform", dev, *args_both)

    def call():   # the whole Python call, host set-up and output allocation included
        edit.transform(model, sim)

    def copy_rows():   # the same bytes moved, nothing allocated
        dst[6].copy_(src[6])

    D = torch.from_numpy(edit.sh_rotation(sim.R).astype(np.float32)).to(dev)
    u, v = (torch.tensor(x, dtype=torch.float32, device=dev) for x in edit.isoclinic_pair(sim.R))

    def torch_rows():
        return torch.einsum("ij,pbjc->pbic", D, src[6].view(P, M // 16, 16, 3))

    def qmul(q, w):   # q * w for rows q [P,4] and one quaternion w: the 16 products and 12 sums of either isoclinic product
        a0, a1, a2, a3 = q.unbind(1)
        b0, b1, b2, b3 = w.unbind(0)
        return torch.stack([a0 * b0 - a1 * b1 - a2 * b2 - a3 * b3, a0 * b1 + a1 * b0 + a2 * b3 - a3 * b2,
                            a0 * b2 - a1 * b3 + a2 * b0 + a3 * b1, a0 * b3 + a1 * b2 - a2 * b1 + a3 * b0], dim=1)

    def torch_geometry():
        Rm = torch.from_numpy((sim.s * sim.R).astype(np.float32)).to(dev)
        xyz = src[0] @ Rm.T + torch.tensor(sim.T, dtype=torch.float32, device=dev)
        t = sim.a * src[1] + sim.b
        return xyz, t, src[2] + math.log(sim.s), src[3] + math.log(sim.a), qmul(src[4], v), qmul(src[5], u)

    tg, tb, tc, tr, tq, tt = timed(geometry), timed(both), timed(copy_rows), timed(torch_rows), timed(torch_geometry), timed(call)
    med = lambda x: x[len(x) // 2]   # noqa: E731
    rng = lambda x: [round(x[0] * 1e6, 2), round(x[-1] * 1e6, 2)]   # noqa: E731
    sh = med(tb) - med(tg)
    res = {"workload": "C3", "P": P, "M": M, "geometry_us": round(med(tg) * 1e6, 2), "geometry_us_range": rng(tg),
           "geometry_GBps": round(geom_bytes / med(tg) * 1e-9, 1),
           "both_kernels_us": round(med(tb) * 1e6, 2), "both_kernels_us_range": rng(tb),
           "sh_kernel_us": round(sh * 1e6, 2), "sh_bytes": sh_bytes, "sh_kernel_GBps": round(sh_bytes / sh * 1e-9, 1),
           "copy_rows_us": round(med(tc) * 1e6, 2), "copy_rows_us_range": rng(tc), "copy_rows_GBps": round(sh_bytes / med(tc) * 1e-9, 1),
           "torch_einsum_rows_us": round(med(tr) * 1e6, 2), "torch_einsum_rows_us_range": rng(tr),
           "torch_geometry_us": round(med(tq) * 1e6, 2), "torch_geometry_us_range": rng(tq),
           "transform_call_us": round(med(tt) * 1e6, 2), "transform_call_us_range": rng(tt)}
    print(json.dumps(res))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=20000, help="Gaussians per scene")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--height", type=int, default=208)
    ap.add_argument("--out", default="composed", help="prefix: <out>_0000.npy ... ([H, W, 3] uint8)")
    ap.add_argument("--bench", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.bench:
        bench(dev)
        return
    from fdgs import edit, playback, synth, train_host
    cfg = synth.SceneConfig("compose", args.P, args.width, args.height, 3, 1, 0.03, 1.0, True, 4, False)
    scene_a = synth.make_scene(cfg, seed=0, bg=(0.05, 0.05, 0.08), pose="rig1", alloc=(3, 2))
    scene_b = synth.make_scene(cfg, seed=1, pose="rig1", alloc=(3, 2))
    a, b = train_host.GaussianParams(scene_a, dev), train_host.GaussianParams(scene_b, dev)
    # the object: what of B lies in a box around its centre
    box = ((b._xyz.detach().abs() < torch.tensor([0.6, 0.6, 0.6], device=dev)).all(dim=1))
    obj = edit.extract(b, box)
    # half size, turned, set down to the right of A's centre; twice as fast and starting mid-way: T_b' = 0.5 T_b
    place = edit.Similarity(rot_axis((0.2, 1.0, 0.1), 0.9), (0.7, -0.2, 0.0), scale=0.5, time_scale=0.5, time_shift=0.5)
    try:
        edit.merge([a, edit.transform(obj, place)])
    except ValueError as e:   # a time degree is active and the durations now differ: the time basis cannot be shared
        print("merge refused, as it must:", e)
    # same duration as A (time_scale 1), shifted to start mid-way
    place = edit.Similarity(place.R, place.T, scale=0.5, time_scale=1.0, time_shift=0.5)
    placed = edit.transform(obj, place)
    merged = edit.merge([a, placed])
    print("A: %d Gaussians, B: %d, extracted %d, merged %d; duration %s" % (a.P, b.P, obj.P, merged.P, merged.time_duration))
    cam = train_host.SyntheticCamera(scene_a, dev)
    cams = playback.time_sweep(cam, 0.0, 1.5, args.frames)
    res = playback.render_path(merged, cams, train_host.PipelineFlags(), scene_a["bg"].to(dev))
    frames = res["frames"].cpu().numpy()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for k in range(frames.shape[0]):
        np.save("%s_%04d.npy" % (args.out, k), frames[k])
    print("%d frames of %s written to %s_*.npy" % (frames.shape[0], frames.shape[1:], args.out))


if __name__ == "__main__":
    main()
