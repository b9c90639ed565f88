"""Times the environment-map composite (csrc/envmap.hip) at C3 (300 k Gaussians, 1352 x 1014) with a 3 x 500 x 500 map, the
rasterizer backward with and without an alpha gradient (a non-NULL dL_dout_alpha selects the heavier blend-backward variant, which
the map makes the default) and the four-view StepPipeline step with and without the map.  Two camera sets: the bench's rig, which
looks at the +z pole (the central tiles take the wide-window path of the map's gradient), and the same rig turned to look along the
equator (the Gaussians' means turned with it; their covariances not: a timing scene).  Prints one JSON line of medians in ms.

    python tools/envmap_cost.py [--reps 50]
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from regularizer_cost import _median_ms  # noqa: E402


class _Pipe:
    compute_cov3D_python = False
    convert_SHs_python = False
    debug = False

    def __init__(self, res):
        self.env_map_res = res


def _rig(scene, dev, equator):
    from fdgs import synth, train_host
    cams = [train_host.SyntheticCamera(scene, dev, timestamp=(b + 0.5) / 4 * scene["time_duration"]) for b in range(4)]
    if equator:   # the world turned by Rx(-90 deg): (x, y, z) -> (x, z, -y); the camera at (0, -4, 0) looking along +y
        c = synth.make_camera(scene["W"], scene["H"], pitch=-math.pi / 2, shift=(0.0, -4.0, 4.0))
        for cam in cams:
            cam.world_view_transform = c["world_view_transform"].to(dev)
            cam.full_proj_transform = c["full_proj_transform"].to(dev)
            cam.camera_center = c["camera_center"].to(dev)
    return cams


def _model(scene, dev, equator, R):
    from fdgs import train_host
    m = train_host.GaussianParams(scene, dev)
    if equator:
        with torch.no_grad():
            xyz = m.params["_xyz"]
            y, z = xyz[:, 1].clone(), xyz[:, 2].clone()
            xyz[:, 1], xyz[:, 2] = z, -y
    g = torch.Generator(device="cpu").manual_seed(3)
    m.env_map = (0.5 + 0.1 * torch.rand(3, R, R, generator=g)).to(dev)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--res", type=int, default=500)
    args = ap.parse_args()
    from fdgs import envmap, synth, train_host
    from fdgs.fused import raw_backward, raw_forward, raw_settings
    from fdgs.pipeline import StepPipeline

    dev = torch.device("cuda:0")
    scene = synth.make_scene(synth.CONFIGS[args.config], seed=0)
    H, W = scene["H"], scene["W"]
    out = {"config": args.config, "env": [3, args.res, args.res]}
    gen = torch.Generator(device="cpu").manual_seed(7)
    gts = [torch.rand(3, H, W, generator=gen).to(dev) for _ in range(4)]
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    for rig in ("pole", "equator"):
        eq = rig == "equator"
        cams = _rig(scene, dev, eq)
        m = _model(scene, dev, eq, args.res)
        env = m.env_map
        rs, tens = raw_settings(cams[0], m, _Pipe(args.res), bg)
        (R, color, flow, depth, T, radii, geom, binb, img, _c, om) = raw_forward(rs, *tens)
        g_col = torch.randn(3, H, W, device=dev) * 1e-3
        g_alpha = torch.empty(1, H, W, device=dev)
        g_env = torch.empty_like(env)
        dst = torch.empty_like(color)
        tb = T.reshape(H, W)
        out[rig + "_T_mean"] = round(float(tb.mean()), 4)
        out[rig + "_composite_fwd_ms"] = _median_ms(lambda: envmap.composite_(color, tb, env, cams[0], out=dst), args.reps)
        out[rig + "_composite_bwd_ms"] = _median_ms(lambda: envmap.composite_backward(tb, g_col, env, cams[0], g_alpha, False, g_env, False),
                                                    args.reps)
        out[rig + "_composite_bwd_no_env_ms"] = _median_ms(lambda: envmap.composite_backward(tb, g_col, env, cams[0], g_alpha, False),
                                                           args.reps)
        sink = m.grad_sink()
        gacc = torch.zeros(m.P, 16, device=dev)
        for name, ga in (("raster_bwd_alpha_null_ms", None), ("raster_bwd_alpha_ms", g_alpha)):
            out[rig + "_" + name] = _median_ms(lambda: raw_backward(rs, tens[0], om, radii, *tens[1:], geom, R, binb, img, g_col, None, ga,
                                                                    None, sink, False, grad_accum=gacc, per_view_outputs=False), args.reps)
        del geom, binb, img
        for name, res in (("step_plain_ms", 0), ("step_env_ms", args.res)):
            sp = StepPipeline(m, train_host.make_optimizer(m), world_size=1, lambda_dssim=0.2)
            out[rig + "_" + name] = _median_ms(lambda: sp.step(cams, gts, _Pipe(res), bg), args.reps)
            del sp
        out[rig + "_step_delta_pct"] = round(100.0 * (out[rig + "_step_env_ms"] / out[rig + "_step_plain_ms"] - 1.0), 2)
        del m
    print(json.dumps({kk: (round(v, 4) if isinstance(v, float) else v) for kk, v in out.items()}))


if __name__ == "__main__":
    main()
