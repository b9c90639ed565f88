#!/usr/bin/env python3
"""Pinned bits of the per-Gaussian geometry kernels (preprocess_fwd.hip, preprocess_bwd.hip): for small crafted models, what one
forward and one geometry backward (fdgs_rasterize_backward with stage_mask = 2: one thread per Gaussian, no atomics, reproducible
from run to run) write, as raw 32-bit patterns.  tests/test_gpu_api.py::test_geometry_kernels_pinned_bits makes the same calls
through ``run_case`` below and compares with ``==``.

The fixtures are NOT an oracle's results: they are what the library computed, on an MI355X, at the commit before the
covariance-at-time code moved into csrc/fdgs_math.h.  They pin the arithmetic of these kernels (every operation, its order, its
double promotions) under one toolchain; a change that is meant to alter a bit has to re-record them, and a compiler that schedules
the same source into other IEEE operations would too.  To re-record, on a machine with the GPU and a built library:

    python tests/golden/make_golden_geometry.py            ->  tests/golden/geometry/models.npz, <variant>_pf<on|off>_mod<1|07>.npz
    python tests/golden/make_golden_geometry.py --keep-models      (outputs only: the models, and so the inputs, stay as committed)

``FDGS_LIB`` selects another build of the library (fdgs/_capi.py), e.g. one of an earlier commit.

models.npz holds, per P in SIZES, every input tensor in both forms (raw parameters and activated ones; they are stored, not
derived at test time, so no host libm enters) and the [P,16] accumulator pattern.  Each model (P >= 63) has Gaussians on both sides
of the 0.05 temporal cull, Gaussian 1 behind the near plane and Gaussian 2 with an empty tile rectangle (far off to the side); a
model of one Gaussian is just that Gaussian.  The pattern has all-zero records, -0.0f and values in every word, 12..15 included.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                    # tests/ (util)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # the repository root (fdgs)

OUT_DIR = os.path.join(HERE, "geometry")
SIZES = (1, 63, 65, 229)
W, H = 48, 40                     # three tiles by three, neither a multiple of the tile
DURATION, TIMESTAMP = 4.0, 2.0
PREFILTER_ON = 0.3
# name -> (rot_4d, gaussian_dim, raw parameters, cov3D_precomp)
VARIANTS = {
    "rot4d_raw": (True, 4, True, False), "rot4d_act": (True, 4, False, False),
    "dim4_raw": (False, 4, True, False), "dim4_act": (False, 4, False, False),
    "dim3_raw": (False, 3, True, False), "precomp": (False, 3, False, True),
}
PREFILTER = {"pfoff": -1.0, "pfon": PREFILTER_ON}
MODIFIER = {"mod1": 1.0, "mod07": 0.7}
FORWARD_KEYS = ("radii", "out_means3D", "covs_com", "out_color")
BACKWARD_KEYS = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dflows", "dL_dts", "dL_dscales",
                 "dL_dscales_t", "dL_drotations", "dL_drotations_r")


def camera():
    from fdgs import synth
    return synth.camera_for("rig2", W, H)


def make_model(P, seed):
    """Every input of the model of P Gaussians as float32 numpy arrays."""
    rng = np.random.default_rng(seed)
    f = np.float32
    cam = camera()
    wv = cam["world_view_transform"].numpy().astype(np.float64)
    right, fwd = wv[:3, 0], wv[:3, 2]
    centre = cam["camera_center"].numpy().astype(np.float64)
    xyz = rng.uniform(-1.3, 1.3, (P, 3))
    ts = rng.uniform(-0.35, 1.35, (P, 1)) * DURATION
    if P > 2:
        xyz[1] = centre + 0.1 * fwd                    # view-space z = 0.1: behind the near plane (0.2)
        xyz[2] = centre + 4.0 * fwd + 40.0 * right     # in front, far off to the side: its rectangle is clamped to nothing
        ts[1] = ts[2] = TIMESTAMP                      # both pass the temporal cull
    scales = 0.06 * np.exp(0.3 * rng.standard_normal((P, 3)))
    scales_t = 0.5 * np.exp(0.3 * rng.standard_normal((P, 1)))
    ident = np.array([1.0, 0.0, 0.0, 0.0])
    unit = lambda q: q / np.linalg.norm(q, axis=1, keepdims=True)   # noqa: E731
    rot, rot_r = unit(ident + 0.5 * rng.standard_normal((P, 4))), unit(ident + 0.5 * rng.standard_normal((P, 4)))
    opa_raw = rng.standard_normal((P, 1))
    shs = 0.2 * rng.standard_normal((P, 4, 3))
    shs[:, 0, :] = rng.uniform(-1.0, 1.0, (P, 3))
    # cov3D_precomp: R diag(s^2) R^T of the same Gaussians (any symmetric positive matrix would do)
    r, x, y, z = rot.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z),
                  2 * (y * z - r * x), 2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(P, 3, 3)
    S = R @ (scales[:, :, None] ** 2 * np.transpose(R, (0, 2, 1)))
    cov = np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], axis=1)
    # the accumulator records: values in every word; every 5th record all zero; -0.0f in one word of every 7th and a record of them
    gacc = 0.1 * rng.standard_normal((P, 16))
    gacc[0::5] = 0.0
    for i in range(3, P, 7):
        gacc[i, i % 16] = -0.0
    if P > 11:
        gacc[11] = -0.0
    return {
        "means3D": f(xyz), "ts": f(ts), "shs": f(shs), "cov3D_precomp": f(cov), "grad_accum": f(gacc),
        "scales_act": f(scales), "scales_raw": f(np.log(scales)), "scales_t_act": f(scales_t), "scales_t_raw": f(np.log(scales_t)),
        "rotations_act": f(rot), "rotations_raw": f(rot * rng.uniform(0.5, 2.0, (P, 1))),
        "rotations_r_act": f(rot_r), "rotations_r_raw": f(rot_r * rng.uniform(0.5, 2.0, (P, 1))),
        "opacities_act": f(1.0 / (1.0 + np.exp(-opa_raw))), "opacities_raw": f(opa_raw),
    }


def scene_of(model, variant, pf, mod, device):
    """The scene dict (tests/util.py: native_args_fwd) of one case, tensors on ``device``."""
    rot_4d, dim, raw, precomp = VARIANTS[variant]
    form = "_raw" if raw else "_act"
    t = lambda k: torch.from_numpy(model[k]).to(device)   # noqa: E731
    sc = dict(camera())
    sc = {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in sc.items()}
    sc.update({
        "bg": torch.tensor([0.1, 0.2, 0.3], device=device), "W": W, "H": H, "means3D": t("means3D"), "shs": t("shs"),
        "opacities": t("opacities" + form), "sh_degree": 1, "sh_degree_t": 0, "timestamp": TIMESTAMP, "time_duration": DURATION,
        "rot_4d": rot_4d, "gaussian_dim": dim, "force_sh_3d": dim == 3, "scale_modifier": MODIFIER[mod], "prefilter_var": PREFILTER[pf],
    })
    if precomp:
        sc["cov3D_precomp"] = t("cov3D_precomp")
    else:
        sc["scales"], sc["rotations"] = t("scales" + form), t("rotations" + form)
    if dim == 4:
        sc["ts"], sc["scales_t"] = t("ts"), t("scales_t" + form)
    if rot_4d:
        sc["rotations_r"] = t("rotations_r" + form)
    return sc, raw


def run_case(model, variant, pf, mod, device):
    """One forward, then the geometry backward alone on the model's accumulator pattern; numpy arrays by name."""
    from fdgs.gaussian_renderer.diff_gaussian_rasterization import _C
    from util import native_args_fwd
    sc, raw = scene_of(model, variant, pf, mod, device)
    P = int(sc["means3D"].shape[0])
    e = torch.Tensor([])
    g = lambda k: sc[k] if sc.get(k) is not None else e  # noqa: E731
    res = _C.rasterize_gaussians(*native_args_fwd(sc), raw_params=raw)
    (R, color, _flow, _depth, _T, radii, geom, binb, img, covs_com, out_means3D) = res
    out = {"radii": radii, "out_means3D": out_means3D, "covs_com": covs_com, "out_color": color}
    gacc = torch.zeros((P, 16), device=device)
    stage = torch.zeros((P, 8), device=device)
    zero = torch.zeros((3, H, W), device=device)
    # the blend backward of an all-zero image gradient (stage_mask 5) only sets the call up ...
    pend = _C.backward_begin(
        sc["bg"], sc["means3D"], out_means3D, radii, e, e, sc["opacities"], g("ts"), g("scales"), g("scales_t"), g("rotations"),
        g("rotations_r"), sc["scale_modifier"], g("cov3D_precomp"), sc["prefilter_var"], sc["world_view_transform"],
        sc["full_proj_transform"], sc["tanfovx"], sc["tanfovy"], zero, None, None, None, sc["shs"], sc["sh_degree"], sc["sh_degree_t"],
        sc["camera_center"], sc["timestamp"], sc["time_duration"], sc["rot_4d"], sc["gaussian_dim"], sc["force_sh_3d"], geom, R, binb,
        img, False, raw_params=raw, grad_accum=gacc, sh_stage=stage)
    torch.cuda.synchronize()
    # ... then the records are the pattern, and the geometry backward (stage_mask 2) runs alone
    gacc.copy_(torch.from_numpy(model["grad_accum"]).to(device))
    grads = _C.backward_finish(pend)
    torch.cuda.synchronize()
    names = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dflows", "dL_dts", "dL_dscales",
             "dL_dscales_t", "dL_drotations", "dL_drotations_r")
    out.update({n: t for n, t in zip(names, grads) if n in BACKWARD_KEYS})
    assert float(gacc.abs().max()) == 0.0   # the backward leaves the records zero again
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


def load_models():
    z = np.load(os.path.join(OUT_DIR, "models.npz"))
    return {P: {k[len("P%d_" % P):]: z[k] for k in z.files if k.startswith("P%d_" % P)} for P in SIZES}


def check_contents(model, variant, pf, mod, got):
    """What a model must contain (P >= 63), from float64 host arithmetic with a margin and from the recorded radii."""
    rot_4d, dim, raw, precomp = VARIANTS[variant]
    radii = got["radii"]
    assert radii[1] == 0 and radii[2] == 0 and (radii > 0).any(), (variant, radii[:3])
    if dim == 4 and not precomp and not rot_4d:
        var = model["scales_t_act"].astype(np.float64)[:, 0] * MODIFIER[mod]
        if PREFILTER[pf] > 0:
            var = var + PREFILTER[pf]
        dt = model["ts"].astype(np.float64)[:, 0] - TIMESTAMP
        m = np.exp(-0.5 * dt * dt / var)
        assert (m > 0.06).sum() >= 4 and (m < 0.04).sum() >= 4, (variant, pf, mod)
    if rot_4d:
        # culled by the marginal: out_means3D is the input mean, bit for bit (no shift applied); kept ones are shifted
        same = (got["out_means3D"].view(np.uint32) == model["means3D"].view(np.uint32)).all(1)
        assert same.sum() >= 4 and (~same).sum() >= 4, (variant, pf, mod, int(same.sum()))


def main():
    keep_models = "--keep-models" in sys.argv[1:]
    os.makedirs(OUT_DIR, exist_ok=True)
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: the fixtures are the library's own results")
    dev = torch.device("cuda:0")
    if not keep_models:
        flat = {}
        for P in SIZES:
            flat.update({"P%d_%s" % (P, k): v for k, v in make_model(P, 900 + P).items()})
        np.savez_compressed(os.path.join(OUT_DIR, "models.npz"), **flat)
    models = load_models()
    for variant in VARIANTS:
        for pf in PREFILTER:
            for mod in MODIFIER:
                d = {}
                for P in SIZES:
                    got = run_case(models[P], variant, pf, mod, dev)
                    again = run_case(models[P], variant, pf, mod, dev)
                    for k in got:
                        assert got[k].tobytes() == again[k].tobytes(), ("not reproducible", variant, pf, mod, P, k)
                    if P >= 63:
                        check_contents(models[P], variant, pf, mod, got)
                    d.update({"P%d_%s" % (P, k): v for k, v in got.items()})
                name = "%s_%s_%s.npz" % (variant, pf, mod)
                np.savez_compressed(os.path.join(OUT_DIR, name), **d)
                print(name, os.path.getsize(os.path.join(OUT_DIR, name)), "bytes")


if __name__ == "__main__":
    sys.exit(main())
