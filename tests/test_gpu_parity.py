"""GPU parity tests: the HIP product (through the C ABI) against the CPU oracle on identical seeded inputs.

Bar (BASELINE.md / north_star): tile / key indexing bit-exact (radii, tiles_touched, depth-key bits,
point_list, ranges, n_contrib), pixels within 1e-4 abs, gradients within 1e-4 (of max(1, max|ref|)).
Pixels flagged by the oracle as sitting on a threshold cliff (alpha ~ 1/255, T ~ 1e-4 within 1e-5 relative)
are excluded from the pixel / n_contrib comparison and their fraction is bounded.
"""
import numpy as np
import pytest
import torch

import os

from util import (CHAIN_ACTIVATED, GRAD_SCALE, NOISE_K, check_backward, check_backward_noise_aware, check_forward, fmt_noise_rep, oracle_four_modes,
                  pyoracle, run_hip, run_oracle, synth)

# How many times the HIP backward is drawn against the (deterministic) oracle results in the full-size tests: the HIP kernels' float
# atomics land in another order every run, the bars must hold for every draw.  FDGS_PARITY_REPEATS=20 is how BASELINE.md section 5's
# "consecutive draws green" count was produced.
REPEATS = max(1, int(os.environ.get("FDGS_PARITY_REPEATS", "1")))

pytestmark = pytest.mark.gpu

SC = synth.SceneConfig


def _variants():
    v = {}
    v["C1_rot4d_sh0"] = dict(cfg=synth.CONFIGS["C1"], kw=dict(random_flow=True, bg=(0.3, 0.5, 0.7)))
    v["rot4d_sh3_t2"] = dict(cfg=SC("v", 30000, 400, 304, 3, 2, 0.015, 10.0, True, 4, False), kw=dict(random_flow=True))
    v["rot4d_sh3_t1"] = dict(cfg=SC("v", 8000, 200, 120, 3, 1, 0.03, 2.0, True, 4, False), kw=dict(bg=(1.0, 1.0, 1.0)))
    v["rot4d_sh2_4d"] = dict(cfg=SC("v", 8000, 200, 120, 2, 2, 0.03, 2.0, True, 4, False), kw=dict())
    v["dim3_sh2"] = dict(cfg=SC("v", 8000, 256, 256, 2, 0, 0.03, 1.0, False, 3, False), kw=dict(random_flow=True))
    v["dim4_norot_sh1"] = dict(cfg=SC("v", 8000, 250, 130, 1, 0, 0.03, 1.0, False, 4, True), kw=dict(bg=(0.1, 0.2, 0.3)))
    v["ragged_33x17"] = dict(cfg=SC("v", 500, 33, 17, 3, 0, 0.05, 1.0, True, 4, True), kw=dict())
    return v


VARIANTS = _variants()


def _scene(name):
    spec = VARIANTS[name]
    return synth.make_scene(spec["cfg"], seed=3, **spec["kw"])


@pytest.mark.parametrize("name", list(VARIANTS))
def test_forward_backward_vs_oracle(name, gpu_device):
    scene = _scene(name)
    grads = synth.make_upstream_grads(scene["W"], scene["H"], seed=1, scale=GRAD_SCALE)
    hip, hipg = run_hip(scene, gpu_device, grads)
    ref, refg = run_oracle(scene, grads, kind="port")
    rep = check_forward(hip, ref, name)
    repg = check_backward(hipg, refg, name)
    print(name, "R", ref["R"], {k: ("%.2e" % v if isinstance(v, float) else v) for k, v in rep.items()})
    print(name, {k: "%.2e/%.1e" % v for k, v in repg.items()})


# scale_modifier != 1 (forward.cu:418-434 scales every axis incl. the temporal one, backward.cu:911-916) and prefilter_var > 0
# (the temporal marginal's variance floor: forward.cu:333 / 434, backward.cu:746) -- the two settings no other scene sets
# (gaussian_renderer/__init__.py:43 scaling_modifier, arguments/__init__.py:62 prefilter_var); with the reference's lists and
# with tile_cull (the reachable rectangle depends on the opacity the marginal scales).
@pytest.mark.parametrize("tile_cull", [False, True])
@pytest.mark.parametrize("mod,pv", [(0.5, 0.01), (2.0, 0.3), (0.5, 0.3), (2.0, 0.01)])
@pytest.mark.parametrize("name", ["rot4d_sh3_t1", "dim4_norot_sh1", "rot4d_sh2_4d"])
def test_scale_modifier_and_prefilter_var_vs_oracle(name, mod, pv, tile_cull, gpu_device):
    scene = _scene(name)
    scene["scale_modifier"], scene["prefilter_var"] = mod, pv
    grads = synth.make_upstream_grads(scene["W"], scene["H"], seed=1, scale=GRAD_SCALE)
    hip, hipg = run_hip(scene, gpu_device, grads, tile_cull=tile_cull)
    ref, refg = run_oracle(scene, grads, kind="port")
    base, _ = run_oracle(_scene(name), None, kind="port")
    assert ref["R"] != base["R"], "the flags changed nothing: the case does not test them"
    rep = check_forward(hip, ref, "%s mod %g pv %g" % (name, mod, pv), tile_cull=tile_cull, WH=(scene["W"], scene["H"]), max_border=2e-3)
    repg = check_backward(hipg, refg, "%s mod %g pv %g" % (name, mod, pv))
    print(name, mod, pv, "R", ref["R"], "(default flags: %d)" % base["R"], {k: "%.2e/%.1e" % v for k, v in repg.items()})


def test_scale_modifier_3d_vs_oracle(gpu_device):
    """gaussian_dim == 3 has no temporal marginal: scale_modifier alone (computeCov3D, forward.cu:242-276)."""
    scene = _scene("dim3_sh2")
    scene["scale_modifier"] = 1.7
    grads = synth.make_upstream_grads(scene["W"], scene["H"], seed=1, scale=GRAD_SCALE)
    hip, hipg = run_hip(scene, gpu_device, grads)
    ref, refg = run_oracle(scene, grads, kind="port")
    check_forward(hip, ref, "dim3 mod 1.7", max_border=2e-3)
    check_backward(hipg, refg, "dim3 mod 1.7")


def test_precomputed_cov_and_colors(gpu_device):
    """cov3D_precomp + colors_precomp branch (forward.cu:411-414, 476): feed the oracle's own cov3D / rgb back in."""
    base = synth.make_scene(SC("v", 6000, 200, 160, 1, 0, 0.03, 1.0, True, 4, True), seed=5)
    ref0, _ = run_oracle(base, None, kind="port")
    scene = dict(base)
    scene["means3D"] = torch.from_numpy(ref0["out_means3D"].copy())
    scene["cov3D_precomp"] = torch.from_numpy(ref0["cov3D"].copy())
    scene["colors_precomp"] = torch.from_numpy(np.random.default_rng(0).random((6000, 3)).astype(np.float32))
    for k in ("shs", "scales", "rotations", "scales_t", "rotations_r", "ts"):
        scene[k] = None
    scene["rot_4d"], scene["gaussian_dim"] = False, 3
    grads = synth.make_upstream_grads(scene["W"], scene["H"], seed=2, scale=GRAD_SCALE)
    hip, hipg = run_hip(scene, gpu_device, grads)
    ref, refg = run_oracle(scene, grads, kind="port")
    check_forward(hip, ref, "precomp", precomp_cov=True, precomp_colors=True)
    check_backward(hipg, refg, "precomp")


def test_all_culled_and_empty(gpu_device):
    """Edge cases: every Gaussian behind the camera (R == 0) and P == 0: background image, T == 1."""
    scene = synth.make_scene(SC("v", 300, 64, 48, 0, 0, 0.03, 1.0, True, 4, True), seed=1, bg=(0.2, 0.4, 0.6))
    scene["means3D"] = scene["means3D"].clone()
    scene["means3D"][:, 2] = -10.0
    hip, _ = run_hip(scene, gpu_device, None)
    assert hip["R"] == 0 and (hip["radii"] == 0).all()
    assert np.allclose(hip["out_T"], 1.0) and (hip["n_contrib"] == 0).all()
    for c, v in enumerate((0.2, 0.4, 0.6)):
        assert np.allclose(hip["out_color"][c], v)
    empty = dict(scene)
    for k in ("means3D", "ts", "scales", "scales_t", "rotations", "rotations_r", "opacities", "shs", "flow_2d"):
        empty[k] = scene[k][:0].clone()
    hip, _ = run_hip(empty, gpu_device, None)
    assert hip["R"] == 0 and np.allclose(hip["out_T"], 1.0)


@pytest.mark.parametrize("pose", ["axis", "rig1"])
def test_c2_full_size(pose, gpu_device):
    """BASELINE configs[1]: 100k Gaussians, 800x800, SH degree 3, forward + backward against the oracle -- on the unrotated on-axis
    camera and on a rotated, off-axis one (upstream gradients zeroed on the oracle-flagged cliff pixels on both sides there)."""
    scene = synth.make_scene(synth.CONFIGS["C2"], seed=0, pose=pose)
    grads = synth.make_upstream_grads(scene["W"], scene["H"], seed=1, scale=GRAD_SCALE)
    if pose != "axis":
        ref0, _ = run_oracle(scene, None, kind="port")
        keep = torch.from_numpy(~ref0["border"].astype(bool)).to(torch.float32)
        grads = {k: v * keep.reshape((1,) * (v.dim() - 2) + (scene["H"], scene["W"])) for k, v in grads.items()}
    hip, hipg = run_hip(scene, gpu_device, grads)
    ref, refg = run_oracle(scene, grads, kind="port")
    rep = check_forward(hip, ref, "C2 " + pose, max_border=5e-4)
    repg = check_backward(hipg, refg, "C2 " + pose)
    print("C2", pose, "R", ref["R"], rep)
    print("C2", pose, {k: "%.2e/%.1e" % v for k, v in repg.items()})


@pytest.mark.parametrize("name", ["rot4d_sh3_t2", "C1_rot4d_sh0", "ragged_33x17"])
def test_colour_only_backward_vs_oracle(name, gpu_device):
    """Only the colour image has an upstream gradient (depth / alpha / flow gradients None at the binding, NULL at
    the C ABI): the colour-only blend-backward variant must equal the oracle fed with explicit zeros."""
    scene = _scene(name)
    grads = synth.make_upstream_grads(scene["W"], scene["H"], seed=3, scale=GRAD_SCALE)
    zeros = {k: (v if k == "grad_color" else torch.zeros_like(v)) for k, v in grads.items()}
    nones = {k: (v if k == "grad_color" else None) for k, v in grads.items()}
    _, hipg = run_hip(scene, gpu_device, nones)
    _, refg = run_oracle(scene, zeros, kind="port")
    check_backward(hipg, refg, name + " colour-only")


def test_depth_only_backward_vs_oracle(gpu_device):
    """No upstream gradient for the colour image (NULL at the C ABI), only for depth and alpha: the general backward
    variant with zeros substituted in the kernel equals the oracle fed with an explicit zero colour gradient."""
    name = "rot4d_sh3_t1"
    scene = _scene(name)
    grads = synth.make_upstream_grads(scene["W"], scene["H"], seed=4, scale=GRAD_SCALE)
    zeros = {k: (torch.zeros_like(v) if k in ("grad_color", "grad_flow") else v) for k, v in grads.items()}
    nones = {k: (None if k in ("grad_color", "grad_flow") else v) for k, v in grads.items()}
    _, hipg = run_hip(scene, gpu_device, nones)
    _, refg = run_oracle(scene, zeros, kind="port")
    check_backward(hipg, refg, name + " depth+alpha only")


# ----------------------------------------------------------------------------------------------------------------
# The configuration the metric is quoted on, through the path bench.py times
# ----------------------------------------------------------------------------------------------------------------

def _timed_path_vs_oracle(cfg, dev, n_views, label, max_border, tile_cull=True, scale_modifier=1.0, prefilter_var=-1.0, poses=None, alloc=None,
                          make_kw=None, raw_quat_scale=None, chain=("_scaling", "_scaling_t", "_rotation", "_rotation_r"), repeats=1, scene_hook=None, dump=None,
                          ready=None):
    """The calls fdgs/pipeline.py::StepPipeline makes for one optimizer step -- raw parameters (activations fused into
    the kernels, fdgs_scene.raw_params = 1), fused L1 + SSIM gradient as the only upstream gradient (colour-only blend
    backward), parameter gradients accumulated over the views into the flat bucket, persistent always-zero blend
    accumulator -- compared with the port oracle view by view.  The oracle is fed the ACTIVATED tensors the kernels
    derive themselves (fdgs_debug_activations: same device functions, bit-identical), and its gradients are pulled
    back to the raw parameters in float64, so the 1e-4 bar applies to this mode unchanged.
    Bar: radii / tiles_touched / depth bits / point_list / sorted tile ids / ranges bit-exact, n_contrib equal and
    pixels <= 1e-4 abs off the flagged cliff pixels, every gradient <= 1e-4 * max(1, max|ref|) -- except that an element of the
    tensors in ``chain`` (default: the four covariance-chain tensors) beyond that bar is held to the conditioning-aware bar of
    util.check_backward_noise_aware: 1e-4 * scale + NOISE_K x what the reference's own accumulation orders do to THAT Gaussian.
    ``repeats``: the HIP backward is drawn that many times against the same oracle results (FDGS_PARITY_REPEATS).  ``tile_cull`` (what StepPipeline runs with): the lists are the reference's with the instances taken out that
    cannot reach alpha >= 1/255 in their tile -- checked as such (util.check_culled_lists) instead of bit for bit.
    ``ready`` = (model, scene, cameras): a ready GaussianParams (e.g. GaussianParams.from_raw of a recorded trained state) instead of one
    built from fdgs.synth -- ``cfg`` is then None; ``scene``: the scene dict the oracle is fed from (its per-Gaussian ACTIVATED tensors are
    replaced by the kernels' own, its means3D / ts / shs must be the model's), ``cameras``: ``n_views`` pairs (camera tensors as
    synth.camera_for returns them, timestamp)."""
    from fdgs import _capi, train_host
    from fdgs.fused import raw_backward, raw_forward, raw_settings
    from fdgs.loss import l1_ssim_grad
    from util import collect_forward

    if ready is None:
        scene = synth.make_scene(cfg, seed=0, **(make_kw or {}))
        if scene_hook is not None:
            scene_hook(scene)
        model = train_host.GaussianParams(scene, dev)
    else:
        model, scene, ready_cams = ready
        assert len(ready_cams) == n_views and model.P == int(scene["means3D"].shape[0])
    P, W, H = int(scene["means3D"].shape[0]), scene["W"], scene["H"]
    if raw_quat_scale is not None:
        # the RAW quaternions of a trained model are not unit (scene/gaussian_model.py:191-197 normalises in the getter, nothing keeps
        # the parameter itself on the sphere): lengths from raw_quat_scale[0] to [1], so that the normalisation's chain rule
        # (g - q (q . g)) / |q| is exercised with |q| != 1
        gq = torch.Generator(device="cpu").manual_seed(5)
        lo, hi = raw_quat_scale
        with torch.no_grad():
            for name in ("_rotation", "_rotation_r"):
                model.params[name].mul_((lo + (hi - lo) * torch.rand(P, 1, generator=gq)).to(dev))
    model.prefilter_var = prefilter_var
    pipe = train_host.PipelineFlags()
    bg = scene["bg"].to(dev)
    dur = scene["time_duration"]
    if ready is None:
        cam_tensors = [synth.camera_for(poses[b] if poses else "axis", W, H) for b in range(n_views)]
        stamps = [(b + 0.5) / n_views * dur for b in range(n_views)]
    else:
        cam_tensors, stamps = [c for c, _ in ready_cams], [t for _, t in ready_cams]
    cams = [train_host.SyntheticCamera(dict(scene, **cam_tensors[b]), dev, timestamp=stamps[b]) for b in range(n_views)]
    gen = torch.Generator(device="cpu").manual_seed(99)
    gts = [torch.rand(3, H, W, generator=gen).to(dev) for _ in range(n_views)]
    # The loss is a mean over 3 N pixels: its image gradient is O(1 / (3 N)).  The kernels are linear in the upstream
    # gradient, so it is scaled up to the magnitude the other parity tests use (GRAD_SCALE); otherwise an absolute
    # 1e-4 bound would be vacuous.
    up = torch.full((1,), 3.0 * W * H * GRAD_SCALE / n_views, dtype=torch.float32, device=dev)
    sink = model.grad_sink()
    model.flat_grad.fill_(float("nan"))        # the first view must overwrite every element
    gacc = torch.zeros((P, 16), dtype=torch.float32, device=dev)
    act = _capi.debug_activations(model._opacity.detach(), model._scaling.detach(), model._scaling_t.detach(),
                                  model._rotation.detach(), model._rotation_r.detach())
    torch.cuda.synchronize()
    a_op, a_sc, a_sct, a_rot, a_rotr = [t.cpu() for t in act]
    raw = {n: model.params[n].detach().cpu().numpy().astype(np.float64) for n in model.NAMES}

    def to_raw(refg):
        """float64 chain rule of the reference's activations (scene/gaussian_model.py:55-66)."""
        o = a_op.numpy().astype(np.float64).reshape(-1)
        out = {"_xyz": refg["dL_dmean3D"].astype(np.float64), "_features": refg["dL_dsh"].astype(np.float64),
               "_t": refg["dL_dts"].astype(np.float64).reshape(-1, 1),
               "_opacity": (refg["dL_dopacity"].astype(np.float64) * o * (1.0 - o)).reshape(-1, 1),
               "_scaling": refg["dL_dscale"].astype(np.float64) * a_sc.numpy().astype(np.float64),
               "_scaling_t": (refg["dL_dscale_t"].astype(np.float64) * a_sct.numpy().astype(np.float64).reshape(-1)).reshape(-1, 1)}
        for name, gname, q32 in (("_rotation", "dL_drot", a_rot), ("_rotation_r", "dL_drot_r", a_rotr)):
            q = q32.numpy().astype(np.float64)
            g = refg[gname].astype(np.float64)
            inv = 1.0 / np.maximum(np.linalg.norm(raw[name], axis=1, keepdims=True), 1e-12)
            out[name] = (g - q * (q * g).sum(1, keepdims=True)) * inv
        return out

    names = ("dL_dmean2D", "dL_dcolor", "dL_dopacity", "dL_dmean3D", "dL_dcov3D", "dL_dsh", "dL_dflows", "dL_dts",
             "dL_dscale", "dL_dscale_t", "dL_drot", "dL_drot_r")
    zeros13 = (torch.zeros(1, H, W), torch.zeros(1, H, W), torch.zeros(2, H, W))
    total = total_rev = total_f64 = total_probe = None
    views = []
    for b, cam in enumerate(cams):
        rs, (xyz, feats, opacity, ts, scaling, scaling_t, rotation, rotation_r, pv) = raw_settings(cam, model, pipe, bg, scale_modifier)
        res = raw_forward(rs, xyz, feats, opacity, ts, scaling, scaling_t, rotation, rotation_r, pv, tile_cull=tile_cull)
        (R, color, flow, depth, T, radii, geom, binb, img, _covs, out_means3D) = res
        hip = collect_forward(res, P, W, H)
        g_color, _handle = l1_ssim_grad(color, gts[b], 0.2, up)
        osc = dict(scene, **cam_tensors[b])
        osc.update(opacities=a_op, scales=a_sc, scales_t=a_sct, rotations=a_rot, rotations_r=a_rotr, timestamp=cam.timestamp,
                   scale_modifier=scale_modifier, prefilter_var=prefilter_var)
        o = pyoracle.Oracle(osc, kind="port")
        ref = dict(o.forward())
        ref["R"] = o.R
        # Pixels the oracle flags as sitting on a threshold cliff (alpha ~ 1/255 or T ~ 1e-4 within 1e-5 relative) may
        # legitimately land on either side in the two implementations; they are excluded from the pixel comparison,
        # and -- the same exclusion for the backward -- their upstream gradient is zeroed on BOTH sides, so that the
        # gradient comparison measures arithmetic, not which side of a threshold a pixel fell on.
        cliff = torch.from_numpy(ref["border"].astype(bool)).to(dev)
        g_unmasked = g_color
        g_color = g_color * (~cliff).to(g_color.dtype)
        # The UNMASKED error, tracked and bounded for EVERY view and ALL twelve gradient tensors: the same backward with the cliff
        # pixels' upstream gradient left in (no sink: nothing is accumulated, the activated-parameter gradients come back as the
        # binding's tuple -- raw-parameter chain rule applied to the oracle's side).  What it adds to the masked comparison is the
        # effect of alpha >= 1/255 / T >= 1e-4 decisions that fell the other way on the ~5e-4 of the pixels that sit on a cliff:
        # bounded by 10 x the bar (100 x for the four covariance-chain tensors).
        gu = raw_backward(rs, xyz, out_means3D, radii, feats, opacity, ts, scaling, scaling_t, rotation, rotation_r, pv,
                          geom, R, binb, img, g_unmasked, None, None, None, None, False, grad_accum=gacc)
        torch.cuda.synchronize()
        refu = dict(o.backward(g_unmasked.cpu(), *zeros13))
        ru = to_raw(refu)
        want_u = {"dL_dmean2D": refu["dL_dmean2D"], "dL_dcolor": refu["dL_dcolor"], "dL_dcov3D": refu["dL_dcov3D"], "dL_dflows": refu["dL_dflows"],
                  "dL_dopacity": ru["_opacity"], "dL_dmean3D": ru["_xyz"], "dL_dsh": ru["_features"], "dL_dts": ru["_t"], "dL_dscale": ru["_scaling"],
                  "dL_dscale_t": ru["_scaling_t"], "dL_drot": ru["_rotation"], "dL_drot_r": ru["_rotation_r"]}
        unm = {}
        for n, t in zip(names, gu):
            want = want_u[n]
            sc = max(1.0, float(np.abs(want).max()))
            e = float(np.abs(t.cpu().numpy().reshape(want.shape) - want).max())
            unm[n] = "%.1e/%.1e" % (e, sc)
            # (the four covariance-chain tensors amplify a flipped pixel as they amplify rounding -- see below: 1e-2 of scale)
            ubound = (1e-2 if n in ("dL_dscale", "dL_dscale_t", "dL_drot", "dL_drot_r") else 1e-3) * sc
            assert e <= ubound, "%s view %d UNMASKED %s: %g > %g" % (label, b, n, e, ubound)
        print("%s view %d UNMASKED gradients, all 12 tensors (cliff pixels' upstream gradient kept; max abs err / max|ref|; bound 1e-3 of scale, "
              "covariance chain 1e-2):" % (label, b), unm)
        del gu
        grads = raw_backward(rs, xyz, out_means3D, radii, feats, opacity, ts, scaling, scaling_t, rotation, rotation_r, pv,
                             geom, R, binb, img, g_color, None, None, None, sink, b > 0, grad_accum=gacc)
        torch.cuda.synchronize()
        assert float(gacc.abs().max()) == 0.0, "the persistent blend accumulator was not left all zero"
        views.append((rs, xyz, out_means3D, radii, feats, opacity, ts, scaling, scaling_t, rotation, rotation_r, pv, geom, R, binb, img, g_color))
        gc = g_color.cpu()
        refg = dict(o.backward(gc, *zeros13))
        # The reference against ITSELF: the same backward with (1) the blend backward's fp32 atomics issued in another legal order
        # (tiles and threads descending, oracle_set_accumulation(1)) and (2) the per-Gaussian sums accumulated in double (mode 2).
        # (0 vs 1) is the accumulation-order noise the reference carries on any GPU -- CUDA fixes no order for atomicAdd.
        pyoracle.set_accumulation(1)
        refg_rev = dict(o.backward(gc, *zeros13))
        pyoracle.set_accumulation(2)
        refg_f64 = dict(o.backward(gc, *zeros13))
        pyoracle.set_accumulation(3)   # the conditioning probe (oracle/fdgs_oracle.c): every term perturbed by a few ulp of what it is computed from
        refg_probe = dict(o.backward(gc, *zeros13))
        pyoracle.set_accumulation(0)
        o.close()
        rep = check_forward(hip, ref, "%s view %d" % (label, b), max_border=max_border, tile_cull=tile_cull, WH=(W, H))
        if tile_cull:
            print("%s view %d: instances listed: %s" % (label, b, rep["instances"]))
        print("%s view %d: R %d, cliff pixel fraction %.2e (upstream gradient zeroed there), max abs pixel err colour %.2e depth %.2e T %.2e" % (
            label, b, ref["R"], rep["border_frac"], rep["out_color"], rep["out_depth"], rep["out_T"]))
        # per-view outputs of the backward (always overwritten): viewspace gradient, colour, covariance
        per_view = {n: t.cpu().numpy() for n, t in zip(names, grads) if n in ("dL_dmean2D", "dL_dcolor", "dL_dcov3D", "dL_dflows")}
        repg = check_backward(per_view, {k: refg[k] for k in per_view}, "%s view %d" % (label, b))
        print("%s view %d per-view gradients (max abs err / max|ref|):" % (label, b), {k: "%.2e/%.1e" % v for k, v in repg.items()})
        r, rr, r64, rpr = to_raw(refg), to_raw(refg_rev), to_raw(refg_f64), to_raw(refg_probe)
        total_probe = rpr if total_probe is None else {k: total_probe[k] + rpr[k] for k in rpr}
        total = r if total is None else {k: total[k] + r[k] for k in r}
        total_rev = rr if total_rev is None else {k: total_rev[k] + rr[k] for k in rr}
        total_f64 = r64 if total_f64 is None else {k: total_f64[k] + r64[k] for k in r64}

    if ready is None:
        n_active = synth.active_sh_coeffs(cfg.sh_degree, cfg.sh_degree_t, cfg.force_sh_3d, cfg.gaussian_dim)
    else:
        n_active = synth.active_sh_coeffs(model.active_sh_degree, model.active_sh_degree_t, model.force_sh_3d, model.gaussian_dim)
    assert float(np.abs(total["_features"].reshape(P, -1, 3)[:, n_active:]).max(initial=0.0)) == 0.0   # the reference's zeros
    # Gradients of the covariance parameters are cancelling sums of products of dL/dcov3D (O(1e3) here) with the
    # scale / rotation matrices: the chain amplifies a 1e-6 relative rounding difference in the blend backward's per-Gaussian
    # sums -- thousands of fp32 atomics per Gaussian, in whatever order the hardware issues them -- by two to three orders of
    # magnitude, in ANY implementation incl. the reference itself.  So for the tensors in ``chain`` an element beyond the plain bar is
    # held to the conditioning-aware bar (tests/util.py::check_backward_noise_aware): the reference's own backward with its atomics in
    # index order (total), in the opposite order (total_rev), with double-accumulated sums (total_f64) and with every term perturbed by
    # a few ulp (total_probe) -- all deterministic -- say what accumulation order and evaluation differences do to each Gaussian; HIP
    # must be within 1e-4 * scale + NOISE_K x that of the double-accumulated result.  Every other tensor: the plain bar, no exception.  No retry: the criterion is evaluated for every one of ``repeats`` draws
    # of the HIP backward.
    shaped = lambda t: {n: t[n].reshape(model.params[n].shape) for n in model.NAMES}   # noqa: E731
    want, want_rev, want_f64, want_probe = shaped(total), shaped(total_rev), shaped(total_f64), shaped(total_probe)
    reports = []
    for draw in range(repeats):
        if draw > 0:
            model.flat_grad.fill_(float("nan"))
            for b, (rs, xyz, out_means3D, radii, feats, opacity, ts, scaling, scaling_t, rotation, rotation_r, pv, geom, R, binb, img, g_color) in enumerate(views):
                raw_backward(rs, xyz, out_means3D, radii, feats, opacity, ts, scaling, scaling_t, rotation, rotation_r, pv,
                             geom, R, binb, img, g_color, None, None, None, sink, b > 0, grad_accum=gacc)
            torch.cuda.synchronize()
        got = {n: model.params[n].grad.detach().cpu().numpy() for n in model.NAMES}
        assert float(np.abs(got["_features"][:, n_active:]).max(initial=0.0)) == 0.0, "%s: a coefficient beyond the %d active ones received a gradient" % (label, n_active)
        assert float(np.abs(got["_features"][:, :n_active]).max()) > 0.0
        if dump is not None:
            dump.append({n: got[n].copy() for n in chain})
            if draw == 0:
                dump.append(dict(want=want, want_rev=want_rev, want_f64=want_f64, want_probe=want_probe))
            continue
        rep = check_backward_noise_aware(got, want, want_rev, want_f64, want_probe, "%s: accumulated gradient (draw %d of %d)" % (label, draw + 1, repeats), chain=chain)
        reports.append(rep)
    if dump is not None:
        return None
    rep = reports[0]
    print("%s accumulated raw-parameter gradients over %d views (max abs err / max|ref|):" % (label, n_views), fmt_noise_rep(rep))
    just = {}
    for n in model.NAMES:
        spread = float(np.abs(want_rev[n] - want[n]).max())
        just[n] = "hip-ref %.2e | ref-ref' %.2e | hip-f64 %.2e | ref-f64 %.2e | passed by: %s" % (
            rep[n][1], spread, float(np.abs(got[n] - want_f64[n]).max()), float(np.abs(want[n] - want_f64[n]).max()), rep[n][0])
    print("%s covariance-chain justification (max abs over the tensor; ref' = reference with its atomics in reverse order, f64 = double-accumulated sums):" % label,
          {n: just[n] for n in chain})
    if repeats > 1:
        worst = {n: max(r[n][4] for r in reports) for n in chain}
        print("%s: %d draws of the HIP backward, all within the bars; worst |hip - f64| / conditioning-aware bound per tensor (NOISE_K = %g): %s; "
              "draws in which the tensor went beyond the plain bar: %s" % (label, repeats, NOISE_K, {n: "%.2f" % v for n, v in worst.items()},
                                                                          {n: sum(1 for r in reports if r[n][0] != "1e-4") for n in chain}))
    return just


@pytest.mark.parametrize("tile_cull", [False, True])
def test_timed_path_small_vs_oracle(tile_cull, gpu_device):
    """The timed path (see _timed_path_vs_oracle) on a small scene, with the reference's lists and with tile_cull."""
    _timed_path_vs_oracle(SC("v", 30000, 400, 304, 3, 2, 0.015, 10.0, True, 4, False), gpu_device, 2, "timed-small", 1e-3, tile_cull=tile_cull)


@pytest.mark.parametrize("mod,pv", [(0.5, 0.3), (2.0, 0.01)])
def test_timed_path_small_with_flags_vs_oracle(mod, pv, gpu_device):
    """The timed path (raw_params = 1, tile_cull = 1, colour-only backward, accumulation) with scale_modifier != 1 and
    prefilter_var > 0 (forward.cu:333, 418-434; backward.cu:746, 911-916): the activations' chain rule meets the modifier."""
    _timed_path_vs_oracle(SC("v", 12000, 320, 240, 3, 2, 0.015, 10.0, True, 4, False), gpu_device, 2, "timed-flags", 2e-3, tile_cull=True,
                          scale_modifier=mod, prefilter_var=pv)


@pytest.mark.parametrize("tile_cull", [True, False])
def test_c3_full_size_vs_oracle(tile_cull, gpu_device):
    """BASELINE configs[2] -- the configuration the metric is quoted on (300 k Gaussians, 1352x1014, M = 48) -- at
    FULL size through the path bench.py times (tile_cull = True; and with the reference's lists, bit for bit), 2 views
    accumulated, against the port oracle.  The views come from bench.py's cameras: the four rotated off-axis poses rig0..rig3
    (fdgs.synth.POSES; rig2 with the centre-shift projection), two per parametrisation."""
    _timed_path_vs_oracle(synth.CONFIGS["C3"], gpu_device, 2, "C3", 1e-3, tile_cull=tile_cull,
                          poses=["rig0", "rig2"] if tile_cull else ["rig1", "rig3"], repeats=REPEATS)


def test_c3_full_size_on_axis_camera_vs_oracle(gpu_device):
    """The same on the unrotated on-axis camera rounds 1-4 quoted the metric on (bench.py's value_axis_camera leg), one view."""
    _timed_path_vs_oracle(synth.CONFIGS["C3"], gpu_device, 1, "C3-axis", 1e-3, tile_cull=True, repeats=REPEATS)


@pytest.mark.parametrize("tile_cull", [False, True])
def test_c3_clustered_full_size_vs_oracle(tile_cull, gpu_device):
    """A skewed C3 (fdgs.synth C3-clustered: 70 % of the 300 k Gaussians on 15 % of the image, the bench's `clustered` leg): 3.2 M
    instances, 188 tile lists beyond 4096 entries (the 1024-thread instance of the LDS sort), the longest 5485 -- forward lists bit
    for bit (or, with tile_cull, instance by instance), pixels and all gradients against the oracle at the usual bar."""
    scene = synth.make_scene(synth.CONFIGS["C3-clustered"], seed=0)
    W, H = scene["W"], scene["H"]
    o = pyoracle.Oracle(scene, kind="port")
    ref = dict(o.forward())
    ref["R"] = o.R
    longest = int((ref["ranges"][:, 1].astype(np.int64) - ref["ranges"][:, 0]).max())
    assert longest > 4096 and ref["R"] > 3_000_000
    keep = torch.from_numpy(~ref["border"].astype(bool)).to(torch.float32)
    grads = synth.make_upstream_grads(W, H, seed=1, scale=GRAD_SCALE)
    grads = {k: v * keep.reshape((1,) * (v.dim() - 2) + (H, W)) for k, v in grads.items()}
    hip, hipg = run_hip(scene, gpu_device, grads, tile_cull=tile_cull)
    rep = check_forward(hip, ref, "C3-clustered", max_border=1e-3, tile_cull=tile_cull, WH=(W, H))
    refg, refg_rev, refg_f64, refg_probe = oracle_four_modes(o, grads)
    o.close()
    for draw in range(REPEATS):
        if draw > 0:
            _, hipg = run_hip(scene, gpu_device, grads, tile_cull=tile_cull)
        repg = check_backward_noise_aware(hipg, refg, refg_rev, refg_f64, refg_probe, "C3-clustered (draw %d of %d)" % (draw + 1, REPEATS), chain=CHAIN_ACTIVATED)
        print("C3-clustered R", ref["R"], "longest list", longest, rep.get("instances", ""), fmt_noise_rep(repg))


def test_c5_full_size_forward_backward_vs_oracle(gpu_device):
    """BASELINE configs[4] (2 M Gaussians, 2704x2028, R = 15.9 M): forward AND backward at full size against the port oracle
    (reference backward.cu:926-1137 + :486-923), both blend-backward variants: all four upstream gradients (AUX) and
    colour only.  As on C3 the upstream gradients are zeroed on the oracle-flagged cliff pixels on both sides; the bar is
    1e-4 * max(1, max|ref|) per tensor; an element of the four covariance-chain tensors beyond it: the conditioning-aware bar
    (tests/util.py::check_backward_noise_aware; see _timed_path_vs_oracle)."""
    # (round 5: through a rotated, off-axis camera with the centre-shift projection -- what bench.py's c5 leg renders)
    scene = synth.make_scene(synth.CONFIGS["C5"], seed=0, pose="rig2")
    W, H = scene["W"], scene["H"]
    o = pyoracle.Oracle(scene, kind="port")
    ref = dict(o.forward())
    ref["R"] = o.R
    keep = torch.from_numpy(~ref["border"].astype(bool)).to(torch.float32)
    grads = synth.make_upstream_grads(W, H, seed=1, scale=GRAD_SCALE)
    grads = {k: v * keep.reshape((1,) * (v.dim() - 2) + (H, W)) for k, v in grads.items()}
    for variant in ("aux", "colour-only"):
        if variant == "aux":
            hip_in, ora_in = grads, grads
        else:
            hip_in = {k: (v if k == "grad_color" else None) for k, v in grads.items()}
            ora_in = {k: (v if k == "grad_color" else torch.zeros_like(v)) for k, v in grads.items()}
        hip, hipg = run_hip(scene, gpu_device, hip_in)
        if variant == "aux":
            rep = check_forward(hip, ref, "C5", max_border=5e-4)
            print("C5 R", ref["R"], rep)
        refg, refg_rev, refg_f64, refg_probe = oracle_four_modes(o, ora_in)   # the reference's atomics in its two orders, and double-accumulated sums
        for draw in range(REPEATS):
            if draw > 0:
                _, hipg = run_hip(scene, gpu_device, hip_in)
            repg = check_backward_noise_aware(hipg, refg, refg_rev, refg_f64, refg_probe, "C5 %s (draw %d of %d)" % (variant, draw + 1, REPEATS), chain=CHAIN_ACTIVATED)
            print("C5 %s gradients (max abs err / max|ref|):" % variant, fmt_noise_rep(repg))
    o.close()


# ----------------------------------------------------------------------------------------------------------------
# tile binning (csrc/tilebin.hip): every path of the per-tile sort and of the count / scatter passes
# ----------------------------------------------------------------------------------------------------------------

def _binning_vs_oracle(scene, dev, label):
    hip, _ = run_hip(scene, dev, None)
    ref, _ = run_oracle(scene, None, kind="port")
    assert hip["R"] == ref["R"], label
    np.testing.assert_array_equal(hip["point_list"], ref["point_list"], err_msg=label + " point_list")
    np.testing.assert_array_equal(hip["ranges"], ref["ranges"], err_msg=label + " ranges")
    return hip, ref


@pytest.mark.parametrize("limits", [(0, 0), (64, 0), (0, 1), (2, 0)], ids=["default", "global-scratch", "lds-bitonic", "all-global"])
def test_tile_sort_paths(limits, gpu_device):
    """The per-tile sort has three paths (bucket + rank in LDS, bitonic in LDS for crowded depth buckets, bitonic in
    global scratch for lists longer than the LDS takes); the debug limits force each of them on an ordinary scene.
    point_list / ranges must stay bit-identical to the oracle's (tile, depth bits, id) order."""
    from fdgs import _capi
    scene = synth.make_scene(SC("v", 20000, 320, 240, 1, 0, 0.03, 1.0, True, 4, True), seed=11)
    try:
        _capi.lib.fdgs_debug_tile_sort_limits(*limits)
        hip, ref = _binning_vs_oracle(scene, gpu_device, "limits %r" % (limits,))
        assert (ref["ranges"][:, 1].astype(np.int64) - ref["ranges"][:, 0]).max() > 256   # lists long enough to matter
    finally:
        _capi.lib.fdgs_debug_tile_sort_limits(0, 0)


def test_tile_sort_equal_and_clustered_depths(gpu_device):
    """Depth ties and clusters: (a) every Gaussian at exactly the same view depth -> inside a tile the order is the
    Gaussian id (the reference's stable sort); (b) two thin depth layers plus a few far outliers, which
    stretch a tile's depth range so that one bucket of the first sorting step holds most of the list."""
    cfg = SC("v", 12000, 256, 192, 0, 0, 0.04, 1.0, False, 3, True)
    scene = synth.make_scene(cfg, seed=12)
    scene["means3D"] = scene["means3D"].clone()
    scene["means3D"][:, 2] = 0.25                      # camera looks down +z: identical depth bits
    hip, ref = _binning_vs_oracle(scene, gpu_device, "equal depths")
    db = ref["depths"][ref["radii"] > 0].view(np.uint32)
    assert len(np.unique(db)) == 1 and ref["R"] > 30000
    scene = synth.make_scene(cfg, seed=13)
    z = scene["means3D"][:, 2].clone()
    g = torch.Generator().manual_seed(5)
    u = torch.rand(z.shape[0], generator=g)
    z = torch.where(u < 0.6, 0.2 + 1e-4 * torch.randn(z.shape[0], generator=g), 0.9 + 1e-3 * torch.randn(z.shape[0], generator=g))
    z = torch.where(u > 0.99, 60.0 * torch.rand(z.shape[0], generator=g) + 2.0, z)
    scene["means3D"] = scene["means3D"].clone()
    scene["means3D"][:, 2] = z
    _binning_vs_oracle(scene, gpu_device, "clustered depths")


def test_tile_sort_long_lists(gpu_device):
    """Few tiles, many Gaussians: lists of several thousand entries.  The second sort launch takes every list beyond 2048 entries
    with ONE instance chosen by the longest list of the view -- 512 threads x 8 keys (longest 3082), 1024 x 8 (6653), 1024 x 16
    (11574), and 1024 x 16 plus, unforced, the global-scratch path for the four lists beyond the 16384 the LDS takes (18088)."""
    longest = []
    for P, W, H in ((30000, 128, 96), (40000, 96, 64), (70000, 96, 64), (110000, 96, 64)):
        scene = synth.make_scene(SC("v", P, W, H, 0, 0, 0.03, 1.0, True, 4, True), seed=15)
        hip, ref = _binning_vs_oracle(scene, gpu_device, "long lists %dx%d" % (W, H))
        n = ref["ranges"][:, 1].astype(np.int64) - ref["ranges"][:, 0]
        longest.append(int(n.max()))
        rep = check_forward(hip, ref, "long lists %d on %dx%d" % (P, W, H))
        print("long lists %d on %dx%d: longest %d, %d lists beyond 2048" % (P, W, H, n.max(), int((n > 2048).sum())), rep)
    assert 2048 < longest[0] <= 4096 < longest[1] <= 8192 < longest[2] <= 16384 < longest[3], longest


def test_forward_run_ahead_matches_exact_path(gpu_device):
    """The forward enqueues scatter / sort / blend before the host knows num_rendered, with buffers sized by the thread's
    previous call for the same (device, W, H, P) (capi.hip "run-ahead"); debug mode takes the exact path (wait, then size).  A
    sequence of scenes of ONE size that makes every guess wrong in turn -- more instances than the capacity, longer lists than the
    sort instances launched, twice over, then much smaller again -- must
    give bit-identical results either way (the forward is deterministic: no float atomics)."""
    from fdgs import _capi
    cfg = SC("ra", 30011, 320, 240, 0, 0, 0.03, 1.0, True, 4, True)   # a P no other test uses: the first call has no guess

    def variant(k_mean, k_scale):
        sc = synth.make_scene(cfg, seed=40)
        sc["means3D"] = (sc["means3D"] * torch.tensor([k_mean, k_mean, 1.0])).contiguous()
        sc["scales"] = (sc["scales"] * k_scale).contiguous()
        return sc

    seq = [("a", 1.0, 0.25),    # small splats: R ~ 55 k
           ("b", 1.0, 1.0),     # R ~ 129 k: over the capacity guessed from a
           ("c", 0.5, 0.45),    # drawn towards the image centre: fewer instances, lists of ~2100 where ~980 were the longest
           ("d", 0.3, 0.45),    # lists beyond 4096: twice what the launched instances take
           ("e", 1.0, 0.15),    # small again: everything fits
           ("f", 1.0, 0.8),     # back up: over capacity
           ("g", 1.0, 0.8)]     # same sizes again: the guess fits
    longest, paths, Rs = [], [], []
    for name, km, ks in seq:
        scene = variant(km, ks)
        before = _capi.run_ahead_stats()
        fast, _ = run_hip(scene, gpu_device, None)
        paths.append(tuple(b - a for a, b in zip(before, _capi.run_ahead_stats())))
        exact, _ = run_hip(dict(scene, debug=True), gpu_device, None)
        label = "run-ahead step %s" % name
        assert fast["R"] == exact["R"], label
        for key in ("point_list", "ranges", "n_contrib", "final_T", "out_color", "out_depth", "out_flow", "radii"):
            np.testing.assert_array_equal(fast[key], exact[key], err_msg="%s %s" % (label, key))
        longest.append(int((exact["ranges"][:, 1].astype(np.int64) - exact["ranges"][:, 0]).max()))
        Rs.append(exact["R"])
    print("run-ahead sequence: R", Rs, "longest list per step", longest, "path (kept, sorted again, exact) per step", paths)
    assert paths == [(0, 0, 1), (0, 0, 1), (0, 1, 0), (0, 1, 0), (1, 0, 0), (0, 0, 1), (1, 0, 0)], paths
    assert longest[3] > 4096 > longest[2] + longest[2] // 4 and longest[2] > longest[1] + longest[1] // 4 and Rs[1] > 2 * Rs[0]


def test_sort_again_borrows_scratch_for_lists_beyond_the_lds(gpu_device):
    """The run-ahead forward that has to sort again, with lists longer than the LDS takes in a binning buffer that was sized without
    the global sort scratch (the guess knew only lists that fit): the scratch is borrowed from the stream-ordered allocator for that one
    call.  The LDS limit is lowered (fdgs_debug_tile_sort_limits) to lie between the guessed longest list and the real one; every output
    equals the exact path's bit for bit."""
    from fdgs import _capi
    cfg = SC("ra2", 30029, 320, 240, 0, 0, 0.03, 1.0, True, 4, True)   # a P no other test uses: the guess is this test's own

    def variant(k_mean, k_scale):
        sc = synth.make_scene(cfg, seed=40)
        sc["means3D"] = (sc["means3D"] * torch.tensor([k_mean, k_mean, 1.0])).contiguous()
        sc["scales"] = (sc["scales"] * k_scale).contiguous()
        return sc

    def longest_of(res):
        return int((res["ranges"][:, 1].astype(np.int64) - res["ranges"][:, 0]).max())

    b, c = variant(1.0, 1.0), variant(0.5, 0.45)   # steps "b" and "c" of test_forward_run_ahead_matches_exact_path
    exact, _ = run_hip(dict(c, debug=True), gpu_device, None)
    L_c = longest_of(exact)
    guess, _ = run_hip(b, gpu_device, None)        # leaves the guess behind: capacity from R_b, sort instances for L_b + L_b // 4
    L_b = longest_of(guess)
    cap = L_b + L_b // 4
    print("sort again with borrowed scratch: R", guess["R"], exact["R"], "longest", L_b, L_c, "LDS limit", cap)
    assert L_c > cap, (L_b, L_c)
    try:
        _capi.lib.fdgs_debug_tile_sort_limits(cap, 0)
        before = _capi.run_ahead_stats()
        fast, _ = run_hip(c, gpu_device, None)
        assert tuple(y - x for x, y in zip(before, _capi.run_ahead_stats())) == (0, 1, 0)
    finally:
        _capi.lib.fdgs_debug_tile_sort_limits(0, 0)
    assert fast["R"] == exact["R"]
    for key in ("point_list", "ranges", "n_contrib", "final_T", "out_color", "out_depth", "out_flow", "radii"):
        np.testing.assert_array_equal(fast[key], exact[key], err_msg="sort again, borrowed scratch: " + key)


def test_run_ahead_can_be_switched_off(gpu_device):
    """fdgs_set_run_ahead(0): every forward waits for num_rendered and sizes the binning buffer exactly (the reference's contract)."""
    from fdgs import _capi
    scene = synth.make_scene(SC("ro", 5000, 160, 128, 0, 0, 0.03, 1.0, True, 4, True), seed=3)
    try:
        _capi.lib.fdgs_set_run_ahead(0)
        run_hip(scene, gpu_device, None)
        before = _capi.run_ahead_stats()
        a, _ = run_hip(scene, gpu_device, None)
        assert tuple(y - x for x, y in zip(before, _capi.run_ahead_stats())) == (0, 0, 1)
    finally:
        _capi.lib.fdgs_set_run_ahead(1)
    before = _capi.run_ahead_stats()
    b, _ = run_hip(scene, gpu_device, None)
    assert tuple(y - x for x, y in zip(before, _capi.run_ahead_stats())) == (1, 0, 0)
    for key in ("point_list", "ranges", "out_color", "n_contrib"):
        np.testing.assert_array_equal(a[key], b[key])


@pytest.mark.parametrize("cfg", [SC("s4", 20000, 320, 240, 3, 2, 0.03, 10.0, True, 4, False), SC("s3", 9000, 208, 160, 2, 0, 0.03, 1.0, False, 3, True),
                                 SC("s0", 5000, 160, 128, 0, 0, 0.03, 1.0, True, 4, True)], ids=["4d-sh", "3d-sh", "deg0"])
def test_split_colour_forward_is_bit_identical(cfg, gpu_device):
    """fdgs_forward_out.split_colour: geometry and SH colour as two launches, the second on the library's own stream next to the
    tile binning.  Same arithmetic: every forward output, the blend records and the clamp bits equal the one-launch forward bit
    for bit; the backward that follows reads the same buffers."""
    from fdgs.gaussian_renderer.diff_gaussian_rasterization import _C
    from util import native_args_fwd, scene_to_device, collect_forward
    scene = synth.make_scene(cfg, seed=61)
    sc = scene_to_device(scene, gpu_device)
    P, W, H = int(sc["means3D"].shape[0]), int(sc["W"]), int(sc["H"])
    outs = []
    for split in (False, True, True):   # twice: the second split call runs ahead of num_rendered
        res = _C.rasterize_gaussians(*native_args_fwd(sc), split_colour=split)
        outs.append(collect_forward(res, P, W, H))
    for other in outs[1:]:
        for key in ("R", "out_color", "out_flow", "out_depth", "out_T", "radii", "n_contrib", "final_T", "point_list", "ranges", "rgb",
                    "clamped_bits", "conic_opacity", "means2D", "rec_depth", "rec_flow"):
            np.testing.assert_array_equal(outs[0][key], other[key], err_msg="split_colour %s" % key)
    assert (outs[0]["rgb"] != 0).any() and outs[0]["R"] > 0


@pytest.mark.parametrize("cfg", [SC("o1", 40000, 640, 480, 0, 0, 0.02, 1.0, True, 4, True), SC("o2", 3000, 100, 36, 0, 0, 0.03, 1.0, True, 4, True),
                                 SC("o3", 3000, 3104, 3104, 0, 0, 0.02, 1.0, True, 4, True)], ids=["1200-tiles", "21-tiles", "37636-tiles"])
def test_tile_order_is_a_longest_first_permutation_dealt_evenly(cfg, gpu_device):
    """The order in which the blend kernels take the tiles (fdgs_debug_view.tile_order, written by the tile scan): a permutation of ALL
    tiles with the longer lists first (64 length classes of the longest list: monotone up to one class width); position p goes to XCD
    p % 8 (blend_common.h, block_of), so the XCDs' shares of the instances differ by no more than a few lists -- whatever part of the
    image the scene covers (rounds 2-4 gave every XCD a contiguous eighth of the tiles: its share of the work was that band's share of
    the scene)."""
    scene = synth.make_scene(cfg, seed=21)
    hip, _ = run_hip(scene, gpu_device, None)
    order, rg = hip["tile_order"], hip["ranges"].astype(np.int64)
    T = rg.shape[0]
    assert order.shape == (T,) and np.array_equal(np.sort(order), np.arange(T))
    n = rg[:, 1] - rg[:, 0]
    width = (int(n.max()) + 1) / 64.0 + 1.0
    ln = n[order]
    assert (ln[:-1] + width >= ln[1:]).all(), "not longest-first"
    share = np.array([int(ln[x::8].sum()) for x in range(8)])
    # (one list more or less where 8 does not divide T, plus a class width per tile taken)
    assert share.max() - share.min() <= n.max() + width * (-(-T // 8)) and share.max() - share.min() <= 0.02 * share.mean() + 2 * n.max(), share
    # the contiguous bands of rounds 2-4 on this scene, for the record
    band = -(-T // 8)
    print("instances per XCD: dealt", share.tolist(), "contiguous bands", [int(n[b * band:(b + 1) * band].sum()) for b in range(8)])
    assert n.max() > 0


def test_binning_many_tiles_direct_path(gpu_device):
    """More tiles than an LDS histogram holds (> 36 864): count / scatter fall back to one global atomic per instance."""
    scene = synth.make_scene(SC("v", 3000, 3104, 3104, 0, 0, 0.02, 1.0, True, 4, True), seed=14)
    assert ((3104 + 15) // 16) ** 2 > 36 * 1024
    hip, ref = _binning_vs_oracle(scene, gpu_device, "direct")
    assert ref["R"] > 3000


# ----------------------------------------------------------------------------------------------------------------
# fdgs_forward_out.lazy: the forward that never waits for num_rendered
# ----------------------------------------------------------------------------------------------------------------

def test_lazy_forward_matches_waiting_forward_and_reports_overflow(gpu_device):
    """A lazy forward returns num_rendered = -1 without touching the device; every output equals the waiting forward's bit for bit,
    the backward takes the -1, and fdgs_forward_lazy_status reports the count afterwards.  A view that outgrows the run-ahead
    buffers (1.5 x the largest of the last four reports) is REPORTED as failed -- its image is not to be used."""
    from fdgs import _capi
    from fdgs.gaussian_renderer.diff_gaussian_rasterization import _C
    from util import collect_forward, native_args_fwd, scene_to_device
    cfg = SC("lz", 20023, 320, 240, 2, 0, 0.03, 1.0, True, 4, True)   # a P no other test uses: the thread has no guess for it yet
    scene = synth.make_scene(cfg, seed=8)
    sc = scene_to_device(scene, gpu_device)
    P, W, H = cfg.P, cfg.W, cfg.H
    _capi.forward_lazy_status(gpu_device, wait=True)   # whatever other tests left behind
    first = _C.rasterize_gaussians(*native_args_fwd(sc), lazy=True)
    assert first[0] > 0, "the first call for a configuration cannot run ahead: it must behave like a waiting call"
    want = collect_forward(first, P, W, H)
    res = _C.rasterize_gaussians(*native_args_fwd(sc), lazy=True)
    assert res[0] == -1
    pend, failed, reported = _capi.forward_lazy_status(gpu_device, wait=True)
    assert (pend, failed, reported) == (0, 0, [want["R"]]), (pend, failed, reported, want["R"])
    got = collect_forward((want["R"],) + tuple(res[1:]), P, W, H)
    for key in ("point_list", "ranges", "n_contrib", "final_T", "out_color", "out_depth", "out_flow", "radii"):
        np.testing.assert_array_equal(got[key], want[key], err_msg="lazy forward: " + key)
    # the backward with num_rendered = -1
    grads = synth.make_upstream_grads(W, H, seed=1, scale=GRAD_SCALE)
    e = torch.Tensor([])
    g = lambda k: sc[k] if sc.get(k) is not None else e  # noqa: E731
    outs = []
    for r in (first, res):
        (R, color, flow, depth, T, radii, geom, binb, img, covs_com, out_means3D) = r
        gd = {k: v.to(gpu_device) for k, v in grads.items()}
        bargs = (sc["bg"], sc["means3D"], out_means3D, radii, g("colors_precomp"), g("flow_2d"), sc["opacities"], g("ts"), g("scales"),
                 g("scales_t"), g("rotations"), g("rotations_r"), 1.0, g("cov3D_precomp"), -1.0, sc["world_view_transform"],
                 sc["full_proj_transform"], sc["tanfovx"], sc["tanfovy"], gd["grad_color"], gd["grad_depth"], gd["grad_alpha"], gd["grad_flow"],
                 g("shs"), sc["sh_degree"], sc["sh_degree_t"], sc["camera_center"], sc["timestamp"], sc["time_duration"], sc["rot_4d"],
                 sc["gaussian_dim"], sc["force_sh_3d"], geom, R, binb, img, False)
        outs.append([t.cpu().numpy() for t in _C.rasterize_gaussians_backward(*bargs)])
    for a, b in zip(*outs):
        scale = max(1.0, float(np.abs(a).max()))
        assert float(np.abs(a - b).max()) <= 1e-5 * scale   # float atomics: summation order differs run to run
    # a view with splats twice the size (2.3 x the instances, 2.2 x the longest list): reported as failed, and the waiting call that follows is right
    big = dict(scene)
    big["scales"] = (scene["scales"] * 2.0).contiguous()
    bsc = scene_to_device(big, gpu_device)
    res_big = _C.rasterize_gaussians(*native_args_fwd(bsc), lazy=True)
    assert res_big[0] == -1
    pend, failed, reported = _capi.forward_lazy_status(gpu_device, wait=True)
    # (here through the longest list: ~1400 entries where 1.5 x 650 + 64 were provided for -- the sort instances launched do not take it)
    assert pend == 0 and failed == 1 and len(reported) == 1 and reported[0] > 2 * want["R"], (failed, reported, want["R"])
    sync_big = _C.rasterize_gaussians(*native_args_fwd(bsc))
    assert sync_big[0] == reported[0]
    ref, _ = run_oracle(big, None, kind="port")
    assert ref["R"] == sync_big[0]
    np.testing.assert_array_equal(collect_forward(sync_big, P, W, H)["point_list"], ref["point_list"])
    # ... and the guess has learnt the new size: the next lazy forward of the big view fits
    res_big2 = _C.rasterize_gaussians(*native_args_fwd(bsc), lazy=True)
    pend, failed, reported = _capi.forward_lazy_status(gpu_device, wait=True)
    assert res_big2[0] == -1 and failed == 0 and reported == [sync_big[0]]
    np.testing.assert_array_equal(collect_forward((sync_big[0],) + tuple(res_big2[1:]), P, W, H)["out_color"], collect_forward(sync_big, P, W, H)["out_color"])


def test_mailbox_ring_wraps_correctly_in_a_fresh_thread(gpu_device):
    """The tile scans report num_rendered through a ring of 64 pinned slots per host thread and device.  A fresh thread issues 70
    waiting and 70 lazy forwards: every one of them -- the 64th and 65th in particular, where the ring wraps -- must return /
    report the right count and render the same image (regression: the 64th forward of a thread used to read its slot before the
    scan had written it, returned num_rendered = 0 whenever the host was faster than the kernel, and the backward that was handed
    that 0 skipped the view)."""
    import threading
    from fdgs import _capi
    from fdgs.gaussian_renderer.diff_gaussian_rasterization import _C
    from util import native_args_fwd, scene_to_device
    scene = synth.make_scene(SC("ring", 3000, 160, 128, 0, 0, 0.03, 1.0, True, 4, True), seed=12)
    sc = scene_to_device(scene, gpu_device)
    want = _C.rasterize_gaussians(*native_args_fwd(sc))
    torch.cuda.synchronize()
    out = {}

    def work():
        try:
            torch.cuda.set_device(gpu_device)
            rs, bad = [], 0
            for i in range(70):
                res = _C.rasterize_gaussians(*native_args_fwd(sc))
                rs.append(res[0])
                bad += int(not torch.equal(res[1], want[1]))
            lazy_r = []
            for i in range(70):
                res = _C.rasterize_gaussians(*native_args_fwd(sc), lazy=True)
                assert res[0] == -1
                bad += int(not torch.equal(res[1], want[1]))
                if i % 16 == 15:
                    pend, failed, reported = _capi.forward_lazy_status(gpu_device, wait=True)
                    assert failed == 0 and pend == 0
                    lazy_r += reported
            pend, failed, reported = _capi.forward_lazy_status(gpu_device, wait=True)
            lazy_r += reported
            out.update(rs=rs, lazy_r=lazy_r, bad=bad, failed=failed)
        except Exception as e:   # surfaces in the main thread
            out["error"] = repr(e)

    t = threading.Thread(target=work)
    t.start()
    t.join()
    assert "error" not in out, out.get("error")
    assert out["rs"] == [want[0]] * 70, out["rs"]
    assert out["lazy_r"] == [want[0]] * 70 and out["failed"] == 0 and out["bad"] == 0, (out["lazy_r"], out["bad"])

