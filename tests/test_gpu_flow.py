"""GPU: fdgs.flow.gaussian_flow (csrc/flow.hip) and ``flow_to`` of render() / render_raw() -- bit for bit against the product's own
projection, exact zeros, values and gradients against the float64 PyTorch statement (tests/flow_oracle.py), and the public path
against its composition by hand.  Images are 64 x 48, at most 1000 Gaussians."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import flow_cases as fc
import flow_oracle as fo
import util
from fdgs import synth

pytestmark = pytest.mark.gpu

W, H = fc.W, fc.H
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)
SEEDS = {1: 4, 63: 4, 64: 4, 65: 4, 255: 3, 256: 3, 257: 3, 1000: 3}   # at least half of the Gaussians visible in both views (checked below)
KINDS = {"rot4d-raw": (True, True), "rot4d-activated": (True, False), "plain4d": (False, False)}   # (rot_4d, raw)
CAMERAS = (("rig0", "rig0"), ("rig0", "rig1"))
DEV = "cuda:0"


def on_dev(par):
    return {n: t.to(DEV) for n, t in par.items()}


def cameras(s0, s1):
    """(source, target): with one pose the target is the source at another time (the NULL matrices of the C entry)."""
    from fdgs.playback import with_timestamp
    cam = fc.Cam(s0, DEV)
    if s0["world_view_transform"].equal(s1["world_view_transform"]):
        return cam, with_timestamp(cam, s1["timestamp"])
    return cam, fc.Cam(s1, DEV)


def flow_of(s0, s1, par, rot_4d, raw, mod=1.0, gaussian_dim=4):
    from fdgs.flow import gaussian_flow
    cam, cam_to = cameras(s0, s1)
    d = on_dev(par)
    return gaussian_flow(cam, cam_to, *[d[n] for n in fo.NAMES], rot_4d=rot_4d, gaussian_dim=gaussian_dim, raw=raw, scaling_modifier=mod)


def records(scene, par, raw, mod):
    """(means2D, radii) of an ordinary forward of ``scene`` with the six tensors of ``par``: the xy of the blend records (fdgs_debug_views)."""
    from fdgs.gaussian_renderer.diff_gaussian_rasterization import _C
    sc = dict(scene)
    sc.update(par)
    sc["scale_modifier"] = mod
    if raw:
        o = scene["opacities"].clamp(1e-6, 1 - 1e-6)
        sc["opacities"] = torch.log(o / (1 - o))
    sc = util.scene_to_device(sc, DEV)
    with torch.no_grad():
        res = _C.rasterize_gaussians(*util.native_args_fwd(sc), raw_params=raw)
    out = util.collect_forward(res, int(scene["P"]), W, H)
    return out["means2D"], out["radii"]


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("P", SIZES)
def test_flow_is_the_difference_of_the_forwards_records_bit_for_bit(gpu_device, P, kind):
    """1: flows[i] == records_to[i].xy - records_from[i].xy (float32, by torch) for every Gaussian with radii > 0 in both forwards; one
    and two cameras, scale modifier 1 and 0.7.  Bar 0: the same operations by construction.  At least half of the Gaussians qualify."""
    rot_4d, raw = KINDS[kind]
    for poses in CAMERAS:
        for mod in (1.0, 0.7):
            s0, s1 = fc.pair(P, rot_4d, poses, seed=SEEDS[P])
            par = fc.params_of(s0, raw)
            m0, r0 = records(s0, par, raw, mod)
            m1, r1 = records(s1, par, raw, mod)
            both = (r0 > 0) & (r1 > 0)
            assert both.mean() >= 0.5, "%s %s mod %g: only %d of %d Gaussians are visible in both views" % (kind, poses, mod, both.sum(), P)
            flows = flow_of(s0, s1, par, rot_4d, raw, mod)
            assert flows.shape == (P, 2) and flows.dtype == torch.float32 and bool(torch.isfinite(flows).all())
            want = (torch.from_numpy(m1) - torch.from_numpy(m0)).numpy()
            got = flows.cpu().numpy()
            bad = (fc.bits(got[both]) != fc.bits(want[both])).any(axis=1)
            assert not bad.any(), "%s %s mod %g: %d of %d flows differ from the records' difference" % (kind, poses, mod, bad.sum(), both.sum())
            if rot_4d or poses[0] != poses[1]:
                assert np.abs(want[both]).max() > 0.5, "the case should have motion"


def test_exact_zeros(gpu_device):
    """2: equal timestamps with one camera; plain 4D and 3D models with one camera: every flow is exactly 0."""
    for raw in (True, False):
        s0, s1 = fc.pair(257, True, ("rig1", "rig1"), t1=fc.T0)
        assert not bool(flow_of(s0, s1, fc.params_of(s0, raw), True, raw, 0.7).any())
    for dim in (4, 3):
        s0, s1 = fc.pair(257, False, ("rig1", "rig1"), gaussian_dim=dim)
        assert not bool(flow_of(s0, s1, fc.params_of(s0, False), False, False, gaussian_dim=dim).any())
        # ... and with two cameras the flow is the cameras' alone: the 4D tensors are not read
        s0, s1 = fc.pair(257, False, ("rig0", "rig1"), gaussian_dim=dim)
        par = fc.params_of(s0, False)
        a = flow_of(s0, s1, par, False, False, gaussian_dim=dim)
        poisoned = dict(par, **{n: torch.full_like(par[n], float("nan")) for n in fo.NAMES[1:]})
        assert bool(a.any()) and torch.equal(a, flow_of(s0, s1, poisoned, False, False, gaussian_dim=dim))


@pytest.mark.parametrize("poses", (("rig0", "slant"), ("slant", "rig0")))
@pytest.mark.parametrize("raw", (True, False))
def test_gaussians_behind_either_camera_have_no_flow_and_no_gradient(gpu_device, poses, raw):
    """2: the 'slant' camera stands inside the volume: part of the scene is behind it (view-space z <= 0.2), as source or as target.
    Those rows are exactly 0 in the flow and in all six gradients; the others are not."""
    s0, s1 = fc.pair(1000, True, poses)
    par = fc.params_of(s0, raw)
    _, _, _, ok = fo.gaussian_flow(*fc.cam_args(s0, s1), *[par[n] for n in fo.NAMES], rot_4d=True, raw=raw, details=True)
    behind = ~ok
    assert 10 <= int(behind.sum()) <= 990
    leaves = {n: t.clone().requires_grad_(True) for n, t in on_dev(par).items()}
    from fdgs.flow import gaussian_flow
    cam, cam_to = cameras(s0, s1)
    flows = gaussian_flow(cam, cam_to, *[leaves[n] for n in fo.NAMES], rot_4d=True, gaussian_dim=4, raw=raw)
    g = torch.Generator().manual_seed(2)
    flows.backward(torch.randn(1000, 2, generator=g).to(DEV))
    b = behind.to(DEV)
    assert not bool(flows[b].any()) and bool(flows[~b].any(dim=1).all())
    for n in fo.NAMES:
        grad = leaves[n].grad.reshape(1000, -1)
        assert bool(torch.isfinite(grad).all()) and not bool(grad[b].any()), n
        assert bool(grad[~b].any(dim=1).float().mean() > 0.99), n


VALUE_CASES = [(kind, poses, mod) for kind in ("rot4d-raw", "rot4d-activated") for poses in CAMERAS for mod in (1.0, 0.7)] + [
    ("plain4d", ("rig0", "rig1"), 1.0)]


@pytest.mark.parametrize("kind,poses,mod", VALUE_CASES)
def test_values_against_the_float64_statement(gpu_device, kind, poses, mod):
    """3: every element within 4 x the float32 oracle's own worst error on the case, over the Gaussians with both |pix| <= 4 max(W, H)
    (at most 10 % may fall outside).  Worst observed ratio: DESIGN.md section 4.9."""
    rot_4d, raw = KINDS[kind]
    P = 1000
    s0, s1 = fc.pair(P, rot_4d, poses)
    par = fc.params_of(s0, raw)
    args = [par[n] for n in fo.NAMES]
    f64, p0, p1, _ok = fo.gaussian_flow(*fc.cam_args(s0, s1), *args, rot_4d=rot_4d, raw=raw, scaling_modifier=mod, details=True)
    f32 = fo.gaussian_flow(*fc.cam_args(s0, s1), *args, rot_4d=rot_4d, raw=raw, scaling_modifier=mod, dtype=torch.float32)
    lim = 4.0 * max(W, H)
    inside = ((p0.abs().max(1).values <= lim) & (p1.abs().max(1).values <= lim)).numpy()
    assert inside.mean() >= 0.9, "pick another scene: %d of %d Gaussians project outside 4 max(W, H)" % ((~inside).sum(), P)
    own = float((f32.double() - f64).abs().numpy()[inside].max())
    got = flow_of(s0, s1, par, rot_4d, raw, mod).cpu().double()
    err = float((got - f64).abs().numpy()[inside].max())
    print("flow values %s %s mod %g: max |flow| %.1f px, kernel err %.3g, float32 oracle err %.3g, ratio %.2f (bar 4)" % (
        kind, poses, mod, float(f64.abs().max()), err, own, err / own))
    assert own > 0.0 and err <= 4.0 * own, "worst error %g > 4 x %g" % (err, own)


def backward_direct(s0, s1, par_dev, dL, rot_4d, raw, mod, scale, bufs):
    """fdgs_gaussian_flow_backward itself: ADDS scale * gradient into ``bufs`` (by flow_oracle.NAMES)."""
    from fdgs import _capi
    from fdgs.flow import _flow_in
    cam, cam_to = cameras(s0, s1)
    tensors = [par_dev[n].contiguous() for n in fo.NAMES]
    a, keep = _flow_in(cam, cam_to, tensors, rot_4d, 4, raw, mod)
    out = _capi.FdgsFlowGrads(*[None if b is None else b.data_ptr() for b in bufs])
    rc = _capi.lib.fdgs_gaussian_flow_backward(C.byref(a), dL.data_ptr(), float(scale), C.byref(out), _capi.current_stream_handle(dL.device))
    assert rc == 0, _capi.last_error()
    torch.cuda.synchronize()
    del keep


@pytest.mark.parametrize("mod", (1.0, 0.7))
@pytest.mark.parametrize("raw", (True, False))
def test_gradients_against_float64_autograd(gpu_device, raw, mod):
    """4: random dL_dflows, two cameras: all six gradients within 1e-4 * max(1, max|ref|) of float64 autograd of the oracle (the
    float32 oracle is itself within that bar on these inputs: asserted); two calls are bitwise equal; ``scale`` scales, and a second
    call doubles a zeroed buffer exactly (ADD)."""
    P = 1000
    s0, s1 = fc.pair(P, True, ("rig0", "rig1"))
    par = fc.params_of(s0, raw)
    dL = torch.randn(P, 2, generator=torch.Generator().manual_seed(11))
    _, g64 = fo.flow_with_grads(*fc.cam_args(s0, s1), par, dL, rot_4d=True, raw=raw, scaling_modifier=mod)
    _, g32 = fo.flow_with_grads(*fc.cam_args(s0, s1), par, dL, rot_4d=True, raw=raw, scaling_modifier=mod, dtype=torch.float32)
    leaves = {n: t.clone().requires_grad_(True) for n, t in on_dev(par).items()}
    from fdgs.flow import gaussian_flow
    cam, cam_to = cameras(s0, s1)
    got = []
    for _ in range(2):
        for t in leaves.values():
            t.grad = None
        flows = gaussian_flow(cam, cam_to, *[leaves[n] for n in fo.NAMES], rot_4d=True, gaussian_dim=4, raw=raw, scaling_modifier=mod)
        flows.backward(dL.to(DEV))
        got.append({n: leaves[n].grad.clone() for n in fo.NAMES})
    for n in fo.NAMES:
        ref = g64[n]
        scale = max(1.0, float(ref.abs().max()))
        own = float((g32[n].double() - ref).abs().max())
        err = float((got[0][n].cpu().double() - ref).abs().max())
        print("flow gradient raw=%s mod %g %-11s: max|ref| %.3g, kernel err / scale %.2e, float32 oracle err / scale %.2e" % (
            raw, mod, n, float(ref.abs().max()), err / scale, own / scale))
        assert float(ref.abs().max()) > 0.0
        assert own <= 1e-4 * scale, "the float32 oracle itself misses the bar on %s: pick other inputs" % n
        assert err <= 1e-4 * scale, "%s: max abs err %g > %g" % (n, err, 1e-4 * scale)
        assert torch.equal(got[0][n], got[1][n]), "%s: two calls differ" % n
    # scale and ADD, on the C entry itself
    par_dev = on_dev(par)
    bufs = [torch.zeros_like(par_dev[n]) for n in fo.NAMES]
    backward_direct(s0, s1, par_dev, dL.to(DEV), True, raw, mod, 0.5, bufs)
    once = [b.clone() for b in bufs]
    backward_direct(s0, s1, par_dev, dL.to(DEV), True, raw, mod, 0.5, bufs)
    for n, a, b in zip(fo.NAMES, once, bufs):
        assert torch.equal(b, a + a), "%s: the second call does not double the buffer" % n
        full = got[0][n]
        assert float((a - 0.5 * full).abs().max()) <= 1e-6 * max(1.0, float(full.abs().max())), "%s: scale" % n
    # NULL outputs are left out, the others are unchanged by that
    some = [torch.zeros_like(par_dev[n]) if n in ("means3D", "scales_t") else None for n in fo.NAMES]
    backward_direct(s0, s1, par_dev, dL.to(DEV), True, raw, mod, 0.5, some)
    assert torch.equal(some[0], once[0]) and torch.equal(some[3], once[3])


# ---- 5: through render() / render_raw() ----

class _Pipe:
    compute_cov3D_python = convert_SHs_python = debug = False
    env_map_res = 0


@functools.lru_cache(maxsize=None)
def block_scene(rot_4d=True):
    """One small Gaussian at the centre of every 8 x 8 pixel block of the image (48 Gaussians, radius <= 3 pixels: each stays inside its
    block), seen by the on-axis camera at the Gaussians' own time, so that no mean has moved.  The blend backward adds one partial sum
    per (block, Gaussian) to the Gaussian's accumulators with float atomics; with one contributing block per Gaussian there is nothing
    whose order could change, and the rasterizer's gradients are bitwise reproducible -- what 'bit-identical' and the 1e-6 bar for the
    order of the two routes' sum need."""
    P = (W // 8) * (H // 8)
    cfg = synth.SceneConfig("flow-blocks", P, W, H, 1, 0, 0.02, 1.0, rot_4d, 4, False)
    scene = synth.make_scene(cfg, seed=6, pose="axis", timestamp_frac=fc.T0, rot_sigma=0.1, bg=(0.1, 0.2, 0.3))
    focal, depth = 0.9 * W, 4.0
    cx = torch.arange(W // 8, dtype=torch.float64).repeat(H // 8) * 8 + 3.5
    cy = torch.arange(H // 8, dtype=torch.float64).repeat_interleave(W // 8) * 8 + 3.5
    xyz = torch.stack([(cx + 0.5 - W / 2) * depth / focal, (cy + 0.5 - H / 2) * depth / focal, torch.zeros(P, dtype=torch.float64)], dim=1)
    scene["means3D"] = xyz.float().contiguous()
    scene["ts"] = torch.full((P, 1), scene["timestamp"])
    scene["opacities"] = scene["opacities"].clamp(0.3, 0.9)
    target = synth.make_scene(cfg, seed=6, pose="rig1", timestamp_frac=fc.T1, rot_sigma=0.1)
    return scene, target


def model_and_cameras(rot_4d=True):
    from fdgs.train_host import GaussianParams
    scene, target = block_scene(rot_4d)
    model = GaussianParams(scene, torch.device(DEV))
    return scene, model, fc.Cam(scene, DEV), fc.Cam(target, DEV), scene["bg"].to(DEV)


GEOMETRY = ("_xyz", "_t", "_scaling", "_scaling_t", "_rotation", "_rotation_r")


def grads_of(model, names=GEOMETRY + ("_opacity", "_features")):
    return {n: model.params[n].grad.clone() for n in names}


def settings_of(cam, model, bg):
    from fdgs.gaussian_renderer.diff_gaussian_rasterization import GaussianRasterizationSettings
    return GaussianRasterizationSettings(
        image_height=int(cam.image_height), image_width=int(cam.image_width), tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5),
        bg=bg, scale_modifier=1.0, viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, sh_degree=model.active_sh_degree,
        sh_degree_t=model.active_sh_degree_t, campos=cam.camera_center, timestamp=cam.timestamp,
        time_duration=model.time_duration[1] - model.time_duration[0], rot_4d=model.rot_4d, gaussian_dim=model.gaussian_dim,
        force_sh_3d=model.force_sh_3d, prefiltered=False, debug=False)


def check_block_scene(pkg, P):
    radii = pkg["radii"].cpu().numpy()
    assert radii.shape == (P,) and (radii > 0).all() and radii.max() <= 3, "every Gaussian visible and inside its 8 x 8 block: radii %s" % radii


def test_render_feeds_the_flow_and_sums_both_gradient_routes(gpu_device):
    """5: render(flow_to=cam_to)['flow'] is, bitwise, the rasterizer fed gaussian_flow(activated getters) as flow_2d; with a loss on
    'flow' only the parameter gradients are the rasterizer backward with flow_2d as a leaf, plus the flow backward on its dL_dflows,
    to 1e-6 * max(1, max|.|) (the order in which autograd sums the two routes)."""
    from fdgs.flow import model_flow
    from fdgs.gaussian_renderer import render
    from fdgs.gaussian_renderer.diff_gaussian_rasterization import GaussianRasterizer
    scene, model, cam, cam_to, bg = model_and_cameras()
    P = int(scene["P"])
    up = torch.randn(2, H, W, generator=torch.Generator().manual_seed(4)).to(DEV)
    model.zero_grad()
    pkg = render(cam, model, _Pipe(), bg, flow_to=cam_to)
    check_block_scene(pkg, P)
    assert bool(pkg["flow"].any()) and pkg["flow"].shape == (2, H, W)
    (pkg["flow"] * up).sum().backward()
    torch.cuda.synchronize()
    public = grads_of(model)

    # by hand: flow_2d as a leaf of the same rasterizer call
    model.zero_grad()
    leaf = model_flow(cam, cam_to, model, raw=False).detach().clone().requires_grad_(True)
    assert float(leaf.detach().abs().max()) > 1.0
    means2D = torch.zeros_like(model.get_xyz, requires_grad=True)
    image, radii, depth, alpha, flow, _covs = GaussianRasterizer(settings_of(cam, model, bg))(
        means3D=model.get_xyz, means2D=means2D, shs=model.get_features, colors_precomp=None, flow_2d=leaf, opacities=model.get_opacity,
        ts=model.get_t, scales=model.get_scaling, scales_t=model.get_scaling_t, rotations=model.get_rotation, rotations_r=model.get_rotation_r,
        cov3D_precomp=None, prefilter_var=-1.0)
    assert torch.equal(flow, pkg["flow"]) and torch.equal(image, pkg["render"]) and torch.equal(alpha, pkg["alpha"])
    (flow * up).sum().backward()
    route_a = grads_of(model)
    assert bool(leaf.grad.any())
    model.zero_grad()
    model_flow(cam, cam_to, model, raw=False).backward(leaf.grad)
    route_b = grads_of(model)
    for n in public:
        want = route_a[n] + route_b[n]
        tol = 1e-6 * max(1.0, float(want.abs().max()))
        assert float((public[n] - want).abs().max()) <= tol, n
    for n in GEOMETRY:
        assert bool(route_a[n].any()) or n in ("_t",), n
        assert bool(route_b[n].any()), "the flow route reaches %s" % n
    assert not bool(route_b["_opacity"].any()) and not bool(route_b["_features"].any())


def test_render_raw_feeds_the_flow_and_sums_both_gradient_routes(gpu_device):
    """5: the same for render_raw: the flow of the RAW parameters, the native forward / backward with ``flows`` by hand."""
    from fdgs.flow import model_flow
    from fdgs.fused import raw_backward, raw_forward, raw_settings, render_raw
    scene, model, cam, cam_to, bg = model_and_cameras()
    P = int(scene["P"])
    up = torch.randn(2, H, W, generator=torch.Generator().manual_seed(4)).to(DEV)
    model.zero_grad()
    pkg = render_raw(cam, model, _Pipe(), bg, flow_to=cam_to)
    check_block_scene(pkg, P)
    (pkg["flow"] * up).sum().backward()
    torch.cuda.synchronize()
    public = grads_of(model)
    with pytest.raises(ValueError, match="grad_sink"):
        render_raw(cam, model, _Pipe(), bg, grad_sink=model.grad_sink(), flow_to=cam_to)

    rs, (xyz, feats, opacity, ts, scaling, scaling_t, rotation, rotation_r, pv) = raw_settings(cam, model, _Pipe(), bg)
    leaf = model_flow(cam, cam_to, model, raw=True).detach()
    with torch.no_grad():
        (R, color, flow, depth, T, radii, geom, binb, img, _c, om) = raw_forward(rs, xyz, feats, opacity, ts, scaling, scaling_t, rotation,
                                                                                 rotation_r, pv, flows=leaf)
        assert torch.equal(flow, pkg["flow"]) and torch.equal(color, pkg["render"])
        (_d2, _dc, d_op, d_xyz, _dcov, d_sh, d_flows, d_ts, d_s, d_st, d_r, d_rr) = raw_backward(
            rs, xyz, om, radii, feats, opacity, ts, scaling, scaling_t, rotation, rotation_r, pv, geom, R, binb, img, None, None, None, up,
            None, False, flows=leaf)
    route_a = {"_xyz": d_xyz, "_t": d_ts, "_scaling": d_s, "_scaling_t": d_st, "_rotation": d_r, "_rotation_r": d_rr, "_opacity": d_op,
               "_features": d_sh}
    assert d_flows is not None and bool(d_flows.any())
    model.zero_grad()
    model_flow(cam, cam_to, model, raw=True).backward(d_flows.reshape(P, 2))
    route_b = grads_of(model)
    for n in public:
        want = route_a[n].reshape(public[n].shape) + route_b[n]
        tol = 1e-6 * max(1.0, float(want.abs().max()))
        assert float((public[n] - want).abs().max()) <= tol, n
    for n in GEOMETRY:
        assert bool(route_b[n].any()), "the flow route reaches %s" % n
    # the blended image is sum_i flow_i alpha_i T_i: where one Gaussian covers a pixel alone, flow / alpha is that Gaussian's flow
    a = pkg["alpha"][0]
    centre = pkg["flow"][:, 3::8, 3::8].reshape(2, -1) / a[3::8, 3::8].reshape(1, -1)
    assert float((centre.t() - leaf).abs().max()) <= 1e-4 * max(1.0, float(leaf.abs().max()))


@pytest.mark.parametrize("which", ("render", "render_raw"))
def test_flow_to_none_is_todays_path(gpu_device, which):
    """5: flow_to=None: outputs and gradients bit-identical to a call that never mentions it (and the flow image is zero)."""
    from fdgs.fused import render_raw
    from fdgs.gaussian_renderer import render
    fn = render if which == "render" else render_raw
    scene, model, cam, _cam_to, bg = model_and_cameras()
    up = synth.make_upstream_grads(W, H, seed=1, scale=1e-2)
    out = []
    for kw in ({}, {"flow_to": None}):
        model.zero_grad()
        pkg = fn(cam, model, _Pipe(), bg, **kw)
        check_block_scene(pkg, int(scene["P"]))
        loss = ((pkg["render"] * up["grad_color"].to(DEV)).sum() + (pkg["depth"] * up["grad_depth"].to(DEV)).sum()
                + (pkg["alpha"] * up["grad_alpha"].to(DEV)).sum() + (pkg["flow"] * up["grad_flow"].to(DEV)).sum())
        loss.backward()
        torch.cuda.synchronize()
        out.append((pkg, grads_of(model), pkg["viewspace_points"].grad.clone()))
    (p0, g0, v0), (p1, g1, v1) = out
    for k in ("render", "depth", "alpha", "flow", "radii"):
        assert torch.equal(p0[k], p1[k]), k
    assert not bool(p0["flow"].any())
    assert torch.equal(v0, v1)
    for n in g0:
        assert bool(g0[n].any()) and torch.equal(g0[n], g1[n]), n


# ---- 6: element by element against the float64 statement (tests/flow_oracle.analytic, the cases of tests/flow_cases.CASES) ----
# Every element of ``flows`` and of the six gradients within K[family][tensor] * (4 ulp32 of |f64_e| + sens_e); no element is exempt.

import json  # noqa: E402

import chain_oracle as co  # noqa: E402
from guarded import Guarded  # noqa: E402

CASE_NAMES = [c.name for c in fc.CASES]
SHAPES = {"means3D": 3, "ts": 1, "scales": 3, "scales_t": 1, "rotations": 4, "rotations_r": 4}


@pytest.fixture(scope="module")
def worst_ratios():
    """The kernels' worst |hip - f64| / (4 ulp32 + sens) per family and tensor over the cases that ran: printed."""
    rep = {}
    yield rep
    print("\nflow kernels, worst ratio per family and tensor: " + json.dumps(
        {fam: {k: float("%.4g" % v) for k, v in sorted(d.items())} for fam, d in sorted(rep.items())}))


def case_cameras(case, b, form=None):
    from fdgs.playback import with_timestamp
    form = form or case.cams
    cam = fc.Cam(b["s0"], DEV)
    if form == "null":
        return cam, with_timestamp(cam, b["s1"]["timestamp"])
    cam_to = fc.Cam(b["s1"], DEV)    # "equal": the same pose in buffers of its own
    assert cam_to.world_view_transform.data_ptr() != cam.world_view_transform.data_ptr()
    assert form == "two" or torch.equal(cam_to.full_proj_transform, cam.full_proj_transform)
    return cam, cam_to


def case_inputs(case, b):
    """The six device tensors as the C entry takes them (None for what a model without rot_4d does not have)."""
    return [b["par"][n].to(DEV).contiguous() if (case.rot_4d or n == "means3D") else None for n in fo.NAMES]


def c_forward(case, cams, tensors, flows_ptr):
    from fdgs import _capi
    from fdgs.flow import _flow_in
    a, keep = _flow_in(cams[0], cams[1], tensors, case.rot_4d, case.dim, case.raw, case.mod)
    assert a.P == case.P and (a.viewmatrix_to is None) == (cams[1].world_view_transform is cams[0].world_view_transform)
    rc = _capi.lib.fdgs_gaussian_flow_forward(C.byref(a), flows_ptr, _capi.current_stream_handle(torch.device(DEV)))
    assert rc == 0, _capi.last_error()
    torch.cuda.synchronize()
    del keep


def c_backward(case, cams, tensors, dL, scale, out_ptrs):
    from fdgs import _capi
    from fdgs.flow import _flow_in
    a, keep = _flow_in(cams[0], cams[1], tensors, case.rot_4d, case.dim, case.raw, case.mod)
    out = _capi.FdgsFlowGrads(*out_ptrs)
    rc = _capi.lib.fdgs_gaussian_flow_backward(C.byref(a), dL.data_ptr(), float(scale), C.byref(out), _capi.current_stream_handle(dL.device))
    assert rc == 0, _capi.last_error()
    torch.cuda.synchronize()
    del keep


def run_forward(case, b, form=None):
    flows = torch.full((case.P, 2), float("nan"), device=DEV)
    c_forward(case, case_cameras(case, b, form), case_inputs(case, b), flows.data_ptr())
    return flows.cpu().numpy()


def zero_bufs(case):
    return [torch.zeros(case.P, SHAPES[n], device=DEV) for n in fo.NAMES]


def run_backward(case, b, form=None, bufs=None, which=None, tensors=None):
    """{name: array} of the buffers after one call at scale SCALE (``which``: the outputs that are not NULL; default all six)."""
    bufs = zero_bufs(case) if bufs is None else bufs
    ptrs = [t.data_ptr() if (which is None or n in which) else None for n, t in zip(fo.NAMES, bufs)]
    c_backward(case, case_cameras(case, b, form), case_inputs(case, b) if tensors is None else tensors, b["dL"].to(DEV).contiguous(), fc.SCALE, ptrs)
    return {n: t.cpu().numpy() for n, t in zip(fo.NAMES, bufs)}


def hold(case, got, f64, sens, names, worst_ratios):
    for k in names:
        r = co.ratio(got[k], f64[k], sens[k])
        w = float(r.max())
        fam = worst_ratios.setdefault(case.family, {})
        fam[k] = max(fam.get(k, 0.0), w)
        print("%s %-11s worst ratio %.4g (K %g)" % (case.name, k, w, fc.K[case.family][k]))
        assert w <= fc.K[case.family][k], "%s %s: element %s is %.4g bars from float64 (K = %g)" % (
            case.name, k, np.unravel_index(int(r.argmax()), r.shape), w, fc.K[case.family][k])


@pytest.mark.parametrize("name", CASE_NAMES)
def test_forward_elements_against_float64(gpu_device, worst_ratios, name):
    """``flows`` within K of the bar on every element; the validity mask is the oracle's; invalid rows are the bits of 0; two runs
    give equal bits; one camera as equal matrices in buffers of their own gives the NULL form's bits."""
    case = fc.BY_NAME[name]
    b = fc.build(case)
    f64, sens = fc.oracle(case)
    got = run_forward(case, b)
    assert np.isfinite(got).all()
    assert not fc.bits(got[~f64["ok"]]).any(), "a Gaussian behind a camera has a flow that is not the bits of 0"
    mask = fc.bits(got).any(axis=1)
    assert np.array_equal(mask, f64["ok"] & (f64["flows"] != 0).any(axis=1)), "the validity mask is not the oracle's"
    hold(case, {"flows": got}, f64, sens, ("flows",), worst_ratios)
    assert np.array_equal(fc.bits(got), fc.bits(run_forward(case, b))), "two runs differ"
    if case.cams == "equal":
        assert np.array_equal(fc.bits(got), fc.bits(run_forward(case, b, "null"))), "equal matrices and NULL matrices differ"
    pops = fc.assert_populations(case, f64, got)
    print(name, {k: v for k, v in pops.items() if v})


@pytest.mark.parametrize("name", CASE_NAMES)
def test_backward_elements_against_float64(gpu_device, worst_ratios, name):
    """fdgs_gaussian_flow_backward itself, scale 0.37, the case's dL_dflows, zeroed buffers: all six gradients within K of the bar on
    every element (without rot_4d the five others stay 0); two runs give equal bits; equal matrices give the NULL form's bits."""
    case = fc.BY_NAME[name]
    b = fc.build(case)
    f64, sens = fc.oracle(case)
    got = run_backward(case, b)
    hold(case, got, f64, sens, fo.NAMES, worst_ratios)
    again = run_backward(case, b)
    other = run_backward(case, b, "null") if case.cams == "equal" else again
    for n in fo.NAMES:
        assert np.array_equal(fc.bits(got[n]), fc.bits(again[n])), "%s: two runs differ" % n
        assert np.array_equal(fc.bits(got[n]), fc.bits(other[n])), "%s: equal matrices and NULL matrices differ" % n
        if not case.rot_4d and n != "means3D":
            assert not fc.bits(got[n]).any(), n


def prefilled(case, seed):
    """Six buffers of a non-zero pattern (no element 0, magnitudes 0.25 .. 4)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in fo.NAMES:
        v = torch.exp2(4.0 * torch.rand(case.P, SHAPES[n], generator=g) - 2.0) * torch.where(torch.rand(case.P, SHAPES[n], generator=g) < 0.5, -1.0, 1.0)
        out.append(v.to(DEV).contiguous())
    return out


@pytest.mark.parametrize("name", ("hard_raw_p257", "hard_act_p1000"))
def test_backward_adds_and_leaves_culled_rows_alone(gpu_device, name):
    """Buffers that already hold values: the rows of Gaussians behind either camera keep their bits in all six; the others are
    prefill + gradient within the gradient's bar plus one float32 addition's rounding (one ulp32 of the larger addend)."""
    case = fc.BY_NAME[name]
    b = fc.build(case)
    f64, sens = fc.oracle(case)
    bufs = prefilled(case, 3)
    before = {n: t.cpu().numpy() for n, t in zip(fo.NAMES, bufs)}
    got = run_backward(case, b, bufs=bufs)
    culled = ~f64["ok"]
    assert culled.sum() >= 12
    for n in fo.NAMES:
        pf = before[n].astype(np.float64)
        assert np.array_equal(fc.bits(got[n][culled]), fc.bits(before[n][culled])), "%s: a culled Gaussian's row was written" % n
        grad = f64[n].reshape(pf.shape)
        bar = fc.K[case.family][n] * co.core_bar(grad, sens[n].reshape(pf.shape)) + co.ulp32(np.maximum(np.abs(pf), np.abs(grad)))
        err = np.abs(got[n].astype(np.float64) - (pf + grad))
        assert (err <= bar).all(), "%s: element %s is %.3g bars from prefill + gradient" % (
            n, np.unravel_index(int((err / bar).argmax()), err.shape), float((err / bar).max()))


@pytest.mark.parametrize("name", ("plain4d_p257", "plain3d_p65"))
def test_backward_without_rot_4d_writes_the_means_only(gpu_device, name):
    """Without rot_4d: NULL for ts / scales / scales_t / rotations / rotations_r is accepted, the five buffers that are not the mean's
    keep every bit of a non-zero prefill, and the mean's is prefill + gradient."""
    case = fc.BY_NAME[name]
    b = fc.build(case)
    f64, sens = fc.oracle(case)
    bufs = prefilled(case, 4)
    before = {n: t.cpu().numpy() for n, t in zip(fo.NAMES, bufs)}
    tensors = case_inputs(case, b)
    assert all(t is None for t in tensors[1:])
    got = run_backward(case, b, bufs=bufs, tensors=tensors)
    for n in fo.NAMES[1:]:
        assert np.array_equal(fc.bits(got[n]), fc.bits(before[n])), "%s was written without rot_4d" % n
    pf, grad = before["means3D"].astype(np.float64), f64["means3D"]
    bar = fc.K[case.family]["means3D"] * co.core_bar(grad, sens["means3D"]) + co.ulp32(np.maximum(np.abs(pf), np.abs(grad)))
    assert (np.abs(got["means3D"].astype(np.float64) - (pf + grad)) <= bar).all() and f64["ok"].all()


SUBSETS = (("ts",), ("rotations_r",), ("means3D",), ("scales", "scales_t", "rotations", "rotations_r"))


@pytest.mark.parametrize("name", ("raw_p257_two_mod1", "hard_act_p257"))
def test_output_subsets_have_the_full_calls_bits(gpu_device, name):
    """NULL outputs: d_ts only (the return before the covariance chain), d_rotations_r only, d_means3D only, the four covariance
    outputs without d_means3D: what is written has the full call's bits, what is NULL is not touched (the buffers stay 0)."""
    case = fc.BY_NAME[name]
    b = fc.build(case)
    full = run_backward(case, b)
    for which in SUBSETS:
        got = run_backward(case, b, which=which)
        for n in fo.NAMES:
            if n in which:
                assert full[n].any() and np.array_equal(fc.bits(got[n]), fc.bits(full[n])), "%s of the call with only %s" % (n, which)
            else:
                assert not fc.bits(got[n]).any(), "%s was written by the call with only %s" % (n, which)


@pytest.mark.parametrize("which", SUBSETS)
def test_autograd_asks_for_the_needed_gradients_only(gpu_device, monkeypatch, which):
    """Through autograd: an input that does not require grad gets None from the backward, the others the full call's bits."""
    from fdgs.flow import _GaussianFlow, gaussian_flow
    returned, inner = [], _GaussianFlow.backward

    def spy(ctx, dL_dflows):
        returned.append(inner(ctx, dL_dflows))
        return returned[-1]

    monkeypatch.setattr(_GaussianFlow, "backward", staticmethod(spy))
    case = fc.BY_NAME["raw_p257_two_mod1"]
    b = fc.build(case)
    cam, cam_to = case_cameras(case, b)
    dL = b["dL"].to(DEV)
    res = []
    for needed in (fo.NAMES, which):
        leaves = {n: b["par"][n].to(DEV).clone().requires_grad_(n in needed) for n in fo.NAMES}
        flows = gaussian_flow(cam, cam_to, *[leaves[n] for n in fo.NAMES], rot_4d=True, gaussian_dim=4, raw=case.raw, scaling_modifier=case.mod)
        flows.backward(dL)
        res.append(returned[-1][:6])
    assert len(returned) == 2
    full, part = res
    for n, f, p in zip(fo.NAMES, full, part):
        if n in which:
            assert torch.equal(p, f) and bool(f.any()), n
        else:
            assert p is None and f is not None, n


@pytest.mark.parametrize("name", ("raw_p63_two_mod0.7", "hard_raw_p257"))
def test_slices_one_float_past_a_16_byte_boundary(gpu_device, name):
    """All six inputs, dL_dflows, flows and all six outputs are slices of ONE flat buffer, each starting 4 bytes past a 16-byte
    boundary (a parameter bucket's layout at its worst): the same bits as the call on separately allocated tensors."""
    case = fc.BY_NAME[name]
    b = fc.build(case)
    P = case.P
    sizes = [("in_" + n, P * SHAPES[n]) for n in fo.NAMES] + [("dL", 2 * P), ("flows", 2 * P)] + [("out_" + n, P * SHAPES[n]) for n in fo.NAMES]
    starts, at = {}, 1
    for k, sz in sizes:
        starts[k] = at
        at = (at + sz + 3) // 4 * 4 + 1
    flat = torch.zeros(at + 4, device=DEV)
    assert flat.data_ptr() % 16 == 0
    view = {k: flat[starts[k]:starts[k] + sz] for k, sz in sizes}
    assert all(v.data_ptr() % 16 == 4 for v in view.values())
    for n in fo.NAMES:
        view["in_" + n].copy_(b["par"][n].to(DEV).reshape(-1))
    view["dL"].copy_(b["dL"].to(DEV).reshape(-1))
    tensors = [view["in_" + n].view(P, SHAPES[n]) for n in fo.NAMES]
    cams = case_cameras(case, b)
    c_forward(case, cams, tensors, view["flows"].data_ptr())
    c_backward(case, cams, tensors, view["dL"], fc.SCALE, [view["out_" + n].data_ptr() for n in fo.NAMES])
    assert np.array_equal(fc.bits(view["flows"].cpu().numpy().reshape(P, 2)), fc.bits(run_forward(case, b)))
    want = run_backward(case, b)
    for n in fo.NAMES:
        assert np.array_equal(fc.bits(view["out_" + n].cpu().numpy().reshape(want[n].shape)), fc.bits(want[n])), n
        assert torch.equal(view["in_" + n], b["par"][n].to(DEV).reshape(-1)), "%s: an input was written" % n
    used = torch.zeros(flat.numel(), dtype=torch.bool, device=DEV)
    for k, sz in sizes:
        used[starts[k]:starts[k] + sz] = True
    assert not bool(flat[~used].any()), "the padding between the slices was written"


@pytest.mark.parametrize("name", ("raw_p1_two_mod1", "raw_p63_two_mod0.7", "raw_p65_null_mod0.7", "raw_p257_two_mod1"))
def test_nothing_is_written_outside_the_rows(gpu_device, name):
    """``flows`` and the six gradient buffers between guard bands (tests/guarded.py): the forward writes every element of ``flows``
    over a NaN prefill, and neither kernel changes a guard element."""
    case = fc.BY_NAME[name]
    b = fc.build(case)
    P = case.P
    cams, tensors = case_cameras(case, b), case_inputs(case, b)
    flows = Guarded(2 * P, DEV)
    c_forward(case, cams, tensors, flows.ptr)
    got = flows.check("flows").cpu().numpy().reshape(P, 2)
    assert np.array_equal(fc.bits(got), fc.bits(run_forward(case, b)))
    outs = [Guarded(P * SHAPES[n], DEV) for n in fo.NAMES]
    for g in outs:
        g.body().zero_()
    c_backward(case, cams, tensors, b["dL"].to(DEV).contiguous(), fc.SCALE, [g.ptr for g in outs])
    want = run_backward(case, b)
    for n, g in zip(fo.NAMES, outs):
        body = g.check("d_" + n, all_written=False).cpu().numpy()
        assert np.array_equal(fc.bits(body.reshape(want[n].shape)), fc.bits(want[n])), n
