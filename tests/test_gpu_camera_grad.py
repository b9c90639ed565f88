"""GPU: the camera gradients (fdgs_camera_backward, csrc/camera_bwd.hip) -- dL/d(viewmatrix, projmatrix, campos, timestamp) against the
float64 autograd of the oracle's forward (tests/camera_oracle.py), the reduction's shapes and bitwise reproducibility, the untouched
per-Gaussian gradients, the autograd path through ``render()`` with a ``fdgs.camera.LearnableCamera``, and a pose / time recovery.

Bar: the project's 1e-4 * max(1, max|ref|) per tensor; where float32 arithmetic of the same formulas cannot meet it (long cancelling
sums over P), 4 x the float32 oracle's own error on the same input (camera_oracle.bars; DESIGN.md section 4.7 has the measured ratios).
Upstream gradients are zeroed on the pixels the C oracle flags as sitting on a discrete threshold (alpha = 1/255, T = 1e-4), where two
correct forwards may take different branches: those decisions are held constant by definition of the derivative."""
import numpy as np
import pytest
import torch

import camera_oracle as co
from util import native_args_fwd, scene_to_device, synth

pytestmark = pytest.mark.gpu
SC = synth.SceneConfig
NAMES = ("viewmatrix", "projmatrix", "campos", "timestamp")

CFG = {
    "dim3_sh2": SC("t", 400, 64, 40, 2, 0, 0.06, 1.0, False, 3, False),
    "dim4_norot_sh1": SC("t", 400, 72, 56, 1, 0, 0.06, 4.0, False, 4, True),
    "rot4d_sh3t2": SC("t", 400, 64, 40, 3, 2, 0.06, 6.0, True, 4, False),
    "rot4d_force3d": SC("t", 400, 72, 56, 3, 0, 0.06, 6.0, True, 4, True),
}
# name: (config, W, H, pose, raw_params, prefilter_var, scale_modifier, colors_precomp)
CASES = {
    "dim3_sh2-rig0": ("dim3_sh2", 64, 40, "rig0", 0, -1.0, 1.0, False),
    "dim4_norot_sh1-rig2-raw": ("dim4_norot_sh1", 72, 56, "rig2", 1, -1.0, 1.0, False),
    "rot4d_sh3t2-slant": ("rot4d_sh3t2", 64, 40, "slant", 0, -1.0, 1.0, False),
    "rot4d_sh3t2-rig2-raw-prefilter": ("rot4d_sh3t2", 72, 56, "rig2", 1, 0.3, 1.0, False),
    "rot4d_force3d-rig0-mod07": ("rot4d_force3d", 72, 56, "rig0", 0, -1.0, 0.7, False),
    "rot4d_force3d-slant-raw": ("rot4d_force3d", 72, 56, "slant", 1, -1.0, 1.0, False),
    "precomp-rig2": ("rot4d_sh3t2", 72, 56, "rig2", 0, -1.0, 1.0, True),
}


def _masked_upstream(scene, lists, seed=2):
    up = synth.make_upstream_grads(scene["W"], scene["H"], seed=seed, scale=1e-2)
    keep = torch.from_numpy(~lists["border"].astype(bool)).float()
    return {k: v * keep for k, v in up.items()}


def _backward_args(sc, res, up, dev):
    (R, _c, _f, _d, _T, radii, geom, binb, img, _cov, out_means3D) = res
    e = torch.Tensor([])
    g = lambda k: sc[k] if sc.get(k) is not None else e  # noqa: E731
    return (sc["bg"], sc["means3D"], out_means3D, radii, g("colors_precomp"), g("flow_2d"), sc["opacities"], g("ts"), g("scales"),
            g("scales_t"), g("rotations"), g("rotations_r"), sc.get("scale_modifier", 1.0), g("cov3D_precomp"), sc.get("prefilter_var", -1.0),
            sc["world_view_transform"], sc["full_proj_transform"], sc["tanfovx"], sc["tanfovy"], up["grad_color"].to(dev),
            up["grad_depth"].to(dev), up["grad_alpha"].to(dev), None, g("shs"), sc["sh_degree"], sc["sh_degree_t"], sc["camera_center"],
            sc["timestamp"], sc["time_duration"], sc["rot_4d"], sc["gaussian_dim"], sc["force_sh_3d"], geom, R, binb, img, False)


def run_camera(scene, up, dev, raw=False, camera=None, grad_accum=None):
    """Forward + backward through the C ABI; ``camera``: the dict rasterize_gaussians_backward takes (None: the unsplit backward).
    Returns (per-Gaussian gradient tuple, camera gradients or None)."""
    from fdgs.gaussian_renderer.diff_gaussian_rasterization import _C
    sc = scene_to_device(co.to_raw(scene) if raw else scene, dev)
    sc["flow_2d"] = None
    res = _C.rasterize_gaussians(*native_args_fwd(sc), raw_params=bool(raw))
    grads = _C.rasterize_gaussians_backward(*_backward_args(sc, res, up, dev), raw_params=bool(raw), camera=camera, grad_accum=grad_accum)
    torch.cuda.synchronize()
    return grads, (None if camera is None else camera["grads"])


def check_against_oracle(scene, dev, raw=False, label=""):
    lists = co.oracle_lists(scene)
    up = _masked_upstream(scene, lists)
    ref, _ = co.camera_reference(scene, up, lists)
    bars = co.bars(scene, up, lists, ref)
    _, got = run_camera(scene, up, dev, raw=raw, camera={})
    rep = {}
    for k in NAMES:
        g = got[k].double().cpu().numpy().reshape(ref[k].shape)
        assert np.isfinite(g).all(), (label, k)
        err = float(np.abs(g - ref[k]).max())
        bar, plain, e32 = bars[k]
        rep[k] = "%.2e (bar %.2e%s; max|ref| %.2e)" % (err, bar, "" if bar == plain else " = 4 x float32 oracle %.2e, plain %.2e" % (e32, plain),
                                                          float(np.abs(ref[k]).max()))
    print(label, "visible %d" % int((lists["radii"] > 0).sum()), rep)
    for k in NAMES:
        g = got[k].double().cpu().numpy().reshape(ref[k].shape)
        assert float(np.abs(g - ref[k]).max()) <= bars[k][0], "%s: dL_d%s %s" % (label, k, rep[k])
    # the structurally zero entries: exactly 0.0
    assert not got["viewmatrix"].reshape(-1)[co.ZERO_VIEW].cpu().numpy().any(), label
    assert not got["projmatrix"].reshape(-1)[co.ZERO_PROJ].cpu().numpy().any(), label
    return got, ref, lists


@pytest.mark.parametrize("name", list(CASES))
def test_camera_gradients_against_the_float64_oracle(name, gpu_device):
    cfgname, W, H, pose, raw, pv, mod, precomp = CASES[name]
    cfg = CFG[cfgname]._replace(W=W, H=H)
    scene = co.build_scene(cfg, pose, seed=5, colors_precomp=precomp, scale_modifier=mod, prefilter_var=pv)
    got, ref, lists = check_against_oracle(scene, gpu_device, raw=bool(raw), label=name)
    assert int((lists["radii"] > 0).sum()) >= 40, name
    assert np.abs(ref["viewmatrix"]).max() > 1e-3 and np.abs(ref["projmatrix"]).max() > 1e-3
    if precomp:
        assert not got["campos"].cpu().numpy().any()       # no SH: exactly zero
    else:
        assert np.abs(ref["campos"]).max() > 0
    if cfg.gaussian_dim == 3:
        assert not got["timestamp"].cpu().numpy().any()    # no time in the model: exactly zero
    else:
        assert abs(ref["timestamp"][0]) > 1e-4
    if pose == "rig2":
        assert np.abs(ref["projmatrix"][2, [0, 1, 3]]).max() > 1e-3   # the principal-point projection: row 2 of the stored matrix is live
    if pose == "slant":
        # the pose exists for the 1.3 tanfov clamp: some visible Gaussian sits beyond it
        V = scene["world_view_transform"].double()
        t = torch.cat([torch.from_numpy(lists["out_means3D"]).double(), torch.ones(scene["P"], 1, dtype=torch.float64)], 1) @ V
        vis = torch.from_numpy(lists["radii"] > 0)
        beyond = ((t[:, 0] / t[:, 2]).abs() > 1.3 * scene["tanfovx"]) | ((t[:, 1] / t[:, 2]).abs() > 1.3 * scene["tanfovy"])
        assert int((beyond & vis).sum()) > 0, "slant: no visible Gaussian beyond the clamp"


@pytest.mark.parametrize("P", [1, 63, 64, 65, 257, 700])
def test_reduction_shapes_against_the_oracle(P, gpu_device):
    """Fewer Gaussians than a wave, exactly one, one more, more than a block, three blocks."""
    cfg = CFG["rot4d_sh3t2"]._replace(s0=0.15 if P == 1 else 0.06)
    scene = co.build_scene(cfg, "rig0", seed=11, P=P)
    if P == 1:   # one Gaussian: in front of the camera, alive at the view's time
        scene["means3D"] = torch.tensor([[0.1, -0.05, 0.2]])
        scene["ts"] = torch.full((1, 1), scene["timestamp"] + 0.3)
        scene["opacities"] = torch.full((1, 1), 0.8)
    _, _, lists = check_against_oracle(scene, gpu_device, label="P=%d" % P)
    assert int((lists["radii"] > 0).sum()) >= 1


class Begun:
    """One view whose blend backward has run (``_C.backward_begin``): the accumulator records every later call reads.  The blend
    backward sums with float atomics, so two runs of IT differ in their last bits; everything that is compared bit for bit below
    therefore starts from the same records."""

    def __init__(self, scene, up, dev, raw=False):
        from fdgs.gaussian_renderer.diff_gaussian_rasterization import _C
        self.C = _C
        sc = scene_to_device(co.to_raw(scene) if raw else scene, dev)
        sc["flow_2d"] = None
        res = _C.rasterize_gaussians(*native_args_fwd(sc), raw_params=bool(raw))
        self.gacc = torch.zeros(scene["P"], 16, device=dev)
        self.stage = torch.empty(scene["P"], 8, device=dev)
        self.pending = _C.backward_begin(*_backward_args(sc, res, up, dev), raw_params=bool(raw), grad_accum=self.gacc, sh_stage=self.stage)
        self.keep = (sc, res)

    def camera(self, **kw):
        g = self.C.camera_backward(self.pending, **kw)
        torch.cuda.synchronize()
        return g

    def finish(self):
        """SH backward + geometry backward; the binding's 12-tuple (dL_dsh is deferred to the stage records: not compared)."""
        self.C.sh_backward_batch([self.pending])
        g = self.C.backward_finish(self.pending)
        torch.cuda.synchronize()
        return [t.clone() for i, t in enumerate(g) if i != 5] + [self.stage.clone()]


def test_nothing_visible_accumulate_scale_and_bitwise_reproducibility(gpu_device):
    dev = gpu_device
    scene = co.build_scene(CFG["rot4d_sh3t2"], "rig0", seed=5)
    lists = co.oracle_lists(scene)
    up = _masked_upstream(scene, lists)
    v = Begun(scene, up, dev)
    a, b = v.camera(), v.camera()
    for k in NAMES:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), "two runs differ in dL_d" + k
        assert a[k].abs().max() > 0
    # scale multiplies the result (one float multiplication of the same sum), accumulate adds to the previous contents
    s = v.camera(scale=0.25)
    prev = {k: torch.full_like(a[k], 3.0) for k in NAMES}
    out = {k: t.clone() for k, t in prev.items()}
    acc = v.camera(scale=0.25, out=out, accumulate=True)
    for k in NAMES:
        assert torch.equal(s[k], a[k] * 0.25), k
        assert acc[k] is out[k] and torch.equal(out[k], prev[k] + s[k]), k
    # only some outputs wanted: the others are not computed, the wanted ones unchanged
    part = v.camera(want=(False, True, False, True))
    assert part["viewmatrix"] is None and part["campos"] is None
    assert torch.equal(part["projmatrix"], a["projmatrix"]) and torch.equal(part["timestamp"], a["timestamp"])
    v.finish()
    # every Gaussian behind the camera: all zeros; with accumulate the arrays keep their contents
    behind = dict(scene)
    behind["means3D"] = scene["means3D"] + torch.tensor([0.0, 0.0, -40.0])
    assert int((co.oracle_lists(behind)["radii"] > 0).sum()) == 0
    w = Begun(behind, up, dev)
    z = w.camera()
    out = {k: t.clone() for k, t in prev.items()}
    w.camera(out=out, accumulate=True)
    for k in NAMES:
        assert not z[k].cpu().numpy().any(), k
        assert torch.equal(out[k], prev[k]), k


@pytest.mark.parametrize("raw", [0, 1])
def test_per_gaussian_gradients_are_not_disturbed(raw, gpu_device):
    """From the same accumulator records: SH + geometry backward without the camera call, and with it in between -- every
    per-Gaussian gradient bit for bit; the camera call leaves the records as they are, and with grad_accum_clean = 1 (the persistent
    buffer of backward_begin) the buffer is all zero after the geometry backward either way.  The split backward of
    rasterize_gaussians_backward(camera=...) (its own accumulator, grad_accum_clean = 0) gives the same gradients up to the blend
    backward's atomics."""
    dev = gpu_device
    scene = co.build_scene(CFG["rot4d_sh3t2"], "slant", seed=7)
    up = _masked_upstream(scene, co.oracle_lists(scene))
    v = Begun(scene, up, dev, raw=bool(raw))
    torch.cuda.synchronize()
    records = v.gacc.clone()
    assert records.abs().max() > 0
    plain = v.finish()
    assert not v.gacc.cpu().numpy().any()
    v.gacc.copy_(records)
    cam = v.camera()
    assert torch.equal(v.gacc.view(torch.int32), records.view(torch.int32)), "the camera call wrote to grad_accum"
    with_camera = v.finish()
    assert not v.gacc.cpu().numpy().any()
    assert cam["viewmatrix"].abs().max() > 0
    for i, (p, c) in enumerate(zip(plain, with_camera)):
        assert torch.equal(p.view(torch.int32), c.view(torch.int32)), "per-Gaussian gradient %d differs" % i
        assert p.abs().max() > 0 or i == 5, i   # (dL_dflows: no flow gradient was given)
    # the one-call form: same gradients (up to the order of the blend backward's atomic sums), same camera gradients
    unsplit, _ = run_camera(scene, up, dev, raw=bool(raw))
    split, cam2 = run_camera(scene, up, dev, raw=bool(raw), camera={})
    for i, (p, q) in enumerate(zip(unsplit, split)):
        assert float((p - q).abs().max()) <= 1e-5 * max(1.0, float(p.abs().max())), i
    for k in NAMES:
        assert float((cam[k] - cam2[k]).abs().max()) <= 1e-5 * max(1.0, float(cam[k].abs().max())), k


# ---- the autograd path: render() with a LearnableCamera ----

def _model_camera(scene, dev):
    import __graft_entry__ as ge
    pc = ge._SmokeModel(scene, dev)
    pc.prefilter_var = scene.get("prefilter_var", -1.0)
    return pc, ge._SmokeCamera(scene, dev), ge._SmokePipe()


def _loss(pkg, up, dev):
    return ((pkg["render"] * up["grad_color"].to(dev)).sum() + (pkg["depth"] * up["grad_depth"].to(dev)).sum()
            + (pkg["alpha"] * up["grad_alpha"].to(dev)).sum())


def test_render_with_a_learnable_camera_matches_the_chained_oracle(gpu_device):
    from fdgs import _capi
    from fdgs.camera import LearnableCamera
    from fdgs.gaussian_renderer import render
    dev = gpu_device
    scene = co.build_scene(CFG["rot4d_sh3t2"], "rig2", seed=9)
    pc, base, pipe = _model_camera(scene, dev)
    bg = scene["bg"].to(dev)
    xi = torch.tensor([0.01, -0.006, 0.004, 0.02, -0.015, 0.01])
    cam = LearnableCamera(base)
    with torch.no_grad():
        cam.pose_delta.copy_(xi.to(dev))
        cam.time_offset.fill_(0.07)
    # the oracle at the camera the kernels saw: the float32 tensors the module produced
    at = dict(scene, world_view_transform=cam.world_view_transform.detach().cpu(), full_proj_transform=cam.full_proj_transform.detach().cpu(),
              camera_center=cam.camera_center.detach().cpu(), timestamp=float(cam.timestamp.detach()))
    lists = co.oracle_lists(at)
    up = _masked_upstream(at, lists)
    _capi.profile_reset()
    _capi.profile_enable(True)
    try:
        _loss(render(cam, pc, pipe, bg), up, dev).backward()
        torch.cuda.synchronize()
        assert _capi.profile_read()["camera_bwd"][1] == 1
    finally:
        _capi.profile_enable(False)
    ref64, _ = co.camera_reference(at, up, lists)
    ref32, _ = co.camera_reference(at, up, lists, dtype=torch.float32)

    def chained(ref):
        """the oracle's camera gradients through the module's own expressions, in float64 on the CPU"""
        import types
        b64 = types.SimpleNamespace(world_view_transform=scene["world_view_transform"].double(), full_proj_transform=scene["full_proj_transform"].double(),
                                    camera_center=scene["camera_center"].double(), timestamp=scene["timestamp"])
        c = LearnableCamera(b64)
        with torch.no_grad():
            c.pose_delta.copy_(xi.double())
            c.time_offset.fill_(0.07)
        t = lambda k: torch.from_numpy(np.asarray(ref[k], np.float64))   # noqa: E731
        ((c.world_view_transform * t("viewmatrix")).sum() + (c.full_proj_transform * t("projmatrix")).sum()
         + (c.camera_center * t("campos")).sum() + c.timestamp * t("timestamp")[0]).backward()
        return c.pose_delta.grad.numpy(), c.time_offset.grad.numpy()
    want, want32 = chained(ref64), chained(ref32)
    got = (cam.pose_delta.grad.double().cpu().numpy(), cam.time_offset.grad.double().cpu().numpy())
    for name, g, w, w32 in zip(("pose_delta", "time_offset"), got, want, want32):
        plain = 1e-4 * max(1.0, float(np.abs(w).max()))
        bar = max(plain, 4.0 * float(np.abs(w32 - w).max()))
        err = float(np.abs(g - w).max())
        print("render(LearnableCamera): d%s err %.2e bar %.2e (plain %.2e) max|ref| %.2e" % (name, err, bar, plain, float(np.abs(w).max())))
        assert err <= bar and np.abs(w).max() > 1e-3, name
    assert pc.get_xyz.grad is not None and torch.isfinite(pc.get_xyz.grad).all()


def test_without_requires_grad_nothing_changes_and_no_camera_launch(gpu_device):
    from fdgs import _capi
    from fdgs.camera import LearnableCamera
    from fdgs.gaussian_renderer import render
    dev = gpu_device
    scene = co.build_scene(CFG["rot4d_sh3t2"], "rig2", seed=9)
    up = synth.make_upstream_grads(scene["W"], scene["H"], seed=2, scale=1e-2)
    results, stages = [], []
    for kind in ("plain", "frozen", "learnable"):
        pc, base, pipe = _model_camera(scene, dev)
        cam = base
        if kind != "plain":
            cam = LearnableCamera(base)   # zero delta: the base camera's tensors bit for bit
            if kind == "frozen":
                cam.requires_grad_(False)
        _capi.profile_reset()
        _capi.profile_enable(True)
        try:
            pkg = render(cam, pc, pipe, scene["bg"].to(dev))
            _loss(pkg, up, dev).backward()
            torch.cuda.synchronize()
            prof = _capi.profile_read()
        finally:
            _capi.profile_enable(False)
        stages.append({k: n for k, (_ms, n) in prof.items() if n})
        results.append([pkg[k].detach() for k in ("render", "depth", "alpha", "radii")]
                       + [getattr(pc, g).grad for g in ("get_xyz", "get_opacity", "get_scaling", "get_rotation", "get_scaling_t", "get_t",
                                                        "get_rotation_r", "get_features")] + [pkg["viewspace_points"].grad])
    assert "camera_bwd" not in stages[0] and stages[1] == stages[0], stages          # same stage list, no camera launch
    assert stages[2] == dict(stages[0], camera_bwd=1), stages
    for other in (results[1], results[2]):
        for i, (a, b) in enumerate(zip(results[0], other)):
            assert a.abs().max() > 0, i
            if i < 4:
                assert torch.equal(a, b), i   # the forward's outputs: bit for bit
            else:
                # the Gaussian gradients: the same launches on the same inputs.  Two runs of the blend backward differ in the last
                # bits of its float atomic sums (also plain against plain), so "the same" is 1e-5 of the tensor's scale here -- two
                # orders above what reordering sums of a few thousand fp32 terms can do, an order below the project's bar
                assert float((a - b).abs().max()) <= 1e-5 * max(1.0, float(a.abs().max())), i


def test_pose_and_time_offset_recovery(gpu_device):
    """Frozen Gaussians, targets from the true cameras; one camera perturbed by a twist of ~0.01 rad / 0.02 units and 0.02 x duration
    in time, refined by 60 Adam steps on the fused L1 + SSIM loss: pose error, time error and loss all end below where they started
    (the ratios are printed; DESIGN.md section 4.7 records them)."""
    from fdgs.camera import LearnableCamera
    from fdgs.gaussian_renderer import render
    from fdgs.loss import fused_l1_ssim
    dev = gpu_device
    cfg = SC("t", 600, 96, 64, 3, 1, 0.07, 6.0, True, 4, False)
    scene = co.build_scene(cfg, "rig0", seed=21)
    pc, base, pipe = _model_camera(scene, dev)
    for t in pc._t.values():
        t.requires_grad_(False)
    bg = scene["bg"].to(dev)
    with torch.no_grad():
        gt = render(base, pc, pipe, bg)["render"].clone()
    cam = LearnableCamera(base)
    with torch.no_grad():
        cam.pose_delta.copy_(torch.tensor([0.006, -0.006, 0.005, 0.012, -0.012, 0.011], device=dev))   # |omega| 0.0098, |u| 0.0202
        cam.time_offset.fill_(0.02 * cfg.duration)
    opt = torch.optim.Adam([{"params": [cam.pose_delta], "lr": 5e-4}, {"params": [cam.time_offset], "lr": 4e-3}])
    pose0, time0 = float(cam.pose_delta.detach().norm()), float(cam.time_offset.detach().abs())
    loss0 = None
    for _ in range(60):
        opt.zero_grad(set_to_none=True)
        loss = fused_l1_ssim(render(cam, pc, pipe, bg)["render"], gt)
        loss.backward()
        loss0 = float(loss.detach()) if loss0 is None else loss0
        opt.step()
    with torch.no_grad():
        loss1 = float(fused_l1_ssim(render(cam, pc, pipe, bg)["render"], gt))
    pose1, time1 = float(cam.pose_delta.detach().norm()), float(cam.time_offset.detach().abs())
    print("recovery: pose error %.4f -> %.4f (x %.3f), time error %.4f -> %.4f (x %.3f), loss %.5f -> %.5f (x %.3f)" % (
        pose0, pose1, pose1 / pose0, time0, time1, time1 / time0, loss0, loss1, loss1 / loss0))
    assert pose1 < pose0 and time1 < time0 and loss1 < loss0
