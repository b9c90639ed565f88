"""GPU: the feature blend and its adjoint (csrc/features.hip, fdgs_feature_blend / fdgs_feature_blend_backward, fdgs.features) against
the numpy restatement on the port oracle's forward (tests/feature_oracle.py, pinned to the oracle by tests/test_feature_oracle_host.py),
against the GPU forward itself, and against each other.

Against the oracle the oracle's ``border`` pixels (a decision within 1e-5 of the alpha = 1/255 or the T = 1e-4 cliff) are left out --
not compared in the forward, given a zero upstream gradient ON BOTH SIDES in the backward; nothing else is, and every case asserts
that they are at most 1 % of the pixels.  Bars: the forward within PIX_TOL * max(1, max |F|) per pixel; the backward within
GRAD_TOL * max(1, max |ref|) per tensor; against the forward's own 1 - T and in the adjoint identity nothing is excluded."""
import numpy as np
import pytest
import torch

from util import GRAD_TOL, PIX_TOL, native_args_fwd, scene_to_device, synth

import contribution_cases as cases
import feature_oracle as fo

pytestmark = pytest.mark.gpu

NAMES = ["a", "b", "c", "d", "opaque", "1x1", "8x8", "17x9"]
CULL = pytest.mark.parametrize("tile_cull", [False, True], ids=["reference-lists", "tile-cull"])


def _fwd(sc, **kw):
    from fdgs.gaussian_renderer.diff_gaussian_rasterization import _C
    return _C.rasterize_gaussians(*native_args_fwd(sc), **kw)


def _dims(scene):
    return int(scene["means3D"].shape[0]), int(scene["W"]), int(scene["H"])


def _blend(res, P, W, H, F, **kw):
    from fdgs import features
    return features.blend_pass(P, W, H, res[6], res[7], res[8], res[0], F, **kw)


def _blend_bwd(res, P, W, H, g, d):
    from fdgs import features
    return features.blend_backward_pass(P, W, H, res[6], res[7], res[8], res[0], g, d)


def _features(P, Cn, seed=0):
    """F ~ U(-1, 1), float32 [P,Cn]."""
    return (2.0 * np.random.default_rng(100 + seed).random((P, Cn)) - 1.0).astype(np.float32)


def _border(name, ref):
    excl = ref["border"].astype(bool)
    assert float(excl.mean()) <= 0.01, "%s: %g of the pixels are cliff pixels by the oracle" % (name, excl.mean())
    return excl


# ---- 1. the forward against the oracle ---------------------------------------------------------------------------------------------

@CULL
@pytest.mark.parametrize("name", NAMES)
def test_forward_against_the_oracle(name, tile_cull, gpu_device):
    scene, ref, wk, _ = cases.oracle(name)
    P, W, H = _dims(scene)
    excl = _border(name, ref)
    if name == "opaque":
        early = float(wk["ended_early"].mean())
        assert early >= 0.05, "the opaque scene ends only %g of its pixels early: the early-termination path is not tested" % early
    res = _fwd(scene_to_device(scene, gpu_device), tile_cull=tile_cull)
    for Cn in (1, 3, 16, 17, 37):   # one channel, a narrow group, a whole group, a group + a tail of one, several groups + a tail
        F = _features(P, Cn)
        want = fo.forward(wk, F)
        got = _blend(res, P, W, H, torch.from_numpy(F).to(gpu_device)).cpu().numpy()
        assert got.shape == (Cn, H, W) and got.dtype == np.float32
        bar = PIX_TOL * max(1.0, float(np.abs(F).max()))
        err = float(np.abs(got - want)[:, ~excl].max()) if (~excl).any() else 0.0
        print("%s/%s C=%d: forward err %.3g (bar %.3g), %d pixels excluded" % (name, "cull" if tile_cull else "ref", Cn, err, bar, int(excl.sum())))
        assert err <= bar, (name, Cn, err, bar)


# ---- 2. the forward against the forward itself, nothing excluded -------------------------------------------------------------------

@pytest.mark.parametrize("lists", ["compact", "lazy-sparse"])
@pytest.mark.parametrize("name", ["b", "opaque"])
def test_ones_give_the_forwards_own_alpha(name, lists, gpu_device):
    from fdgs import _capi
    scene = cases.make(name)
    P, W, H = _dims(scene)
    sc = scene_to_device(scene, gpu_device)
    if lists == "compact":
        res = _fwd(sc)
    else:
        _capi.forward_lazy_status(gpu_device, wait=True)
        first = _fwd(sc, tile_cull=True)          # the waiting forward leaves the run-ahead guess behind
        s0 = _capi.sparse_lists_stats()
        res = _fwd(sc, tile_cull=True, lazy=True, sparse_lists=True)
        assert res[0] == -1, "the second forward of a configuration must run ahead"
    got = _blend(res, P, W, H, torch.ones(P, device=gpu_device))   # a [P] vector is one channel
    if lists != "compact":
        pend, failed, reported = _capi.forward_lazy_status(gpu_device, wait=True)
        assert (pend, failed, reported) == (0, 0, [first[0]])
        assert _capi.sparse_lists_stats()[0] - s0[0] == 1
    torch.cuda.synchronize()
    alpha = 1.0 - res[4]
    assert got.shape == (1, H, W) and float(alpha.max()) > 0.5
    err = float((got - alpha).abs().max())
    print("%s/%s: blend(ones) - (1 - T) %.3g (bar %.1g)" % (name, lists, err, PIX_TOL))
    assert err <= PIX_TOL, err


# ---- 3. determinism, independence of the grouping ----------------------------------------------------------------------------------

def test_bit_identical_run_to_run_and_for_every_grouping(gpu_device):
    scene = cases.make("b")
    P, W, H = _dims(scene)
    res = _fwd(scene_to_device(scene, gpu_device), tile_cull=True)
    F = torch.from_numpy(_features(P, 37, seed=1)).to(gpu_device)
    a = _blend(res, P, W, H, F)
    b = _blend(res, P, W, H, F)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "two runs differ"
    assert float(a.abs().max()) > 0.1
    for j in (0, 15, 16, 36):
        one = _blend(res, P, W, H, F[:, j].contiguous())
        assert torch.equal(one[0].view(torch.int32), a[j].view(torch.int32)), "channel %d of 37 differs from the same column rendered alone" % j
    # ... and rendered with 16 others, and into a buffer of the caller's
    out = torch.full((16, H, W), 7.0, device=gpu_device)
    assert _blend(res, P, W, H, F[:, 16:32].contiguous(), out=out) is out
    assert torch.equal(out.view(torch.int32), a[16:32].view(torch.int32))


# ---- 4. the backward against the oracle --------------------------------------------------------------------------------------------

@CULL
@pytest.mark.parametrize("name", NAMES)
def test_backward_against_the_oracle(name, tile_cull, gpu_device):
    scene, ref, wk, _ = cases.oracle(name)
    P, W, H = _dims(scene)
    excl = _border(name, ref)
    res = _fwd(scene_to_device(scene, gpu_device), tile_cull=tile_cull)
    # Gaussians without a contribution by the oracle (on an excluded pixel the GPU may decide otherwise: there the gradient is zero)
    touched = np.zeros(P, bool)
    touched[wk["gid"]] = True
    for Cn in (1, 16, 17):
        g = np.random.default_rng(200 + Cn).standard_normal((Cn, H, W)).astype(np.float32)
        g[:, excl] = 0.0
        want = fo.backward(wk, g, P)
        gd = torch.from_numpy(g).to(gpu_device)
        d = torch.zeros((P, Cn), device=gpu_device)
        assert _blend_bwd(res, P, W, H, gd, d) is d
        got = d.cpu().numpy()
        bar = GRAD_TOL * max(1.0, float(np.abs(want).max()))
        err = float(np.abs(got - want).max())
        print("%s/%s C=%d: backward err %.3g (bar %.3g)" % (name, "cull" if tile_cull else "ref", Cn, err, bar))
        assert err <= bar, (name, Cn, err, bar)
        # rows of Gaussians with no contribution are exactly zero (one that only the GPU takes, on a cliff pixel, gets w * 0)
        assert not got[~touched].any(), "a Gaussian without a contribution received a gradient"
        # a second call into the same buffer doubles it
        _blend_bwd(res, P, W, H, gd, d)
        err2 = float(np.abs(d.cpu().numpy() - 2.0 * want).max())
        assert err2 <= 2.0 * bar, (name, Cn, err2)
        # a pre-filled buffer is added to, not overwritten
        d.fill_(3.0)
        _blend_bwd(res, P, W, H, gd, d)
        err3 = float(np.abs(d.cpu().numpy() - 3.0 - want).max())
        assert err3 <= bar, (name, Cn, err3)


# ---- 5. the adjoint identity, no oracle, nothing excluded --------------------------------------------------------------------------

@pytest.mark.parametrize("name,Cn", [("b", 17), ("8x8", 1)])
def test_adjoint_identity(name, Cn, gpu_device):
    scene = cases.make(name)
    P, W, H = _dims(scene)
    res = _fwd(scene_to_device(scene, gpu_device), tile_cull=True)
    rng = np.random.default_rng(9)
    F = torch.from_numpy(_features(P, Cn, seed=2)).to(gpu_device)
    G = torch.from_numpy(rng.standard_normal((Cn, H, W)).astype(np.float32)).to(gpu_device)
    out = _blend(res, P, W, H, F)
    d = _blend_bwd(res, P, W, H, G, torch.zeros((P, Cn), device=gpu_device))
    lhs = float((out.double() * G.double()).sum())
    rhs = float((F.double() * d.double()).sum())
    bar = GRAD_TOL * float((out.double().abs() * G.double().abs()).sum())
    print("%s C=%d: <blend(F), G> %.9g  <F, blend_backward(G)> %.9g  difference %.3g (bar %.3g)" % (name, Cn, lhs, rhs, abs(lhs - rhs), bar))
    assert bar > 0.0 and abs(lhs - rhs) <= bar


# ---- 6. render_features ------------------------------------------------------------------------------------------------------------

class _Model:
    """A model that has only the reference's post-activation getters (the duck type render() reads), holding a scene's tensors as
    leaves that could take a gradient."""

    def __init__(self, scene, dev):
        t = {k: scene[k].to(dev).clone().requires_grad_(True) for k in ("means3D", "opacities", "scales", "rotations", "scales_t", "ts", "rotations_r", "shs")}
        self.leaves = t
        self.get_xyz, self.get_opacity, self.get_scaling, self.get_rotation = t["means3D"], t["opacities"], t["scales"], t["rotations"]
        self.get_scaling_t, self.get_t, self.get_rotation_r, self.get_features = t["scales_t"], t["ts"], t["rotations_r"], t["shs"]
        self.active_sh_degree, self.active_sh_degree_t = scene["sh_degree"], scene["sh_degree_t"]
        self.time_duration = [0.0, scene["time_duration"]]
        self.rot_4d, self.gaussian_dim, self.force_sh_3d = scene["rot_4d"], scene["gaussian_dim"], scene["force_sh_3d"]
        self.prefilter_var = -1.0
        self.env_map = None
        self.get_max_sh_channels = scene["M"]


def _camera(scene, dev, timestamp=None):
    from fdgs import train_host
    return train_host.SyntheticCamera(scene, dev, timestamp=timestamp)


def _pipe():
    from fdgs import train_host
    return train_host.PipelineFlags()


@pytest.mark.parametrize("style", ["getters", "raw"])
def test_render_features(style, gpu_device):
    from fdgs import features, fused, train_host
    from fdgs.gaussian_renderer import render
    scene = cases.make("a")
    P, W, H = _dims(scene)
    cam, pipe, bg = _camera(scene, gpu_device), _pipe(), scene["bg"].to(gpu_device)
    Cn = 5
    if style == "getters":
        model = _Model(scene, gpu_device)
        hand = _fwd(scene_to_device(scene, gpu_device))
        pkg = {k: v.detach() for k, v in render(cam, model, pipe, bg).items() if k in ("render", "alpha")}
    else:
        model = train_host.GaussianParams(scene, gpu_device)
        rs, (xyz, feats, opacity, ts, scaling, scaling_t, rotation, rotation_r, pv) = fused.raw_settings(cam, model, pipe, bg)
        with torch.no_grad():
            hand = fused.raw_forward(rs, xyz, feats, opacity, ts, scaling, scaling_t, rotation, rotation_r, pv)
            pkg = fused.render_raw(cam, model, pipe, bg)
        grad_before = model.flat_grad.clone()
    F = torch.from_numpy(_features(P, Cn, seed=3)).to(gpu_device).requires_grad_(True)
    out = features.render_features(cam, model, pipe, F, bg_color=bg)
    assert set(out) == {"features", "render", "alpha", "depth", "radii"}
    assert out["features"].shape == (Cn, H, W) and out["alpha"].shape == (1, H, W) and out["depth"].shape == (1, H, W) and out["radii"].shape == (P,)
    want = _blend(hand, P, W, H, F.detach())
    assert torch.equal(out["features"].detach().view(torch.int32), want.view(torch.int32)), "render_features differs from blend_pass on the same forward"
    e_a = float((out["alpha"] - pkg["alpha"]).abs().max())
    e_r = float((out["render"] - pkg["render"]).abs().max())
    print("%s: alpha err %.3g render err %.3g (bar %.1g)" % (style, e_a, e_r, PIX_TOL))
    assert e_a <= PIX_TOL and e_r <= PIX_TOL
    assert not any(out[k].requires_grad for k in ("render", "alpha", "depth", "radii")) and out["features"].requires_grad
    out["features"].sum().backward()
    ref = _blend_bwd(hand, P, W, H, torch.ones((Cn, H, W), device=gpu_device), torch.zeros((P, Cn), device=gpu_device))
    bar = GRAD_TOL * max(1.0, float(ref.abs().max()))
    e_g = float((F.grad - ref).abs().max())
    print("%s: features.grad err %.3g (bar %.3g)" % (style, e_g, bar))
    assert F.grad.shape == (P, Cn) and e_g <= bar
    if style == "getters":
        assert all(t.grad is None for t in model.leaves.values()), "the model's parameters received a gradient"
    else:
        # (this model's .grad tensors are views of its gradient bucket, bound at construction: the bucket is untouched)
        assert torch.equal(model.flat_grad, grad_before) and all(not p.grad.any() for p in model.params.values())
    # a [P] vector is one channel, default background, tile_cull: the same image
    one = features.render_features(cam, model, pipe, F.detach()[:, 2].contiguous(), tile_cull=True)
    assert one["features"].shape == (1, H, W) and torch.equal(one["features"][0], want[2])


# ---- 7. fit_features end to end ----------------------------------------------------------------------------------------------------

def test_fit_features_recovers_one_hot_labels(gpu_device):
    from fdgs import features
    k = 4
    views = [(pose, tf) for pose in ("rig0", "rig1", "rig3") for tf in (0.35, 0.65)]   # three rig poses x two timestamps
    scenes = [cases.make("a", pose, tf) for pose, tf in views]
    P, W, H = _dims(scenes[0])
    model, pipe = _Model(scenes[0], gpu_device), _pipe()
    cams = [_camera(s, gpu_device) for s in scenes]
    assert len({c.timestamp for c in cams}) == 2
    xyz = scenes[0]["means3D"]
    label = (xyz[:, 0] > xyz[:, 0].median()).long() + 2 * (xyz[:, 1] > xyz[:, 1].median()).long()   # four clusters by position
    truth = torch.nn.functional.one_hot(label, k).float().to(gpu_device)
    with torch.no_grad():
        rendered = [features.render_features(c, model, pipe, truth) for c in cams]
    targets = [r["features"] for r in rendered]
    steps = []
    # a noiseless, exactly realisable target: 120 Adam steps at the default lr take the CPU restatement of this problem (the oracle's
    # weights as a sparse matrix) to 0.1 % of the initial loss
    fitted, history = features.fit_features(model, cams, targets, pipe, iterations=120, on_step=lambda it, v: steps.append(it))
    assert fitted.shape == (P, k) and not fitted.requires_grad and len(history) == 120 and steps == list(range(120))
    with torch.no_grad():
        final = [features.render_features(c, model, pipe, fitted)["features"] for c in cams]
    loss0 = float(torch.stack([(t ** 2).mean() for t in targets]).mean())             # the loss at the start value, zeros
    loss1 = float(torch.stack([((f - t) ** 2).mean() for f, t in zip(final, targets)]).mean())
    seen = [r["alpha"][0] > 0.5 for r in rendered]
    hit = sum(int((f.argmax(0)[m] == t.argmax(0)[m]).sum()) for f, t, m in zip(final, targets, seen))
    n = sum(int(m.sum()) for m in seen)
    print("fit_features: loss %.3g -> %.3g (%.2f %%), argmax accuracy %.4f on %d pixels" % (loss0, loss1, 100.0 * loss1 / loss0, hit / n, n))
    assert abs(history[0] - float((targets[0] ** 2).mean())) <= 1e-6 and n > 1000
    assert loss1 < 0.05 * loss0
    assert hit / n >= 0.95
    assert all(t.grad is None for t in model.leaves.values())
    # the other losses run, from a start value, and leave it alone
    start = fitted.clone()
    for kind in ("l1", "cosine"):
        f2, h2 = features.fit_features(model, cams[:2], targets[:2], pipe, iterations=2, loss=kind, features=start, lr=1e-3)
        assert f2.shape == (P, k) and len(h2) == 2 and all(np.isfinite(h2)) and torch.equal(start, fitted)
        # better than the zero start value: mean |target| for l1, 1 for cosine
        assert h2[0] < (float(targets[0].abs().mean()) if kind == "l1" else 1.0), (kind, h2)


# ---- 8. P == 0 and an empty forward ------------------------------------------------------------------------------------------------

def test_empty_model_and_a_camera_that_sees_nothing(gpu_device):
    from fdgs import _capi
    scene = cases.make("a")
    W, H = int(scene["W"]), int(scene["H"])
    empty = dict(scene)
    for key in synth.PER_GAUSSIAN_KEYS:
        empty[key] = scene[key][:0].contiguous()
    res = _fwd(scene_to_device(empty, gpu_device))
    out = torch.full((3, H, W), 5.0, device=gpu_device)
    _blend(res, 0, W, H, torch.zeros((0, 3), device=gpu_device), out=out)
    assert not out.any()
    d = torch.zeros((0, 3), device=gpu_device)
    assert _blend_bwd(res, 0, W, H, torch.ones((3, H, W), device=gpu_device), d) is d
    # everything far behind the camera: num_rendered = 0 (nothing is launched), then -1 (the passes walk empty lists)
    scene["means3D"] = scene["means3D"].clone()
    scene["means3D"][:, 2] -= 100.0
    P = int(scene["means3D"].shape[0])
    _capi.forward_lazy_status(gpu_device, wait=True)
    for lazy in (False, True):
        res = _fwd(scene_to_device(scene, gpu_device), lazy=lazy)
        assert res[0] in (0, -1)
        out = torch.full((17, H, W), 5.0, device=gpu_device)
        _blend(res, P, W, H, torch.ones((P, 17), device=gpu_device), out=out)
        assert not out.any()
        d = torch.full((P, 17), 2.0, device=gpu_device)
        _blend_bwd(res, P, W, H, torch.ones((17, H, W), device=gpu_device), d)
        assert bool((d == 2.0).all())
    _capi.forward_lazy_status(gpu_device, wait=True)
