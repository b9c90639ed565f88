"""GPU: fdgs.depth (csrc/depth_loss.hip) -- the Pearson and scale-shift-invariant depth losses, the normals from depth and their
gradients against the float64 statement tests/depth_oracle.py.

The bars are those of tests/test_gpu_loss_edges.py (tests/loss_cases.py: MARGIN, VALUE_FLOOR): 4 x the float32 statement's own error
on the input, floored by the same figure on the ``smooth`` input of the same shape (and 2e-6 for a value); a bar never looks at a
kernel's output, every comparison is a maximum over all elements, and the worst ratio error / bar of a run is printed."""
import ctypes as C
import functools

import pytest
import torch

import depth_oracle as do
from guarded import Guarded as _Guarded
from loss_cases import MARGIN, VALUE_FLOOR

pytestmark = pytest.mark.gpu

UP = 0.37                      # upstream scalar: not 1; gradients and their bars scale by it
SHAPES = [(1, 1), (1, 2), (1, 7), (7, 1), (2, 2), (15, 16), (16, 16), (17, 19), (33, 31), (65, 130)]
BIG = (515, 513)               # 264195 pixels = 259 workgroups: more partials than one 256-wide trip of the finish loop
WORST = {}


def _ratio(tag, err, bar):
    r = err / bar if bar > 0 else (0.0 if err == 0 else float("inf"))
    WORST[tag] = max(WORST.get(tag, 0.0), r)
    return r


def _grads(fn, x, dtype):
    """(value, aux, d/d depth, d/d alpha) of the oracle function ``fn(depth, alpha) -> (scalar, aux)`` in ``dtype``, as float64."""
    d = x["depth"].detach().clone().to(dtype).requires_grad_(True)          # (a copy: the cached inputs stay plain tensors)
    a = None if x["alpha"] is None else x["alpha"].detach().clone().to(dtype).requires_grad_(True)
    val, aux = fn(d, a)
    val.backward()
    z = torch.zeros_like(d)
    return (float(val.detach()), aux, (d.grad if d.grad is not None else z).double(),
            None if a is None else (a.grad if a.grad is not None else z).double())


@functools.lru_cache(maxsize=None)
def loss_ref(kind, shape, mode):
    """Inputs, the float64 reference, the float32 statement's error and the bars of one case; computed once, shared, read-only."""
    x = do.make_inputs(kind, *shape)
    if shape == (1, 2):
        # a degenerate-n case: one of the two pixels is masked (n = 1).  With both valid rho is exactly +-1 and the ssi residual exactly
        # 0, where the gradient is 0 / a sign of 0 and the float32 statement's error -- the bar -- is 0 or 1e-15 by accident
        x["mask"] = torch.tensor([[[1.0, 0.0]]])
    fn = lambda dt: (lambda d, a: do.depth_loss(d, a, x["prior"], x["mask"], mode=mode, dtype=dt))   # noqa: E731
    v64, st64, gd64, ga64 = _grads(fn(torch.float64), x, torch.float64)
    v32, _, gd32, ga32 = _grads(fn(torch.float32), x, torch.float32)
    r = {"x": x, "value": v64, "stats": st64, "gd": gd64, "ga": ga64, "err_v": abs(v32 - v64),
         "err_gd": float((gd32 - gd64).abs().max()), "err_ga": 0.0 if ga64 is None else float((ga32 - ga64).abs().max())}
    floor = r if kind == "smooth" else loss_ref("smooth", shape, mode)
    r["bar_v"] = max(VALUE_FLOOR, MARGIN * max(r["err_v"], floor["err_v"]))
    r["bar_gd"] = MARGIN * max(r["err_gd"], floor["err_gd"])
    r["bar_ga"] = MARGIN * max(r["err_ga"], floor["err_ga"])
    _, ok = do.depth_z(x["depth"], x["alpha"], x["mask"], 0.5, torch.float64)
    r["ok"] = ok & do.prior_ok(x["prior"])
    return r


def _to(x, dev):
    return {k: (None if v is None else v.detach().to(dev)) for k, v in x.items()}


def _run_loss(x, mode, dev, up=UP):
    from fdgs import depth
    g = _to(x, dev)
    d = g["depth"].requires_grad_(True)
    a = None if g["alpha"] is None else g["alpha"].requires_grad_(True)
    loss, stats = depth.depth_loss(d, a, g["prior"], g["mask"], mode=mode, return_stats=True)
    (loss * up).backward()
    torch.cuda.synchronize()
    return float(loss.detach()), stats.cpu(), d.grad.cpu(), None if a is None else a.grad.cpu()


def _check_loss(kind, shape, mode, dev):
    r = loss_ref(kind, shape, mode)
    val, stats, gd, ga = _run_loss(r["x"], mode, dev)
    bad = ~r["ok"].view(-1)
    err_v = abs(val - r["value"])
    err_gd = float((gd.double() - UP * r["gd"]).abs().max())
    rv, rd = _ratio("value", err_v, r["bar_v"]), _ratio("d_depth", err_gd, UP * r["bar_gd"])
    line = "%-14s %-8s %-7s | value %.9g err %.2e (bar %.2e) | d_depth err %.2e (bar %.2e, ratio %.2f, ref32 %.2e)" % (
        kind, "%dx%d" % shape, mode, val, err_v, r["bar_v"], err_gd, UP * r["bar_gd"], rd, UP * r["err_gd"])
    assert torch.isfinite(gd).all() and val == val
    assert not gd.view(-1)[bad].view(torch.int32).any(), "d_depth is not +0 at an invalid pixel"
    assert rv <= 1.0, line
    assert rd <= 1.0, line
    if ga is not None:
        err_ga = float((ga.double() - UP * r["ga"]).abs().max())
        ra = _ratio("d_alpha", err_ga, UP * r["bar_ga"])
        line += " | d_alpha err %.2e (bar %.2e, ratio %.2f)" % (err_ga, UP * r["bar_ga"], ra)
        assert torch.isfinite(ga).all()
        assert not ga.view(-1)[bad].view(torch.int32).any(), "d_alpha is not +0 at an invalid pixel"
        assert ra <= 1.0, line
    print(line)
    n, s1, s2 = r["stats"]
    assert float(stats[0]) == n
    if n >= 2 and kind not in ("constant",):
        assert abs(float(stats[1]) - s1) <= 1e-5 * max(1.0, abs(s1)) and abs(float(stats[2]) - s2) <= 1e-5 * max(1.0, abs(s2))
    return r, val, gd, ga


# ---- 1. the losses: input classes and shapes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["pearson", "ssi"])
@pytest.mark.parametrize("shape", [(17, 19), (65, 130)], ids=["17x19", "65x130"])
@pytest.mark.parametrize("kind", do.KINDS)
def test_loss_input_classes_against_float64(kind, shape, mode, gpu_device):
    """Smooth depth plus noise; a prior that is an affine map of z (rho = 1, zero ssi residual); constant depth (degenerate
    variance); an all-invalid mask; alpha on both sides of alpha_min (and exactly at it, and 0); alpha=None; priors with 0, inf, nan
    and negative entries.  Value and both gradients at the bars, exact +0 at every invalid pixel, no NaN anywhere."""
    r, val, gd, ga = _check_loss(kind, shape, mode, gpu_device)
    if kind in ("constant", "all_invalid"):
        assert val == (1.0 if mode == "pearson" else 0.0)
        assert not gd.view(torch.int32).any() and (ga is None or not ga.view(torch.int32).any())
    if kind == "affine":
        assert val <= 2e-6
    if kind in ("alpha_straddle", "bad_prior"):
        assert 0 < int((~r["ok"]).sum()) < r["ok"].numel()


@pytest.mark.parametrize("mode", ["pearson", "ssi"])
@pytest.mark.parametrize("shape", SHAPES + [BIG], ids=["%dx%d" % s for s in SHAPES + [BIG]])
@pytest.mark.parametrize("kind", ["smooth", "alpha_straddle"])
def test_loss_shapes_against_float64(kind, shape, mode, gpu_device):
    """1x1 (n < 2: degenerate) and 1x2, single rows and columns, below / at / above the 16-pixel tile and the 1024-pixel chunk of a
    workgroup, and one image with more workgroups than one trip of the finish loop."""
    from fdgs import _capi
    H, W = shape
    assert _capi.lib.fdgs_depth_loss_num_partials(H, W) == 16 + 7 * ((H * W + 1023) // 1024)
    if shape == BIG:
        assert (H * W + 1023) // 1024 > 256
    r, val, gd, ga = _check_loss(kind, shape, mode, gpu_device)
    if r["stats"][0] < 2:
        assert val == (1.0 if mode == "pearson" else 0.0) and not gd.view(torch.int32).any()


# ---- 2. every output element written, nothing around it -------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["pearson", "ssi"])
@pytest.mark.parametrize("shape", [(1, 7), (17, 19), (33, 31)], ids=["1x7", "17x19", "33x31"])
def test_loss_writes_every_output_element_and_nothing_else(shape, mode, gpu_device):
    """The C ABI directly: both gradients, the 4 output floats and the partials are slices of larger buffers pre-filled with a NaN
    pattern, 4096 elements of guard on both sides; afterwards every gradient / output element is written and finite, every guard
    element still holds its pattern, and what was written is the loss: value and gradients against the float64 reference."""
    from fdgs import _capi
    dev = gpu_device
    H, W = shape
    r = loss_ref("alpha_straddle", shape, mode)
    g = _to(r["x"], dev)
    up = torch.full((1,), UP, dtype=torch.float32, device=dev)
    gd, ga, out = _Guarded(H * W, dev), _Guarded(H * W, dev), _Guarded(4, dev)
    parts = _Guarded(_capi.lib.fdgs_depth_loss_num_partials(H, W), dev, torch.float64)
    din = _capi.FdgsDepthIn(H, W, g["depth"].data_ptr(), g["alpha"].data_ptr(), _capi._ptr(g["mask"]), 0.5)
    grads = _capi.FdgsDepthGrads(gd.ptr, ga.ptr, up.data_ptr(), 1.0, 0)
    with torch.cuda.device(dev):
        rc = _capi.lib.fdgs_depth_loss(C.byref(din), g["prior"].data_ptr(), 0 if mode == "pearson" else 1, C.byref(grads), parts.ptr,
                                       out.ptr, _capi.current_stream_handle(dev))
        assert rc == 0, _capi.last_error()
        torch.cuda.synchronize()
    parts.check("partials", all_written=False)
    o = out.check("out").cpu()
    d, a = gd.check("d_depth").cpu(), ga.check("d_alpha").cpu()
    assert torch.isfinite(o).all() and torch.isfinite(d).all() and torch.isfinite(a).all()
    assert abs(float(o[0]) - r["value"]) <= r["bar_v"] and float(o[1]) == r["stats"][0]
    assert float((d.double() - UP * r["gd"].view(-1)).abs().max()) <= UP * r["bar_gd"]
    assert float((a.double() - UP * r["ga"].view(-1)).abs().max()) <= UP * r["bar_ga"]
    # accumulate = 1 adds the same gradient once more, scale scales it
    grads2 = _capi.FdgsDepthGrads(gd.ptr, ga.ptr, None, 2.0 * UP, 1)
    with torch.cuda.device(dev):
        assert _capi.lib.fdgs_depth_loss(C.byref(din), g["prior"].data_ptr(), 0 if mode == "pearson" else 1, C.byref(grads2), parts.ptr,
                                         out.ptr, _capi.current_stream_handle(dev)) == 0
        torch.cuda.synchronize()
    assert float((gd.check("d_depth").cpu().double() - 3 * UP * r["gd"].view(-1)).abs().max()) <= 3 * UP * r["bar_gd"] + 1e-7 * float(r["gd"].abs().max())


# ---- 3. normals -----------------------------------------------------------------------------------------------------------------
def _holes(H, W):
    """A mask with holes on the 16 x 16 tile edges and corners: x or y = 0, 1, 15 (mod 16)."""
    m = torch.ones(1, H, W)
    for y in range(H):
        for x in range(W):
            if (x % 16 in (0, 1, 15) or y % 16 in (0, 1, 15)) and (x * 7 + y * 13) % 5 == 0:
                m[0, y, x] = 0
    return m


@functools.lru_cache(maxsize=None)
def normal_ref(kind, shape, world):
    H, W = shape
    x = dict(do.make_inputs(kind, H, W))
    if kind == "smooth":
        x["mask"] = _holes(H, W)
    intr = do.intrinsics_for(H, W)
    from fdgs import synth
    vm = synth.camera_for("rig1", W, H)["world_view_transform"] if world else None
    w = torch.randn(3, H, W, generator=torch.Generator().manual_seed(11))
    out = {"x": x, "intr": intr, "vm": vm, "w": w}
    for dt, tag in ((torch.float64, "64"), (torch.float32, "32")):
        holder = {}

        def fn(d, a):
            n, valid, len2 = do.normals(d, a, intr, x["mask"], viewmatrix=vm, dtype=dt)
            holder.update(n=n.detach().double(), valid=valid, len2=len2)
            return (n * w.to(dt)).sum(), None
        _, _, gd, ga = _grads(fn, x, dt)
        out["n" + tag], out["valid" + tag], out["len2" + tag], out["gd" + tag], out["ga" + tag] = holder["n"], holder["valid"], holder["len2"], gd, ga
    out["err_n"] = float((out["n32"] - out["n64"]).abs().max())
    out["err_gd"] = float((out["gd32"] - out["gd64"]).abs().max())
    out["err_ga"] = 0.0 if out["ga64"] is None else float((out["ga32"] - out["ga64"]).abs().max())
    floor = out if kind == "smooth" else normal_ref("smooth", shape, world)
    for k in ("n", "gd", "ga"):
        out["bar_" + k] = MARGIN * max(out["err_" + k], floor["err_" + k])
    return out


def _run_normals(r, dev):
    from fdgs import depth
    g = _to(r["x"], dev)
    d = g["depth"].requires_grad_(True)
    a = None if g["alpha"] is None else g["alpha"].requires_grad_(True)
    n, valid = depth.depth_normals(d, a, r["intr"], g["mask"], viewmatrix=None if r["vm"] is None else r["vm"].to(dev))
    (n * r["w"].to(dev)).sum().backward()
    torch.cuda.synchronize()
    return n.detach().cpu(), valid.cpu(), d.grad.cpu(), None if a is None else a.grad.cpu()


@pytest.mark.parametrize("world", [False, True], ids=["view", "world"])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
@pytest.mark.parametrize("kind", ["smooth", "alpha_straddle", "alpha_none"])
def test_normals_forward_and_backward_against_float64(kind, shape, world, gpu_device):
    """Normals, validity and the gather backward under a random dL/dn, in view space and rotated to world space; ``smooth`` carries a
    mask with holes on the tile edges and corners (x or y = 0, 1, 15 mod 16).  ``valid`` must equal the oracle's bit for bit: the inputs
    keep |b x a|^2 away from the 1e-20 threshold (asserted).  Exact +0 gradient wherever z is invalid."""
    r = normal_ref(kind, shape, world)
    H, W = shape
    len2 = r["len264"]
    assert not ((len2 > 1e-20 * (1 - 1e-3)) & (len2 < 1e-20 * (1 + 1e-3))).any(), "the input puts a stencil on the threshold"
    assert torch.equal(r["valid64"], r["valid32"])
    n, valid, gd, ga = _run_normals(r, gpu_device)
    assert n.shape == (3, H, W) and valid.shape == (1, H, W) and valid.dtype == torch.uint8
    assert torch.equal(valid.bool(), r["valid64"]), "valid differs from the oracle's on %d pixels" % int((valid.bool() != r["valid64"]).sum())
    if min(H, W) >= 15:
        assert 0 < int(valid.sum()) <= (H - 2) * (W - 2) and (kind == "alpha_none") == (int(valid.sum()) == (H - 2) * (W - 2))
    assert not n[:, ~valid[0].bool()].view(torch.int32).any(), "a normal is not +0 where valid = 0"
    err_n = float((n.double() - r["n64"]).abs().max())
    err_gd = float((gd.double() - r["gd64"]).abs().max())
    rn, rd = _ratio("normals", err_n, r["bar_n"]), _ratio("normals d_depth", err_gd, r["bar_gd"])
    line = "%-14s %-7s %-5s | normals err %.2e (bar %.2e, ratio %.2f) | d_depth err %.2e (bar %.2e, ratio %.2f, max|g| %.2e)" % (
        kind, "%dx%d" % shape, "world" if world else "view", err_n, r["bar_n"], rn, err_gd, r["bar_gd"], rd, float(r["gd64"].abs().max()))
    _, ok = do.depth_z(r["x"]["depth"], r["x"]["alpha"], r["x"]["mask"], 0.5, torch.float64)
    assert torch.isfinite(n).all() and torch.isfinite(gd).all()
    assert not gd.view(-1)[~ok.view(-1)].view(torch.int32).any(), "d_depth is not +0 at an invalid pixel"
    assert rn <= 1.0, line
    assert rd <= 1.0, line
    if ga is not None:
        err_ga = float((ga.double() - r["ga64"]).abs().max())
        ra = _ratio("normals d_alpha", err_ga, r["bar_ga"])
        line += " | d_alpha err %.2e (bar %.2e, ratio %.2f)" % (err_ga, r["bar_ga"], ra)
        assert torch.isfinite(ga).all()
        assert not ga.view(-1)[~ok.view(-1)].view(torch.int32).any(), "d_alpha is not +0 at an invalid pixel"
        assert ra <= 1.0, line
    print(line)


@pytest.mark.parametrize("shape", [(1, 7), (17, 19), (33, 31)], ids=["1x7", "17x19", "33x31"])
def test_normals_write_every_output_element_and_nothing_else(shape, gpu_device):
    from fdgs import _capi
    dev = gpu_device
    H, W = shape
    r = normal_ref("smooth", shape, True)
    g = _to(r["x"], dev)
    vm, w = r["vm"].to(dev).contiguous(), r["w"].to(dev).contiguous()
    nrm, val = _Guarded(3 * H * W, dev), _Guarded(H * W, dev, torch.uint8)
    gd, ga = _Guarded(H * W, dev), _Guarded(H * W, dev)
    din = _capi.FdgsDepthIn(H, W, g["depth"].data_ptr(), g["alpha"].data_ptr(), _capi._ptr(g["mask"]), 0.5)
    grads = _capi.FdgsDepthGrads(gd.ptr, ga.ptr, None, 1.0, 0)
    with torch.cuda.device(dev):
        st = _capi.current_stream_handle(dev)
        assert _capi.lib.fdgs_depth_normals(C.byref(din), *r["intr"], vm.data_ptr(), nrm.ptr, val.ptr, st) == 0, _capi.last_error()
        assert _capi.lib.fdgs_depth_normals_backward(C.byref(din), *r["intr"], vm.data_ptr(), w.data_ptr(), C.byref(grads), st) == 0, _capi.last_error()
        torch.cuda.synchronize()
    n = nrm.check("normals").cpu().view(3, H, W)
    val.check("valid", all_written=False)          # (0xAB is no value the kernel writes, but check the body explicitly)
    v = val.body().cpu()
    assert set(v.unique().tolist()) <= {0, 1}
    d, a = gd.check("d_depth").cpu(), ga.check("d_alpha").cpu()
    assert torch.equal(v.view(1, H, W).bool(), r["valid64"])
    assert float((n.double() - r["n64"]).abs().max()) <= r["bar_n"]
    assert float((d.double() - r["gd64"].view(-1)).abs().max()) <= r["bar_gd"]
    assert float((a.double() - r["ga64"].view(-1)).abs().max()) <= r["bar_ga"]


def test_normal_loss_matches_its_statement(gpu_device):
    from fdgs import depth
    r = normal_ref("smooth", (33, 31), False)
    n, valid, _, _ = _run_normals(r, gpu_device)
    prior = torch.nn.functional.normalize(torch.randn(3, 33, 31, generator=torch.Generator().manual_seed(4)), dim=0)
    got = depth.normal_loss(n.to(gpu_device), valid.to(gpu_device), prior.to(gpu_device))
    want = do.normal_loss(r["n64"], r["valid64"], prior.double())
    assert got.is_cuda and abs(float(got) - float(want)) <= 1e-5
    none = depth.normal_loss(n.to(gpu_device), torch.zeros_like(valid).to(gpu_device), prior.to(gpu_device))
    assert float(none) == 0.0


# ---- 4. reproducibility ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(33, 31), BIG], ids=["33x31", "515x513"])
def test_two_runs_are_bit_identical(shape, gpu_device):
    """Every kernel twice on one input: values, statistics, gradients, normals and validity agree bit for bit (no atomics anywhere)."""
    r = loss_ref("alpha_straddle", shape, "ssi")
    for mode in ("pearson", "ssi"):
        a, b = _run_loss(r["x"], mode, gpu_device), _run_loss(r["x"], mode, gpu_device)
        assert a[0] == b[0] and torch.equal(a[1], b[1])
        assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32)) and torch.equal(a[3].view(torch.int32), b[3].view(torch.int32))
    H, W = shape
    nr = {"x": r["x"], "intr": do.intrinsics_for(H, W), "vm": None, "w": torch.randn(3, H, W, generator=torch.Generator().manual_seed(5))}
    a, b = _run_normals(nr, gpu_device), _run_normals(nr, gpu_device)
    assert torch.equal(a[1], b[1])
    for i in (0, 2, 3):
        assert torch.equal(a[i].view(torch.int32), b[i].view(torch.int32))


# ---- 5. end to end through the rasterizer ---------------------------------------------------------------------------------------
def _scene_and_priors(dev):
    from fdgs import depth, synth, train_host
    from fdgs.fused import render_raw
    cfg = synth.SceneConfig("depth", 400, 64, 48, 1, 0, 0.2, 1.0, True, 4, True)
    scene = synth.make_scene(cfg, seed=9, pose="rig2")
    cam, pipe, bg = train_host.SyntheticCamera(scene, dev), train_host.PipelineFlags(), scene["bg"].to(dev)
    target = train_host.GaussianParams(scene, dev)
    with torch.no_grad():
        pkg = render_raw(cam, target, pipe, bg)
        z = pkg["depth"] / pkg["alpha"].clamp(min=0.5)
    g = torch.Generator().manual_seed(21)
    prior = (0.6 * z + 1.5 + 0.05 * torch.randn(z.shape, generator=g).to(dev)).clamp(min=0.05)       # an unknown affine map plus noise
    intr = depth.intrinsics_of(cam)
    with torch.no_grad():
        n_prior, _ = depth.depth_normals(pkg["depth"], pkg["alpha"], intr)
    n_prior = torch.nn.functional.normalize(n_prior + 0.1 * torch.randn(n_prior.shape, generator=g).to(dev), dim=0, eps=1e-6)
    return scene, cam, pipe, bg, prior, n_prior, intr, z


def _perturbed(scene, dev):
    from fdgs import train_host
    model = train_host.GaussianParams(scene, dev)
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        model.params["_xyz"].add_(0.05 * torch.randn(model.params["_xyz"].shape, generator=g).to(dev))
        model.params["_opacity"].add_(0.3 * torch.randn(model.params["_opacity"].shape, generator=g).to(dev))
    return model


@pytest.mark.parametrize("mode", ["pearson", "ssi"])
@pytest.mark.parametrize("path", ["render", "render_raw"])
def test_end_to_end_gradients_match_the_torch_formulation(path, mode, gpu_device):
    """depth_loss + normal_loss(depth_normals) on render()'s / render_raw()'s outputs, backward to the parameters, against the same
    graph with the new terms replaced by their float32 torch formulation on the GPU (tests/depth_oracle.py on device tensors).  The
    rasterizer backward is the same on both sides; the bar is the one of tests/test_gpu_api.py: 1e-4 of max(1, max|ref|)."""
    from fdgs import depth
    from fdgs.fused import render_raw
    from fdgs.gaussian_renderer import render
    dev = gpu_device
    scene, cam, pipe, bg, prior, n_prior, intr, _ = _scene_and_priors(dev)
    fn = render if path == "render" else render_raw
    got = {}
    for side in ("hip", "torch"):
        model = _perturbed(scene, dev)
        pkg = fn(cam, model, pipe, bg)
        if side == "hip":
            ld, stats = depth.depth_loss(pkg["depth"], pkg["alpha"], prior, mode=mode, return_stats=True)
            n, valid = depth.depth_normals(pkg["depth"], pkg["alpha"], intr)
            ln = depth.normal_loss(n, valid, n_prior)
            assert float(stats[0]) >= 300, "the scene covers too few pixels for the test to mean anything"
            assert int(valid.sum()) >= 100
        else:
            ld, _ = do.depth_loss(pkg["depth"], pkg["alpha"], prior, mode=mode, dtype=torch.float32)
            n, valid, _ = do.normals(pkg["depth"], pkg["alpha"], intr, dtype=torch.float32)
            ln = do.normal_loss(n, valid, n_prior)
        (ld + 0.5 * ln).backward()
        torch.cuda.synchronize()
        got[side] = (float(ld.detach()), float(ln.detach()), {k: p.grad.detach().double().cpu() for k, p in model.params.items()})
    assert abs(got["hip"][0] - got["torch"][0]) <= 1e-5 and abs(got["hip"][1] - got["torch"][1]) <= 1e-5
    moved = 0
    for name, ref in got["torch"][2].items():
        g = got["hip"][2][name]
        scale = max(1.0, float(ref.abs().max()))
        err = float((g - ref).abs().max())
        moved += float(ref.abs().sum()) > 0
        print("%s %s %-12s max abs gap %.2e (max|ref| %.2e, bar %.1e)" % (path, mode, name, err, float(ref.abs().max()), 1e-4 * scale))
        assert torch.isfinite(g).all()
        assert err <= 1e-4 * scale, (name, err, scale)
    assert moved >= 4, "the depth terms reached too few parameter tensors"


def test_twenty_steps_lower_the_aligned_depth_error(gpu_device):
    """examples/train_with_depth.py at tiny size, in this process: twenty optimiser steps with the depth term lower the training
    views' depth error after alignment."""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "train_with_depth.py")
    spec = importlib.util.spec_from_file_location("train_with_depth", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    r = mod.run(gpu_device, iterations=20, lambda_depth=2.0, W=64, H=48, P=400, s0=0.2, seed=9, log=None)
    print("aligned depth error of the training views: %.5f -> %.5f; held-out %.5f, PSNR %.2f dB" % (
        r["train_depth_error_before"], r["train_depth_error_after"], r["heldout_depth_error"], r["heldout_psnr"]))
    assert r["train_depth_error_before"] > 0
    assert r["train_depth_error_after"] < r["train_depth_error_before"]


def test_worst_ratios_are_reported():
    """Not a check of its own: prints the worst error / bar ratios the tests above observed (DESIGN.md section 4.7 records them)."""
    for k, v in sorted(WORST.items()):
        print("worst ratio %-18s %.3f" % (k, v))
