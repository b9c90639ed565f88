"""GPU: the k-NN query (fdgs.knn.knn), the rigid / motion regularisers (fdgs.loss.rigid_motion_loss) and the opacity-mask loss
(fdgs.loss.opa_mask_loss) against the CPU oracle (tests/regularizer_oracle.py), and a reference-style training loop with them."""
import numpy as np
import pytest
import torch

from util import synth
import regularizer_oracle as ro

pytestmark = pytest.mark.gpu
SC = synth.SceneConfig


def _pts(P, seed, kind):
    rng = np.random.default_rng(seed)
    if kind == "gauss":
        return (rng.standard_normal((P, 3)) * np.array([3.0, 1.0, 0.2])).astype(np.float32)
    if kind == "shifted":
        return (rng.random((P, 3)) + np.array([50.0, -20.0, 7.0])).astype(np.float32)
    if kind == "dups":
        base = rng.standard_normal((max(P // 3, 1), 3)).astype(np.float32)
        return base[rng.integers(0, base.shape[0], P)]
    raise ValueError(kind)


def _check_rows(got_i, got_d, want_i, want_d):
    np.testing.assert_array_equal(got_d.view(np.uint32), want_d.view(np.uint32))
    np.testing.assert_array_equal(got_i, want_i)


@pytest.mark.parametrize("k", [1, 3, 8, 20, 32, 64])
@pytest.mark.parametrize("P,kind", [(1, "gauss"), (5, "gauss"), (19, "gauss"), (20, "gauss"), (21, "gauss"), (1025, "shifted"),
                                    (4097, "dups"), (20000, "gauss")])
def test_knn_exact_vs_oracle(P, kind, k, gpu_device):
    """b = 2, queries != sources (their own set, of another size): d2 bit-exact, indices exact under the (d2, index) rule,
    slots beyond the sources padded with (1e10, 0)."""
    from fdgs.knn import knn
    n = max(1, P // 2 + 3)
    src = np.stack([_pts(P, 11 * P + b, kind) for b in range(2)])
    x = np.stack([_pts(n, 13 * P + b, kind) for b in range(2)])
    if kind == "dups":
        x[:, : n // 2] = src[:, : n // 2]          # queries sitting on (duplicated) sources: ties at d2 = 0
    idx, d2 = knn(torch.from_numpy(x).to(gpu_device), torch.from_numpy(src).to(gpu_device), k)
    assert idx.dtype == torch.int64 and d2.dtype == torch.float32 and tuple(idx.shape) == (2, n, k)
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    rows = np.arange(n) if n <= 5000 else np.random.default_rng(P + k).choice(n, 1500, replace=False)
    for b in range(2):
        wi, wd = ro.knn(x[b], src[b], k, rows=rows)
        _check_rows(idx[b][rows], d2[b][rows], wi, wd)
    if P < k:
        assert (d2[:, :, P:] == 1e10).all() and (idx[:, :, P:] == 0).all()


def test_knn_self_query_and_transpose(gpu_device):
    from fdgs.knn import knn
    pts = torch.from_numpy(_pts(3000, 5, "dups")).to(gpu_device)[None]
    idx, d2 = knn(pts, pts, 20)
    assert (d2[..., 0] == 0).all()
    idx_t, d2_t = knn(pts.transpose(1, 2), pts.transpose(1, 2), 20, transpose=True)
    assert torch.equal(idx, idx_t) and torch.equal(d2, d2_t)
    wi, wd = ro.knn(pts[0].cpu().numpy(), pts[0].cpu().numpy(), 20)
    _check_rows(idx[0].cpu().numpy(), d2[0].cpu().numpy(), wi, wd)


def test_knn_at_c3_size_sampled_rows(gpu_device):
    """The C3 means (300 k), k = 20: 2000 sampled rows against brute force over all of them."""
    from fdgs.knn import knn
    scene = synth.make_scene(synth.CONFIGS["C3"], seed=0)
    pts = scene["means3D"].float().contiguous()
    idx, d2 = knn(pts.to(gpu_device)[None], pts.to(gpu_device)[None], 20)
    rows = np.random.default_rng(3).choice(pts.shape[0], 2000, replace=False)
    wi, wd = ro.knn(pts.numpy(), pts.numpy(), 20, rows=rows, chunk=50)
    _check_rows(idx[0].cpu().numpy()[rows], d2[0].cpu().numpy()[rows], wi, wd)


def test_knn_refuses_what_it_does_not_do(gpu_device):
    from fdgs.knn import knn
    x = torch.zeros(1, 10, 3, device=gpu_device)
    with pytest.raises(ValueError, match="k <= 64"):
        knn(x, x, 65)
    with pytest.raises(ValueError, match="k <= 64"):
        knn(x, x, 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        knn(x.cpu(), x.cpu(), 3)


# ---- rigid + motion ----

def _model(dev, P, seed, dup=0):
    from fdgs import train_host
    cfg = SC("reg", P, 96, 64, 1, 1, 0.05, 10.0, True, 4, False)
    scene = synth.make_scene(cfg, seed=seed)
    m = train_host.ReferenceStyleModel(scene, dev)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        m._rotation.mul_((0.5 + 1.5 * torch.rand(P, 1, generator=g)).to(dev))
        m._rotation_r.mul_((0.5 + 1.5 * torch.rand(P, 1, generator=g)).to(dev))
        m._scaling_t.add_((torch.randn(P, 1, generator=g) * 0.3).to(dev))
        if dup:   # densification clones: exact copies of the first `dup` Gaussians appended
            for n in ("_xyz", "_scaling", "_scaling_t", "_rotation", "_rotation_r", "_t"):
                t = getattr(m, n)
                setattr(m, n, torch.nn.Parameter(torch.cat([t, t[:dup]]).contiguous()))
    return m


NAMES4 = ("_scaling", "_scaling_t", "_rotation", "_rotation_r")


def _kernel_run(m, k, g_rigid=1.0, g_motion=0.5):
    from fdgs.loss import rigid_motion_loss
    for n in NAMES4:
        getattr(m, n).grad = None
    lr, lm = rigid_motion_loss(m, k)
    (g_rigid * lr + g_motion * lm).backward()
    return float(lr.detach()), float(lm.detach()), {n: getattr(m, n).grad.detach().cpu().clone() for n in NAMES4}


def _oracle_run(m, k, g_rigid=1.0, g_motion=0.5):
    from fdgs.knn import knn
    idx, d2 = knn(m._xyz.detach()[None], m._xyz.detach()[None], k)
    params = {n: getattr(m, n).detach().cpu() for n in NAMES4 + ("_t",)}
    return ro.rigid_motion_with_grads(params, idx[0].cpu(), d2[0].cpu(), torch.float64, g_rigid, g_motion)


@pytest.mark.parametrize("P,dup,k", [(700, 0, 20), (3000, 0, 8), (2000, 400, 20), (300_000, 0, 20)], ids=["small", "k8", "clones", "C3"])
def test_rigid_motion_vs_float64_oracle(P, dup, k, gpu_device):
    m = _model(gpu_device, P, seed=P + dup, dup=dup)
    lr, lm, g = _kernel_run(m, k)
    wr, wm, wg = _oracle_run(m, k)
    assert abs(lr - wr) <= 1e-5 * abs(wr) and abs(lm - wm) <= 1e-5 * abs(wm), (lr, wr, lm, wm)
    for n in NAMES4:
        ref = wg[n].float()
        err = float((g[n] - ref).abs().max())
        assert err <= 1e-4 * max(1.0, float(ref.abs().max())), (n, err, float(ref.abs().max()))


def test_rigid_motion_gradient_is_bit_reproducible(gpu_device):
    m = _model(gpu_device, 20000, seed=9, dup=3000)
    a = _kernel_run(m, 20)
    b = _kernel_run(m, 20)
    assert a[0] == b[0] and a[1] == b[1]
    for n in NAMES4:
        assert torch.equal(a[2][n], b[2][n]), n


def test_rigid_motion_on_the_flat_bucket_model(gpu_device):
    """GaussianParams: the gradients land in the flat gradient bucket's slices (the reference attribute names)."""
    from fdgs import train_host
    from fdgs.loss import rigid_motion_loss
    scene = synth.make_scene(SC("reg", 1500, 96, 64, 1, 1, 0.05, 10.0, True, 4, False), seed=2)
    gp = train_host.GaussianParams(scene, gpu_device)
    gp.zero_grad()
    lr, lm = rigid_motion_loss(gp)
    (lr + lm).backward()
    wr, wm, wg = _oracle_run(gp, 20, 1.0, 1.0)
    assert abs(float(lr) - wr) <= 1e-5 * abs(wr)
    for n in NAMES4:
        got = gp.flat_grad[gp.offsets[n][0]:gp.offsets[n][1]].view(wg[n].shape).cpu()
        assert float((got - wg[n].float()).abs().max()) <= 1e-4 * max(1.0, float(wg[n].abs().max())), n


def test_rigid_motion_refuses_a_model_without_rot_4d(gpu_device):
    from fdgs import train_host
    from fdgs.loss import rigid_motion_loss
    scene = synth.make_scene(SC("norot", 500, 96, 64, 1, 0, 0.05, 1.0, False, 4, True), seed=1)
    with pytest.raises(ValueError, match="rot_4d"):
        rigid_motion_loss(train_host.ReferenceStyleModel(scene, gpu_device))


# ---- opacity mask ----

def test_opa_mask_value_and_gradient_vs_oracle(gpu_device):
    from fdgs.loss import opa_mask_loss
    H, W = 97, 131
    gen = torch.Generator().manual_seed(4)
    alpha = torch.rand(1, H, W, generator=gen)
    flat = alpha.view(-1)
    flat[:6] = torch.tensor([1e-6, 1 - 1e-6, 0.0, 1.0, 1e-7, 1 - 1e-7])   # at and beyond both clamp bounds
    mask = (torch.rand(1, H, W, generator=gen) > 0.4).float()
    mask.view(-1)[:6] = 0.0    # sky = 1 there: the clamp decides the gradient
    a = alpha.to(gpu_device).requires_grad_(True)
    val = opa_mask_loss(a, mask.to(gpu_device))
    (3.0 * val).backward()
    ar = alpha.double().requires_grad_(True)
    want = ro.opa_mask(ar, mask.double(), bounds=ro.OPA_BOUNDS_F32)
    (3.0 * want).backward()
    assert abs(float(val) - float(want)) <= 1e-5 * abs(float(want))
    g = a.grad.cpu().double()
    torch.testing.assert_close(g, ar.grad, rtol=1e-5, atol=1e-12)
    # torch.clamp passes the gradient AT both float32 bounds and blocks it beyond them
    assert (g.view(-1)[:2] > 0).all() and (g.view(-1)[2:6] == 0).all(), g.view(-1)[:6]


def test_render_with_opa_mask_matches_the_torch_expression(gpu_device):
    """render()'s alpha -> opa_mask_loss gives the parameter gradients of the reference's torch expression (blend AUX path)."""
    from fdgs import train_host
    from fdgs.gaussian_renderer import render
    from fdgs.loss import opa_mask_loss
    scene = synth.make_scene(SC("opa", 4000, 160, 112, 2, 1, 0.03, 10.0, True, 4, False), seed=6)
    model = train_host.ReferenceStyleModel(scene, gpu_device)
    cam = train_host.SyntheticCamera(scene, gpu_device, timestamp=0.4 * scene["time_duration"])
    bg = torch.tensor([0.1, 0.2, 0.3], device=gpu_device)
    mask = (torch.rand(1, scene["H"], scene["W"], generator=torch.Generator().manual_seed(1)) > 0.5).float().to(gpu_device)
    names = ("_xyz", "_opacity", "_scaling", "_rotation", "_t", "_scaling_t", "_rotation_r")
    grads = {}
    for which in ("fdgs", "torch"):
        for n in names:
            getattr(model, n).grad = None
        pkg = render(cam, model, train_host.PipelineFlags(), bg)
        loss = opa_mask_loss(pkg["alpha"], mask) if which == "fdgs" else ro.opa_mask(pkg["alpha"], mask)
        loss.backward()
        grads[which] = {n: getattr(model, n).grad.detach().clone() for n in names}
    for n in names:
        ref = grads["torch"][n]
        err = float((grads["fdgs"][n] - ref).abs().max())
        assert err <= 1e-4 * max(1.0, float(ref.abs().max())), (n, err)


def test_reference_loop_with_the_regularisers(gpu_device):
    """ReferenceStyleModel + render() + fdgs.optim.Adam + the fused terms against torch.optim.Adam + the torch oracle terms."""
    from fdgs import train_host
    from fdgs.gaussian_renderer import render
    from fdgs.knn import knn
    from fdgs.loss import opa_mask_loss, rigid_motion_loss
    cfg = SC("loop", 5000, 160, 112, 2, 1, 0.03, 10.0, True, 4, False)
    scene = synth.make_scene(cfg, seed=8)
    gen = torch.Generator().manual_seed(2)
    gts = [torch.rand(3, cfg.H, cfg.W, generator=gen).to(gpu_device) for _ in range(2)]
    masks = [(torch.rand(1, cfg.H, cfg.W, generator=gen) > 0.5).float().to(gpu_device) for _ in range(2)]
    bg = torch.tensor([0.1, 0.2, 0.3], device=gpu_device)
    final, losses, first = {}, {}, {}
    for which in ("fdgs", "torch"):
        model = train_host.ReferenceStyleModel(scene, gpu_device, optimizer=which)
        for g in model.optimizer.param_groups:
            g["lr"] = 1e-3
        cams = [train_host.SyntheticCamera(scene, gpu_device, timestamp=(b + 0.5) / 2 * scene["time_duration"]) for b in range(2)]
        hist = []
        for step in range(3):
            model.optimizer.zero_grad(set_to_none=True)
            for b in range(2):
                pkg = render(cams[b], model, train_host.PipelineFlags(), bg)
                loss = (pkg["render"] - gts[b]).abs().mean()
                if which == "fdgs":
                    lo = opa_mask_loss(pkg["alpha"], masks[b])
                    lr, lm = rigid_motion_loss(model, 20)
                else:
                    lo = ro.opa_mask(pkg["alpha"], masks[b])
                    idx, d2 = knn(model.get_xyz.detach()[None], model.get_xyz.detach()[None], 20)
                    v = ro.velocity(model._scaling, model._scaling_t, model._rotation, model._rotation_r, model._t, torch.float32)
                    lr, lm = ro.rigid(v, idx[0], d2[0]), ro.motion(v)
                loss = loss + 0.5 * lo + 1.0 * lr + 0.1 * lm
                (loss / 2).backward()
                hist.append(float(loss))
            if step == 0:
                first[which] = {n: getattr(model, n).grad.detach().clone() for n in ("_scaling", "_rotation", "_scaling_t", "_rotation_r")}
            model.optimizer.step()
        losses[which] = hist
        final[which] = {n: getattr(model, n).detach().clone() for n in ("_xyz", "_scaling", "_rotation", "_scaling_t", "_rotation_r")}
    np.testing.assert_allclose(losses["fdgs"], losses["torch"], rtol=2e-5)
    for n, ref in first["torch"].items():
        err = float((first["fdgs"][n] - ref).abs().max())
        assert err <= 1e-4 * max(1.0, float(ref.abs().max())), (n, err)
    # Adam divides by sqrt(v): where a gradient is ~0 an ulp of difference can move that element by up to lr per step, so the
    # parameters are held to the project's bar on all but 0.1 % of their elements and to Adam's bounded step (3 steps x lr) everywhere
    for n, ref in final["torch"].items():
        d = (final["fdgs"][n] - ref).abs()
        bar = 1e-4 * max(1.0, float(ref.abs().max()))
        assert float((d > bar).float().mean()) <= 1e-3 and float(d.max()) <= 3 * 1e-3 * 1.01, (n, float(d.max()))
