"""GPU: StepPipeline(exposure=) against the plain pipeline (identity table) and against render_raw + exposure.apply + fused_l1_ssim +
backward() per view with the oracle's Adam on the table; the direction a known gain pulls the rows in; held-out evaluation.

The comparator of two pipelines on the same numbers is tests/test_gpu_api.py's: losses to rtol 3e-5 / atol 1e-6, gradients to 1e-3
of their scale, parameters after Adam steps to its float-atomics bar."""
import numpy as np
import pytest
import torch

import exposure_oracle as eo
from util import synth
from test_gpu_envmap import smooth_env

pytestmark = pytest.mark.gpu
B = 3
ENV = (24, 48)


class Pipe:
    compute_cov3D_python = False
    convert_SHs_python = False
    debug = False

    def __init__(self, res=0):
        self.env_map_res = res


def _setup(dev, seed=4):
    from fdgs import train_host
    cfg = synth.SceneConfig("exposure", 400, 64, 48, 3, 2, 0.06, 4.0, True, 4, False)
    scene = synth.make_scene(cfg, seed=seed)
    cams = [train_host.SyntheticCamera(scene, dev, timestamp=(b + 0.5) / B * scene["time_duration"]) for b in range(B)]
    for b, c in enumerate(cams):
        c.uid = b
    gen = torch.Generator(device="cpu").manual_seed(7)
    gts = [torch.rand(3, scene["H"], scene["W"], generator=gen).to(dev) for _ in range(B)]
    return scene, cams, gts, torch.tensor([0.1, 0.2, 0.3], device=dev)


def _model(scene, dev, env=False):
    from fdgs import train_host
    m = train_host.GaussianParams(scene, dev)
    if env:
        m.env_map = smooth_env(*ENV, 9, dev).requires_grad_(True)
    return m


def _random_table(dev, n=B + 1):
    """Rows near the identity, every one different; one more row than cameras (it must stay as it is)."""
    rng = np.random.default_rng(3)
    t = np.tile(eo.IDENTITY, (n, 1)) + np.concatenate([rng.normal(0, 0.2, (n, 3, 3)), rng.normal(0, 0.05, (n, 3, 1))], axis=2).reshape(n, 12)
    return torch.from_numpy(t.astype(np.float32)).to(dev)


def _exposure(dev, table=None, **kw):
    from fdgs.exposure import ExposureModel
    ex = ExposureModel(B + 1, dev, **kw)
    if table is not None:
        ex.table.copy_(table)
    return ex


def _close_params(a, b):
    perr = (a - b).abs()
    assert (perr > 2e-3).float().mean().item() <= 2e-3 and perr.max().item() <= 0.25, ((perr > 2e-3).float().mean().item(), perr.max().item())


def _close_grads(got, ref):
    gerr, gscale = (got - ref).abs().max().item(), max(1e-6, ref.abs().max().item())
    assert gerr <= 1e-3 * gscale, (gerr, gscale)


def test_identity_table_is_the_plain_pipeline(gpu_device):
    """(a) identity rows, optimize_exposure=False: three steps give the plain pipeline's losses and parameters; the corrected image is
    the rasterizer's bit for bit; the table and its moments are never touched."""
    from fdgs import train_host
    from fdgs.pipeline import StepPipeline
    scene, cams, gts, bg = _setup(gpu_device)
    runs = {}
    for mode in ("plain", "exposure"):
        m = _model(scene, gpu_device)
        ex = _exposure(gpu_device) if mode == "exposure" else None
        sp = StepPipeline(m, train_host.make_optimizer(m), world_size=1, lambda_dssim=0.2, **({"exposure": ex} if ex is not None else {}))
        losses = []
        for _ in range(3):
            res, ls = sp.step(cams, gts, Pipe(), bg, **({"optimize_exposure": False} if ex is not None else {}))
            losses += [float(l) for l in ls]
            for r in res:
                assert ("render_uncorrected" in r) == (ex is not None)
                if ex is not None:
                    assert r["render"].data_ptr() != r["render_uncorrected"].data_ptr() and torch.equal(r["render"], r["render_uncorrected"])
        torch.cuda.synchronize()
        runs[mode] = (m.flat.detach().clone(), losses, ex)
    np.testing.assert_allclose(runs["exposure"][1], runs["plain"][1], rtol=3e-5, atol=1e-6)
    _close_params(runs["exposure"][0], runs["plain"][0])
    ex = runs["exposure"][2]
    assert np.array_equal(ex.table.cpu().numpy(), np.tile(eo.IDENTITY.astype(np.float32), (B + 1, 1)))
    assert not ex.exp_avg.any() and not ex.exp_avg_sq.any() and not ex.steps.any()


def _reference_step(scene, cams, gts, bg, table, pipe, env, indices):
    """One step the hand-written way: render_raw + exposure.apply + fused_l1_ssim + backward() per view.  Returns (the model with its
    gradient bucket, the views' losses, the views' table gradients [B, 12])."""
    from fdgs import exposure
    from fdgs.fused import render_raw
    from fdgs.loss import fused_l1_ssim
    ma = _model(scene, bg.device, env)
    sink = ma.grad_sink()
    tab = table.clone().requires_grad_(True)
    losses, slots = [], []
    for b in range(B):
        tab.grad = None
        img = render_raw(cams[b], ma, pipe, bg, grad_sink=sink, accumulate=b > 0)["render"]
        loss = fused_l1_ssim(exposure.apply(img, tab, indices[b]), gts[b], 0.2)
        (loss / B).backward()
        losses.append(float(loss.detach()))
        slots.append(tab.grad[indices[b]].clone())
        assert int(tab.grad.abs().sum(dim=1).count_nonzero()) == 1
    torch.cuda.synchronize()
    return ma, losses, torch.stack(slots)


def _pipeline_steps(scene, cams, gts, bg, table, pipe, env, indices, steps=1, lr=1e-3, **kw):
    from fdgs import train_host
    from fdgs.pipeline import StepPipeline
    mp = _model(scene, bg.device, env)
    ex = _exposure(bg.device, table, lr=lr)
    sp = StepPipeline(mp, train_host.make_optimizer(mp), world_size=1, lambda_dssim=0.2, exposure=ex, **kw)
    losses, tables, slots = [], [], []
    for _ in range(steps):
        res, ls = sp.step(cams, gts, pipe, bg, camera_indices=indices)
        losses += [float(l) for l in ls]
        tables.append(ex.table.clone())
        slots.append(sp._bufs["exp_slots"].clone())
    torch.cuda.synchronize()
    assert all(r["render"].shape == r["render_uncorrected"].shape == (3, scene["H"], scene["W"]) for r in res)
    return mp, sp, ex, losses, tables, slots


def _check_against_reference(ref, run, table, indices):
    """The first step of ``run`` against the hand-written step: losses, the views' slots, the Gaussians' gradient bucket (below the SH
    segment where the fused SH update leaves that out of the bucket), and the table against the oracle's Adam from the slots."""
    ma, ref_losses, ref_slots = ref
    mp, sp, ex, losses, tables, slots = run
    np.testing.assert_allclose(losses[:B], ref_losses, rtol=3e-5, atol=1e-6)
    _close_grads(slots[0], ref_slots)
    if len(tables) == 1:
        n_cmp = mp.offsets["_features"][0] if sp.fuse_sh_adam else mp.flat.numel()
        _close_grads(mp.flat_grad[:n_cmp], ma.flat_grad[:n_cmp])
    N = table.shape[0]
    want = eo.adam(table.cpu().numpy(), np.zeros((N, 12)), np.zeros((N, 12)), np.zeros(N, np.int64), indices, slots[0].cpu().numpy(), lr=1e-3)
    got = tables[0].cpu().numpy()
    bar = 4 * np.spacing(np.abs(want[0]).astype(np.float32)).astype(np.float64)
    assert (np.abs(got - want[0]) <= bar).all()
    others = [i for i in range(N) if i not in indices]
    assert np.array_equal(got[others], table.cpu().numpy()[others]) and ex.steps.tolist() == [len(tables) * int(i in indices) for i in range(N)]


@pytest.mark.parametrize("variant", ["views", "batched", "waiting", "envmap", "twice"])
def test_one_step_is_the_hand_written_step(variant, gpu_device):
    """(b), (c): a random table, one step.  Variants: the per-view step, _step_batched (sh_group=2), lazy=False, with an environment
    map, and a camera that two views share.  The variant run a second time leaves the same table bit for bit."""
    scene, cams, gts, bg = _setup(gpu_device)
    table = _random_table(gpu_device)
    env = variant == "envmap"
    pipe = Pipe(ENV[0] if env else 0)
    indices = [2, 0, 2] if variant == "twice" else [1, 2, 0]
    kw = {"batched": {"sh_group": 2}, "waiting": {"lazy": False}}.get(variant, {})
    ref = _reference_step(scene, cams, gts, bg, table, pipe, env, indices)
    run = _pipeline_steps(scene, cams, gts, bg, table, pipe, env, indices, **kw)
    _check_against_reference(ref, run, table, indices)
    again = _pipeline_steps(scene, cams, gts, bg, table, pipe, env, indices, **kw)
    assert torch.equal(again[4][0].view(torch.int32), run[4][0].view(torch.int32))
    assert torch.equal(again[5][0].view(torch.int32), run[5][0].view(torch.int32))
    if variant == "waiting":     # ... and the lazy step's
        lazy = _pipeline_steps(scene, cams, gts, bg, table, pipe, env, indices)
        assert torch.equal(lazy[4][0].view(torch.int32), run[4][0].view(torch.int32))


def test_overlap_steps_follows_the_plain_pipeline(gpu_device):
    """(c) overlap_steps over 4 steps against the plain pipeline: the first step (identical inputs) against the hand-written one with
    the same table bit for bit in both runs; the later steps read Gaussians that carry the float-atomics noise of the steps before,
    so losses and parameters follow under the two-pipeline comparator and the table to Adam's reach on a gradient whose sign that noise
    may turn: 2 lr per step after the first."""
    scene, cams, gts, bg = _setup(gpu_device)
    table = _random_table(gpu_device)
    indices, steps, lr = [1, 2, 0], 4, 1e-3
    ref = _reference_step(scene, cams, gts, bg, table, Pipe(), False, indices)
    plain = _pipeline_steps(scene, cams, gts, bg, table, Pipe(), False, indices, steps=steps)
    over = _pipeline_steps(scene, cams, gts, bg, table, Pipe(), False, indices, steps=steps, overlap_steps=True)
    assert over[1].overlap_steps and over[1].steps_carried == steps - 1 and plain[1].steps_carried == 0
    for run in (plain, over):
        _check_against_reference(ref, run, table, indices)
    assert torch.equal(over[4][0].view(torch.int32), plain[4][0].view(torch.int32))
    np.testing.assert_allclose(over[3], plain[3], rtol=1e-4, atol=1e-6)
    _close_params(over[0].flat, plain[0].flat)
    terr = (over[4][-1] - plain[4][-1]).abs()
    print("table after %d steps: worst difference %.3e, different bits in %d of %d" % (
        steps, terr.max().item(), int((over[4][-1].view(torch.int32) != plain[4][-1].view(torch.int32)).sum()), terr.numel()))
    assert terr.max().item() <= 2 * lr * (steps - 1) + 1e-6
    assert ((plain[4][-1] - table).abs()[:B].amax(dim=1) > lr).all()     # every camera's row has moved, step after step


def test_known_gains_pull_the_rows_their_way(gpu_device):
    """(d) the model that rendered the ground truth, frames multiplied by 0.6, 1.0 and 1.4, 30 steps at lr 1e-3: a gradient of
    constant sign moves Adam by about lr per step, so the diagonals of the 0.6 row end below 1 and those of the 1.4 row above 1 by at
    least a third of 30 lr."""
    from fdgs import train_host
    from fdgs.fused import render_raw
    from fdgs.pipeline import StepPipeline
    scene, cams, _gts, bg = _setup(gpu_device)
    gains, steps, lr = (0.6, 1.0, 1.4), 30, 1e-3
    m = _model(scene, gpu_device)
    with torch.no_grad():
        gts = [(render_raw(c, m, Pipe(), bg)["render"] * g).contiguous() for c, g in zip(cams, gains)]
    ex = _exposure(gpu_device, lr=lr)
    sp = StepPipeline(m, train_host.make_optimizer(m), world_size=1, lambda_dssim=0.2, exposure=ex)
    for _ in range(steps):
        sp.step(cams, gts, Pipe(), bg)
    torch.cuda.synchronize()
    diag = ex.table.cpu().numpy().reshape(-1, 3, 4)[:, [0, 1, 2], [0, 1, 2]]
    print("diagonals after %d steps:\n%s" % (steps, diag))
    assert (diag[0] <= 1.0 - steps * lr / 3).all() and (diag[2] >= 1.0 + steps * lr / 3).all()
    assert ex.steps.tolist() == [steps] * B + [0] and np.array_equal(diag[3], np.ones(3, np.float32))


def test_two_ranks_are_refused(gpu_device):
    """(e)"""
    from fdgs import train_host
    from fdgs.pipeline import StepPipeline
    scene, _cams, _gts, _bg = _setup(gpu_device)
    m = _model(scene, gpu_device)
    with pytest.raises(NotImplementedError, match="one rank"):
        StepPipeline(m, train_host.make_optimizer(m), world_size=2, exposure=_exposure(gpu_device))
    sp = StepPipeline(m, train_host.make_optimizer(m), world_size=1, exposure=_exposure(gpu_device))
    with pytest.raises(ValueError, match="camera_indices"):
        sp.step(_cams, _gts, Pipe(), _bg, camera_indices=[0, 1])
    with pytest.raises(ValueError, match="camera_indices"):
        sp.step(_cams, _gts, Pipe(), _bg, camera_indices=[0, 1, B + 1])


def test_held_out_views_are_aligned_before_the_metrics(gpu_device):
    """(f) frames that are an exact affine map of the clamped renders: the oracle's fit undoes the map (PSNR limited by the ridge
    alone), so on the oracle psnr_cc - psnr >= 20 dB with room -- asserted -- and evaluate_corrected reports the same."""
    from fdgs import exposure, metrics
    from fdgs.fused import render_raw
    scene, cams, _gts, bg = _setup(gpu_device)
    m = _model(scene, gpu_device)
    rows = [np.array([0.7, 0.05, 0, 0.02, 0, 0.6, 0.1, 0.05, 0.05, 0, 0.8, 0.0]), np.array([0.5, 0, 0, 0.2, 0, 0.5, 0, 0.2, 0, 0, 0.5, 0.2]),
            np.array([1.1, 0, 0, -0.05, 0, 1.2, 0, -0.05, 0, 0, 0.9, 0.02])]
    renders, gts, margin = [], [], []
    with torch.no_grad():
        for c, A in zip(cams, rows):
            r = np.clip(render_raw(c, m, Pipe(), bg)["render"].cpu().numpy(), 0.0, 1.0)
            gt = eo.apply(r, A).astype(np.float32)
            fit = eo.fit_affine(r, gt, 1e-6, clamp=True)
            raw, cc = eo.psnr(r, gt), eo.psnr(eo.apply(r, fit), gt)
            print("oracle: psnr %.2f dB, after the fit %.2f dB" % (raw, cc))
            assert cc - raw >= 25.0
            margin.append((raw, cc))
            renders.append(r)
            gts.append(torch.from_numpy(gt).to(gpu_device))
    out = exposure.evaluate_corrected(m, cams, gts, Pipe(), bg, msssim=False)
    plain = metrics.evaluate(m, cams, gts, Pipe(), bg, msssim=False)
    assert set(out) == set(plain) | {k + "_cc" for k in plain if k != "views"} | {"fits"}
    for k in ("l1", "psnr", "ssim"):
        assert out[k] == plain[k]
    assert torch.equal(out["rows"][:, :3], plain["rows"][:, :3])
    print("psnr %.2f dB, psnr_cc %.2f dB" % (out["psnr"], out["psnr_cc"]))
    assert abs(out["psnr"] - np.mean([a for a, _ in margin])) <= 1e-2
    assert out["psnr_cc"] >= out["psnr"] + 20.0 and out["l1_cc"] < out["l1"] and out["ssim_cc"] > out["ssim"]
    assert out["views"] == B and tuple(out["fits"].shape) == (B, 12) and tuple(out["rows_cc"].shape) == (B, 4)
    for v in range(B):
        want = eo.fit_affine(renders[v], gts[v].cpu().numpy(), 1e-6, clamp=True)
        assert np.abs(out["fits"][v].numpy() - want).max() <= 1e-4
