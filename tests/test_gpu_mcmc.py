"""GPU: fdgs.mcmc (csrc/mcmc.hip) against the float64 / Python-int restatement of tests/mcmc_oracle.py: the fixed-point sampler bit
for bit, relocate / grow, the noise step, the regularisers, the StepPipeline hook and a short run to a cap."""
import numpy as np
import pytest
import torch

import mcmc_cases as mc
import mcmc_oracle as mo
from util import synth

pytestmark = pytest.mark.gpu
MODES = tuple(mc.MODES)
SCALE_NAMES = ("_scaling", "_scaling_t")


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


# ---- sampling ----
@pytest.mark.parametrize("P", mc.SAMPLE_SIZES)
def test_weights_prefix_sums_and_draws(gpu_device, P):
    """wq within 2 units of rint(o 2^24) in float64; given the kernel's own wq, everything downstream bit for bit."""
    from fdgs import mcmc
    worst = 0
    for name, (o, min_opacity) in mc.opacity_patterns(P, seed=P).items():
        raw = torch.from_numpy(mc.logit(o).astype(np.float32)).to(gpu_device)
        alive, wq, prefix = mcmc.weights(raw, min_opacity)
        wq_k, want = _u32(wq).astype(np.int64), mo.weights_f64(raw.cpu().numpy(), min_opacity).astype(np.int64)
        worst = max(worst, int(np.abs(wq_k - want).max()))
        assert np.abs(wq_k - want).max() <= 2, (name, np.abs(wq_k - want).max())
        assert np.array_equal(alive.cpu().numpy() != 0, wq_k > 0) or min_opacity == 0.0
        ref_prefix = mo.prefix_of(wq_k.astype(np.uint64))
        assert np.array_equal(_u64(prefix), ref_prefix), name
        for n in sorted({1, max(1, P // 2), 3 * P}):
            source, counts, words = mcmc.draw(prefix, n, seed=0x1234567890ABCDEF, stream_id=3, call=(1 << 32) + 7, return_words=True)
            s_ref, c_ref, w_ref = mo.draw(ref_prefix, n, 0x1234567890ABCDEF, 3, (1 << 32) + 7)
            assert np.array_equal(_u32(words), w_ref), (name, n)
            assert np.array_equal(source.cpu().numpy(), s_ref), (name, n)
            assert np.array_equal(counts.cpu().numpy(), c_ref), (name, n)
            assert (wq_k[s_ref] > 0).all()
        if name == "one-alive":
            assert set(s_ref.tolist()) == {P // 2}
    print("P=%d worst |wq - rint(o 2^24)| = %d units" % (P, worst))


# ---- relocate ----
RELOCATE_CASES = {   # name -> (P, dead fraction or count of alive, M)
    "half-dead": (600, 0.5, 16), "more-dead-than-alive": (600, 0.8, 16), "one-alive": (120, "one", 16), "m1": (300, 0.5, 1), "m48": (300, 0.5, 48),
}


def _opacities(P, spec, seed):
    rng = np.random.default_rng(seed)
    o = rng.uniform(0.02, 0.99, P)
    if spec == "one":
        o[:] = rng.uniform(1e-4, 0.004, P)
        o[P // 3] = 0.7
    else:
        dead = rng.permutation(P)[:int(spec * P)]
        o[dead] = rng.uniform(1e-4, 0.004, len(dead))
    return o


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(RELOCATE_CASES))
def test_relocate(gpu_device, mode, case):
    from fdgs import layout, mcmc
    P, spec, M = RELOCATE_CASES[case]
    model, opt = mc.make_model(gpu_device, P, mode, M=M, seed=11, opacity=_opacities(P, spec, 5))
    before = mc.as_numpy(model)
    m0, v0, flat_ptr = opt.exp_avg.clone(), opt.exp_avg_sq.clone(), model.flat.data_ptr()
    _alive, wq, _prefix = mcmc.weights(model._opacity, 0.005)
    wq_k = _u32(wq).astype(np.uint64)
    dead = np.flatnonzero(wq_k == 0)
    source, counts, _ = mo.draw(mo.prefix_of(wq_k), len(dead), seed=42, stream_id=mo.STREAM_RELOCATE, call=6)
    version = model.flat._version
    out = mcmc.relocate(model, opt, seed=42, call=6)
    after = mc.as_numpy(model)
    assert out["drew"] and out["relocated"] == len(dead) and out["dead"] == len(dead) and out["sources"] == int((counts > 0).sum())
    assert model.P == P and model.flat.data_ptr() == flat_ptr and model.flat._version > version
    N = mo.multiplicity(counts)
    if case == "one-alive":
        assert counts.max() == P - 1 > 51 and N.max() == 51       # the clamp
    srcs = np.flatnonzero(counts > 0)
    touched = np.zeros(P, bool)
    touched[srcs] = touched[dead] = True
    # copied segments: bit-equal to the source's old rows (opacity and scales are updated afterwards)
    for name in model.NAMES:
        if name in ("_opacity",) + SCALE_NAMES[:1] or (name == "_scaling_t" and model.gaussian_dim == 4):
            continue
        assert np.array_equal(after[name][dead].view(np.uint32), before[name][source].view(np.uint32)), name
        assert np.array_equal(after[name][~touched].view(np.uint32), before[name][~touched].view(np.uint32)), name
        assert np.array_equal(after[name][srcs].view(np.uint32), before[name][srcs].view(np.uint32)), name
    for name in ("_opacity", "_scaling", "_scaling_t"):
        assert np.array_equal(after[name][~touched].view(np.uint32), before[name][~touched].view(np.uint32)), name
    # opacity and scales of sources and copies against the oracle, on the activated values
    worst = [0.0]
    rows = list(srcs) + list(dead)
    of = [(s, N[s]) for s in srcs] + [(s, N[s]) for s in source]
    four = model.gaussian_dim == 4
    for r, (src, n) in zip(rows, of):
        o_new, s_new = mo.updated(before["_opacity"][src, 0], np.concatenate([before["_scaling"][src], before["_scaling_t"][src]]), n)
        got_o = float(mo.sigmoid(after["_opacity"][r, 0]))
        got_s = np.exp(np.concatenate([after["_scaling"][r], after["_scaling_t"][r]]).astype(np.float64))
        k = 4 if four else 3
        err = max([abs(got_o - o_new) / o_new] + list(np.abs(got_s[:k] - s_new[:k]) / s_new[:k]))
        worst[0] = max(worst[0], err)
        assert err <= 1e-6, (r, src, n, err)
        assert got_o > 0.005 or np.float32(got_o) > np.float32(0.005)
    print("relocate %s %s: worst relative error of new opacity / scales %.3e (bar 1e-6)" % (mode, case, worst[0]))
    # moments: zero in every segment of every source and relocated row, bit-identical elsewhere
    for buf, old in ((opt.exp_avg, m0), (opt.exp_avg_sq, v0)):
        for name in model.NAMES:
            got, was = layout.segment(buf, model, name).cpu().numpy().reshape(P, -1), layout.segment(old, model, name).cpu().numpy().reshape(P, -1)
            assert not got[touched].any(), name
            assert np.array_equal(got[~touched].view(np.uint32), was[~touched].view(np.uint32)), name
    # right after a relocation nothing is dead
    alive, _, _ = mcmc.weights(model._opacity, 0.005)
    assert bool(alive.all())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", ["none-dead", "none-alive"])
def test_relocate_noop_touches_nothing(gpu_device, mode, case):
    from fdgs import mcmc
    P = 300
    o = np.random.default_rng(2).uniform(0.02, 0.9, P) if case == "none-dead" else np.full(P, 0.002)
    model, opt = mc.make_model(gpu_device, P, mode, seed=3, opacity=o)
    flat, m0, v0, version = model.flat.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), model.flat._version
    out = mcmc.relocate(model, opt, seed=1, call=0)
    assert not out["drew"] and out["relocated"] == 0 and out["dead"] == (0 if case == "none-dead" else P)
    for got, was in ((model.flat, flat), (opt.exp_avg, m0), (opt.exp_avg_sq, v0)):
        assert torch.equal(got.view(torch.int32), was.view(torch.int32))
    assert model.flat._version == version
    s = mcmc.MCMCStrategy(model, opt, cap=P)
    s.refine()
    assert s.call == 0 and torch.equal(model.flat.view(torch.int32), flat.view(torch.int32))


# ---- grow ----
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cap,P_new", [(5000, 1050), (1020, 1020)])
def test_grow(gpu_device, mode, cap, P_new):
    from fdgs import layout, mcmc
    P = 1000
    model, opt = mc.make_model(gpu_device, P, mode, seed=21, opacity=_opacities(P, 0.1, 8))
    before = mc.as_numpy(model)
    old_moments = {n: (layout.segment(opt.exp_avg, model, n).cpu().numpy().reshape(P, -1), layout.segment(opt.exp_avg_sq, model, n).cpu().numpy().reshape(P, -1))
                   for n in model.NAMES}
    _alive, wq, _ = mcmc.weights(model._opacity, 0.005)
    source, counts, _ = mo.draw(mo.prefix_of(_u32(wq).astype(np.uint64)), P_new - P, seed=5, stream_id=mo.STREAM_GROW, call=9)
    out = mcmc.grow(model, opt, cap, seed=5, call=9)
    assert out == {"P_old": P, "P_new": P_new, "added": P_new - P, "sources": int((counts > 0).sum()), "drew": True} and model.P == P_new
    after = mc.as_numpy(model)
    N, srcs = mo.multiplicity(counts), np.flatnonzero(counts > 0)
    plain = np.ones(P, bool)
    plain[srcs] = False
    updated_names = ("_opacity", "_scaling") + (("_scaling_t",) if model.gaussian_dim == 4 else ())
    for name in model.NAMES:
        assert after[name].shape[0] == P_new
        if name not in updated_names:
            assert np.array_equal(after[name][:P].view(np.uint32), before[name].view(np.uint32)), name
            assert np.array_equal(after[name][P:].view(np.uint32), before[name][source].view(np.uint32)), name
        else:
            assert np.array_equal(after[name][:P][plain].view(np.uint32), before[name][plain].view(np.uint32)), name
    k = 4 if model.gaussian_dim == 4 else 3
    for r, src in list(zip(srcs, srcs)) + list(zip(range(P, P_new), source)):
        o_new, s_new = mo.updated(before["_opacity"][src, 0], np.concatenate([before["_scaling"][src], before["_scaling_t"][src]]), N[src])
        got_s = np.exp(np.concatenate([after["_scaling"][r], after["_scaling_t"][r]]).astype(np.float64))
        err = max([abs(float(mo.sigmoid(after["_opacity"][r, 0])) - o_new) / o_new] + list(np.abs(got_s[:k] - s_new[:k]) / s_new[:k]))
        assert err <= 1e-6, (r, src, err)
    # old rows carry their moments (the sources': zero), new rows start from zero
    for name in model.NAMES:
        for buf, was in zip((opt.exp_avg, opt.exp_avg_sq), old_moments[name]):
            got = layout.segment(buf, model, name).cpu().numpy().reshape(P_new, -1)
            assert np.array_equal(got[:P][plain].view(np.uint32), was[plain].view(np.uint32)), name
            assert not got[:P][~plain].any() and not got[P:].any(), name
    # the optimizer's segment table is valid: one Adam step against the torch formulation
    g = torch.Generator(device="cpu").manual_seed(1)
    model.flat_grad.copy_(torch.randn(model.flat_grad.shape, generator=g))
    flat_before_step = model.flat.detach().cpu().clone()
    from fdgs import train_host
    twin = train_host.GaussianParams.empty(P_new, model.M, "cpu").apply_settings(**model.settings())
    twin._bind(model.flat.detach().cpu().clone(), model.flat_grad.cpu().clone(), P_new)
    twin_opt = train_host.FlatAdam(twin)
    twin_opt.rebind(opt.exp_avg.cpu().clone(), opt.exp_avg_sq.cpu().clone())
    opt.step()
    twin_opt.step()
    # two float32 evaluations of one step; the first step's bias correction 1 - 0.999 carries 1.3e-5 relative in float32, half of it
    # after the square root, on a step of at most lr / 0.1 * |m| / denom = 0.15 here: 1e-6
    assert opt.step_count == 1 and torch.allclose(model.flat.detach().cpu(), twin.flat.detach(), rtol=1e-5, atol=2e-6)
    assert not torch.equal(model.flat.detach().cpu(), flat_before_step)


def test_grow_at_the_cap_touches_nothing(gpu_device):
    from fdgs import mcmc
    model, opt = mc.make_model(gpu_device, 1000, "rot4d", seed=4)
    flat, ptr, m_ptr = model.flat.clone(), model.flat.data_ptr(), opt.exp_avg.data_ptr()
    out = mcmc.grow(model, opt, 1000, seed=5, call=0)
    assert not out["drew"] and out["P_new"] == 1000 and model.P == 1000
    assert model.flat.data_ptr() == ptr and opt.exp_avg.data_ptr() == m_ptr and torch.equal(model.flat.view(torch.int32), flat.view(torch.int32))
    assert mcmc.grow(model, opt, 900, seed=5, call=0)["added"] == 0 and model.flat.data_ptr() == ptr


# ---- the noise step ----
def _noise_model(dev, P, mode, seed):
    rng = np.random.default_rng(seed)
    o = rng.uniform(1e-4, 0.02, P)       # around the gate's centre at 0.005
    return mc.make_model(dev, P, mode, seed=seed, opacity=o, moments=False)


@pytest.mark.parametrize("P", [1, 65, 5000])
@pytest.mark.parametrize("mode", MODES)
def test_noise_step_with_injected_normals(gpu_device, mode, P):
    """delta within 1e-5 max(1, |delta_oracle|), |.| the Euclidean norm of the Gaussian's step: raw quaternions of any norm, scales
    from e^-6 to e^2 in one Gaussian."""
    from fdgs import mcmc
    model, _ = _noise_model(gpu_device, P, mode, seed=P + 1)
    before = mc.as_numpy(model)
    xi = torch.randn((P, 4 if model.gaussian_dim == 4 else 3), generator=torch.Generator().manual_seed(P)).to(gpu_device)
    lr_xyz, noise_lr = 1.6e-4, 5e5
    version = model.flat._version
    mcmc.noise_step(model, lr_xyz, noise_lr, xi=xi)
    assert model.flat._version > version
    after = mc.as_numpy(model)
    scale = float(np.float32(noise_lr * lr_xyz))
    want = mo.noise_delta(before, xi.cpu().numpy(), scale)
    got = after["_xyz"].astype(np.float64) - before["_xyz"].astype(np.float64)
    if model.gaussian_dim == 4:
        got = np.concatenate([got, after["_t"].astype(np.float64) - before["_t"].astype(np.float64)], 1)
    else:
        assert np.array_equal(after["_t"].view(np.uint32), before["_t"].view(np.uint32))
    # the parameters are float32: the step is read back through one rounding of position + step
    pos = np.concatenate([before["_xyz"], before["_t"]], 1)[:, :got.shape[1]].astype(np.float64)
    rounding = np.abs(pos + want) * 2.0 ** -24
    bar = 1e-5 * np.maximum(1.0, np.linalg.norm(want, axis=1, keepdims=True))
    err = np.abs(got - want)
    print("noise %s P=%d: worst err / bar %.3f (err %.3e), largest |delta| %.3e" % (mode, P, (err / (bar + rounding)).max(), err.max(), np.abs(want).max()))
    assert (err <= bar + rounding).all()
    for name in model.NAMES:
        if name not in ("_xyz", "_t"):
            assert np.array_equal(after[name].view(np.uint32), before[name].view(np.uint32)), name


@pytest.mark.parametrize("mode", MODES)
def test_noise_gate(gpu_device, mode):
    """At o = 0.9 nothing moves (below 1e-30); at o = 0.004 the gate is at least half open."""
    from fdgs import mcmc
    P = 257
    for o, lo in ((0.9, None), (0.004, 0.5)):
        model, _ = mc.make_model(gpu_device, P, mode, seed=9, opacity=np.full(P, o), scale_range=(-1.0, 0.0), moments=False)
        before = mc.as_numpy(model)
        xi = torch.randn((P, 4), generator=torch.Generator().manual_seed(1)).to(gpu_device)
        mcmc.noise_step(model, 1.6e-4, 5e5, xi=xi)
        after = mc.as_numpy(model)
        moved = np.abs(after["_xyz"].astype(np.float64) - before["_xyz"])
        if lo is None:
            assert moved.max() < 1e-30 and np.array_equal(after["_t"].view(np.uint32), before["_t"].view(np.uint32))
        else:
            open_ = mo.noise_delta(before, xi.cpu().numpy(), 80.0)[:, :3] / mo.gate(mo.sigmoid(before["_opacity"]))
            big = np.abs(open_) > 1e-2
            ratio = (after["_xyz"].astype(np.float64) - before["_xyz"])[big] / open_[big]
            assert mo.gate(np.float64(0.004)) >= 0.5 and (ratio >= 0.5 * (1 - 1e-3)).all() and (ratio <= 0.56).all()


@pytest.mark.parametrize("P", [1, 65, 5000])
def test_noise_step_generator(gpu_device, P):
    """The Philox words bit for bit; xi within 1e-5 of float64 Box-Muller on the same words; the step taken is the injected one's."""
    from fdgs import mcmc
    seed, call = 0xDEADBEEF12345678, (3 << 32) + 11
    model, _ = _noise_model(gpu_device, P, "rot4d", seed=7)
    twin, _ = _noise_model(gpu_device, P, "rot4d", seed=7)
    out = mcmc.noise_step(model, 1.6e-4, 5e5, seed=seed, call=call, return_xi=True, return_words=True)
    words = mo.philox_words(P, seed, mo.STREAM_NOISE, call)
    assert np.array_equal(_u32(out["words"]), words)
    xi_ref = mo.box_muller(words)
    err = np.abs(out["xi"].cpu().numpy().astype(np.float64) - xi_ref).max()
    print("generator P=%d: worst |xi - float64 Box-Muller| %.3e (bar 1e-5), largest |xi| %.2f" % (P, err, np.abs(xi_ref).max()))
    assert err <= 1e-5 and np.isfinite(xi_ref).all()
    mcmc.noise_step(twin, 1.6e-4, 5e5, xi=out["xi"])
    assert torch.equal(model.flat.view(torch.int32), twin.flat.view(torch.int32))
    other, _ = _noise_model(gpu_device, P, "rot4d", seed=7)
    o2 = mcmc.noise_step(other, 1.6e-4, 5e5, seed=seed, call=call + 1, return_xi=True)
    assert not torch.equal(o2["xi"], out["xi"])


# ---- the regularisers ----
@pytest.mark.parametrize("P", [1, 257, 5000])
@pytest.mark.parametrize("lam_st", [0.0, 0.02])
def test_regularizer(gpu_device, P, lam_st):
    from fdgs import mcmc
    rng = np.random.default_rng(P)
    o = np.concatenate([rng.uniform(1e-6, 1 - 1e-6, P - P // 2), 1.0 - 2.0 ** -rng.uniform(10, 23, P // 2)])
    model, _ = mc.make_model(gpu_device, P, "rot4d", seed=3, opacity=o, moments=False)
    lam_o, lam_s = 0.01, 0.02
    raw = mc.as_numpy(model)
    terms_ref, g_o, g_s, g_st = mo.regularizer(raw["_opacity"], raw["_scaling"], raw["_scaling_t"], lam_o, lam_s, lam_st)
    sink = model.grad_sink()
    model.flat_grad.zero_()
    terms = mcmc.regularize(model, sink, lam_o, lam_s, lam_st)
    got = {k: sink[k].cpu().numpy().astype(np.float64).reshape(P, -1) for k in ("dL_dopacity", "dL_dscales", "dL_dscales_t")}
    for k, want in (("dL_dopacity", g_o.reshape(P, 1)), ("dL_dscales", g_s), ("dL_dscales_t", g_st.reshape(P, 1))):
        if k == "dL_dscales_t" and lam_st == 0.0:
            assert not got[k].any()
            continue
        rel = np.abs(got[k] - want) / np.abs(want)
        assert rel.max() <= 1e-6, (k, rel.max())
    np.testing.assert_allclose(terms.cpu().numpy(), terms_ref, rtol=1e-6, atol=0)
    for k in ("dL_dopacity", "dL_dscales", "dL_dscales_t"):
        sink[k].zero_()
    assert not model.flat_grad.any()       # nothing but the three sinks was written
    # added into a non-zero sink, not written over it: bit-equal to sink + the gradient just measured, one float32 addition
    base = torch.randn(model.flat_grad.shape, generator=torch.Generator().manual_seed(2)).to(gpu_device)
    model.flat_grad.copy_(base)
    terms2 = mcmc.regularize(model, sink, lam_o, lam_s, lam_st)
    want = base.clone()
    for k in ("dL_dopacity", "dL_dscales", "dL_dscales_t"):
        b, e = model.offsets[{"dL_dopacity": "_opacity", "dL_dscales": "_scaling", "dL_dscales_t": "_scaling_t"}[k]]
        want[b:e] += torch.from_numpy(got[k].astype(np.float32).reshape(-1)).to(gpu_device)
    assert torch.equal(model.flat_grad.view(torch.int32), want.view(torch.int32)) and torch.equal(terms2, terms)


# ---- determinism ----
def _sequence(dev, seed):
    from fdgs import mcmc
    model, opt = mc.make_model(dev, 1500, "rot4d", seed=13, opacity=_opacities(1500, 0.3, 4), scale_range=(-4.0, -1.0))
    s = mcmc.MCMCStrategy(model, opt, cap=1700, seed=seed)
    log = []
    for _ in range(3):
        log.append(s.refine())
        s.after_step(1.6e-4)
        with torch.no_grad():
            model._opacity[::7] -= 3.0       # some die again
    return model, opt, s, log


def test_same_seed_same_bits_other_seed_other_draws(gpu_device):
    a, b, c = _sequence(gpu_device, 5), _sequence(gpu_device, 5), _sequence(gpu_device, 6)
    assert a[0].P == b[0].P == 1700 and a[3] == b[3] and a[2].state_dict() == b[2].state_dict() == {"seed": 5, "call": a[2].call}
    assert torch.equal(a[0].flat.view(torch.int32), b[0].flat.view(torch.int32))
    assert torch.equal(a[1].exp_avg.view(torch.int32), b[1].exp_avg.view(torch.int32))
    assert a[2].call >= 6 and not torch.equal(a[0].flat, c[0].flat)


# ---- the StepPipeline hook ----
def _views(dev, B, P=2000):
    from fdgs import train_host
    cfg = synth.SceneConfig("mcmc", P, 160, 128, 2, 1, 0.04, 10.0, True, 4, False)
    scene = synth.make_scene(cfg, seed=4)
    cams = [train_host.SyntheticCamera(scene, dev, timestamp=(b + 0.5) / B * scene["time_duration"]) for b in range(B)]
    gen = torch.Generator(device="cpu").manual_seed(7)
    gts = [torch.rand(3, scene["H"], scene["W"], generator=gen).to(dev) for _ in range(B)]
    return scene, cams, gts, train_host.PipelineFlags(), torch.tensor([0.1, 0.2, 0.3], device=dev)


# weights at which the regularisers' gradient (lambda / P per Gaussian) stands well above the bars below: a hook that did not run, ran
# twice or ran after the geometry Adam cannot pass
HOOK_LAMBDAS = dict(lambda_opacity=2000.0, lambda_scale=2000.0, lambda_scale_t=500.0)


@pytest.mark.parametrize("overlap", [False, True], ids=["one-stream", "two-streams"])
@pytest.mark.parametrize("B", [1, 3])
def test_pipeline_hook_matches_the_gradient_added_by_hand(gpu_device, B, overlap):
    from fdgs import mcmc, train_host
    from fdgs.fused import render_raw
    from fdgs.loss import fused_l1_ssim
    from fdgs.pipeline import StepPipeline
    scene, cams, gts, pipe, bg = _views(gpu_device, B)
    steps = 2
    # by hand: render_raw + fused loss per view on one stream, then the regularisers into the bucket, then Adam
    ma = train_host.GaussianParams(scene, gpu_device)
    oa = train_host.make_optimizer(ma)
    sa = mcmc.MCMCStrategy(ma, oa, cap=ma.P, **HOOK_LAMBDAS)
    sink, ref_losses, ref_grads = ma.grad_sink(), [], []
    for _ in range(steps):
        for b in range(B):
            pkg = render_raw(cams[b], ma, pipe, bg, grad_sink=sink, accumulate=b > 0)
            l1s = fused_l1_ssim(pkg["render"], gts[b], 0.2)
            (l1s / B).backward()
            ref_losses.append(float(l1s.detach()))
        sa.add_regularizer_grads()
        ref_grads.append(ma.flat_grad.clone())
        oa.step()
    mp = train_host.GaussianParams(scene, gpu_device)
    op = train_host.make_optimizer(mp)
    sp_ = mcmc.MCMCStrategy(mp, op, cap=mp.P, **HOOK_LAMBDAS)
    sp = StepPipeline(mp, op, world_size=1, lambda_dssim=0.2, overlap=overlap, grad_terms=[sp_.add_regularizer_grads])
    got_losses, got_grads = [], []
    for _ in range(steps):
        _res, ls = sp.step(cams, gts, pipe, bg)
        got_losses += [float(l) for l in ls]
        torch.cuda.synchronize()
        got_grads.append(mp.flat_grad.clone())
    np.testing.assert_allclose(got_losses, ref_losses, rtol=3e-5, atol=1e-6)
    n_cmp = mp.offsets["_features"][0]         # (the fused SH update does not materialise _features.grad)
    for name in ("_opacity", "_scaling", "_scaling_t"):
        b, e = mp.offsets[name]
        reg = (HOOK_LAMBDAS["lambda_scale_t" if name == "_scaling_t" else "lambda_scale" if name == "_scaling" else "lambda_opacity"]
               / mp.P / (3 if name == "_scaling" else 1))
        gerr = (got_grads[0][b:e] - ref_grads[0][b:e]).abs().max().item()
        assert reg > 0.1 and gerr <= 1e-3 * max(1e-6, ref_grads[0][:n_cmp].abs().max().item()), (name, gerr)
    # the bars of tests/test_gpu_api.py::test_step_pipeline_matches_autograd_step (float atomics in the blend backward)
    gerr = (got_grads[0][:n_cmp] - ref_grads[0][:n_cmp]).abs().max().item()
    assert gerr <= 1e-3 * max(1e-6, ref_grads[0].abs().max().item())
    perr = (mp.flat - ma.flat).abs()
    assert (perr > 2e-3).float().mean().item() <= 2e-3 and perr.max().item() <= 0.25, ((perr > 2e-3).float().mean().item(), perr.max().item())
    # and the hook is what made the difference: without it the same step leaves another opacity gradient
    mq = train_host.GaussianParams(scene, gpu_device)
    StepPipeline(mq, train_host.make_optimizer(mq), world_size=1, lambda_dssim=0.2, overlap=overlap).step(cams, gts, pipe, bg)
    torch.cuda.synchronize()
    b, e = mp.offsets["_opacity"]
    raw = mc.as_numpy(train_host.GaussianParams(scene, gpu_device))
    _t, g_o, _gs, _gst = mo.regularizer(raw["_opacity"], raw["_scaling"], raw["_scaling_t"], *HOOK_LAMBDAS.values())
    diff = (got_grads[0][b:e] - mq.flat_grad[b:e]).double().cpu().numpy()
    assert np.abs(diff - g_o).max() <= 1e-3 * np.abs(g_o).max() + 1e-3 * mq.flat_grad[b:e].abs().max().item()
    assert np.isclose(float(sp_.last_terms[0]), float(sa.last_terms[0]), rtol=1e-3)


def test_pipeline_without_grad_terms_is_the_plain_pipeline(gpu_device):
    """grad_terms=None launches exactly what a pipeline built without the keyword launches.  The first step's images and losses (a
    forward on identical inputs: no float atomics) are bit-identical; the parameters after 3 steps are bit-identical wherever two runs
    of the plain pipeline are (the blend backward's float atomics may order differently from run to run, on one stream too), and
    otherwise within the bars tests/test_gpu_pipeline_terms.py holds two such runs to."""
    from fdgs import train_host
    from fdgs.pipeline import StepPipeline
    scene, cams, gts, pipe, bg = _views(gpu_device, 3)
    flats, firsts = {}, {}
    for mode in ("plain", "none", "plain-again"):
        mp = train_host.GaussianParams(scene, gpu_device)
        kw = dict(grad_terms=None) if mode == "none" else {}
        sp = StepPipeline(mp, train_host.make_optimizer(mp), world_size=1, lambda_dssim=0.2, overlap=False, **kw)
        assert sp.grad_terms == ()
        for k in range(3):
            res, ls = sp.step(cams, gts, pipe, bg)
            if k == 0:
                firsts[mode] = ([r["render"].clone() for r in res], torch.stack(list(ls)).clone())
        torch.cuda.synchronize()
        flats[mode] = mp.flat.clone()
    for a, b in zip(firsts["none"][0], firsts["plain"][0]):
        assert torch.equal(a, b)
    assert torch.equal(firsts["none"][1], firsts["plain"][1])
    if torch.equal(flats["plain"].view(torch.int32), flats["plain-again"].view(torch.int32)):     # two runs agree
        assert torch.equal(flats["none"].view(torch.int32), flats["plain"].view(torch.int32))
    else:
        perr = (flats["none"] - flats["plain"]).abs()
        assert (perr > 2e-3).float().mean().item() <= 2e-3 and perr.max().item() <= 0.25, ((perr > 2e-3).float().mean().item(), perr.max().item())
    with pytest.raises(NotImplementedError):
        StepPipeline(mp, train_host.make_optimizer(mp), world_size=2, grad_terms=[lambda sink: None])


# ---- end to end ----
def test_training_to_a_cap(gpu_device):
    """2000 Gaussians, cap 3000, 300 steps: P never exceeds the cap and ends at it, nothing is dead right after a refinement,
    everything stays finite and the loss falls.  A refinement every 30 steps: at 5 % per refinement 2000 reaches 3000 with the ninth
    (2000 x 1.05^8 = 2955), which one every 50 steps (six in 300) cannot."""
    from fdgs import mcmc, train_host
    from fdgs.fused import render_raw
    from fdgs.pipeline import StepPipeline
    dev = gpu_device
    cfg = synth.SceneConfig("mcmc-e2e", 2000, 160, 128, 2, 1, 0.04, 10.0, True, 4, False)
    scene = synth.make_scene(cfg, seed=6)
    pipe, bg = train_host.PipelineFlags(), torch.zeros(3, device=dev)
    target = train_host.GaussianParams(scene, dev)
    V, B = 8, 2
    cams = [train_host.SyntheticCamera(scene, dev, timestamp=(v + 0.5) / V * scene["time_duration"]) for v in range(V)]
    with torch.no_grad():
        gts = [render_raw(c, target, pipe, bg)["render"].clone() for c in cams]
    student = train_host.GaussianParams(scene, dev)
    g = torch.Generator(device="cpu").manual_seed(0)
    with torch.no_grad():
        student.params["_features"].add_(0.3 * torch.randn(student.params["_features"].shape, generator=g).to(dev))
        student.params["_xyz"].add_(0.01 * torch.randn(student.params["_xyz"].shape, generator=g).to(dev))
    opt = train_host.make_optimizer(student)
    strategy = mcmc.MCMCStrategy(student, opt, cap=3000, seed=1)
    sp = StepPipeline(student, opt, world_size=1, lambda_dssim=0.2, grad_terms=[strategy.add_regularizer_grads])
    losses, sizes = [], []
    for it in range(300):
        ix = [(it * B + b) % V for b in range(B)]
        _res, ls = sp.step([cams[i] for i in ix], [gts[i] for i in ix], pipe, bg)
        losses.append(torch.stack(list(ls)).mean())
        strategy.after_step()
        if (it + 1) % 30 == 0:
            out = strategy.refine()
            sizes.append(out["P_new"])
            assert student.P == out["P_new"] <= 3000
            alive, _, _ = mcmc.weights(student._opacity, strategy.min_opacity)
            assert bool(alive.all())
    torch.cuda.synchronize()
    losses = torch.stack(losses).cpu().numpy()
    print("sizes", sizes, "loss first 20 %.5f last 20 %.5f" % (losses[:20].mean(), losses[-20:].mean()), "terms", strategy.last_terms.tolist())
    assert sizes == sorted(sizes) and sizes[0] == 2100 and student.P == 3000
    assert torch.isfinite(student.flat).all() and np.isfinite(losses).all()
    assert losses[-20:].mean() < losses[:20].mean()
