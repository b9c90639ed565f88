"""GPU: the edges of the densification (csrc/densify.hip, fdgs/densify.py, DensificationStats.update in fdgs/harness.py):
fdgs_densify_classify on its own against the hand-built table of tests/densify_cases.py; densify_and_prune against
oracle/densify_oracle.py with N = 1 and 3, raw quaternions far from unit length, the empty and degenerate plans, and the samples
drawn from a generator; the statistics kernels at 1, 16, 17 and 33 views."""
import numpy as np
import pytest
import torch

import densify_cases as dc
from util import synth
from test_gpu_densify import _state_of
from test_oracle_densify import assert_state_equal

pytestmark = pytest.mark.gpu

CALLS = dc.calls()
KINDS = {"rot4d": (3, 2, True, 4), "dim4_norot": (1, 0, False, 4), "dim3": (2, 0, False, 3)}     # sh_degree, sh_degree_t, rot_4d, gaussian_dim
MAX_GRAD, MAX_GRAD_T = 2e-4, 2e-4 / 40


@pytest.mark.parametrize("call", [c for _, c in CALLS], ids=[t for t, _ in CALLS])
def test_classify_flags_equal_the_table(gpu_device, call):
    """fdgs_densify_classify called directly: the flag byte of EVERY row equals the float64 restatement's (rows exactly on a
    threshold included: g == max_grad clones / splits, smax == limit clones and is not pruned, max_radii2D == max_screen_size is
    not pruned), at P = 1, 255, 256, 257 (one workgroup short, exact, one past) -- max_screen_size None travels as -1, 0 as 0."""
    from fdgs import _capi
    dev = gpu_device
    for P in dc.P_SIZES:
        t = dc.table(call, P)
        want = dc.expected_flags(call, t)
        d = {k: torch.from_numpy(v).to(dev).contiguous() for k, v in t.items()}
        flags = torch.full((P,), 0xFF, dtype=torch.uint8, device=dev)
        screen = -1.0 if call["max_screen_size"] is None else float(call["max_screen_size"])
        rc = _capi.lib.fdgs_densify_classify(P, d["xyz_gradient_accum"].data_ptr(), d["denom"].data_ptr(), d["scaling_raw"].data_ptr(),
                                             d["opacity_raw"].data_ptr(), d["max_radii2D"].data_ptr(), call["max_grad"], call["min_opacity"],
                                             call["extent"], screen, call["percent_dense"], call["N"], int(call["prune_only"]),
                                             flags.data_ptr(), _capi.current_stream_handle(dev))
        assert rc == 0
        torch.cuda.synchronize()
        got = flags.cpu().numpy()
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, [(int(i), int(i) % len(dc._ROWS), int(got[i]), int(want[i])) for i in bad[:8]]


def _names(kind):
    _, _, rot_4d, gdim = KINDS[kind]
    return ("_xyz", "_features", "_opacity", "_scaling", "_rotation") + (("_t", "_scaling_t") if gdim == 4 else ()) + (("_rotation_r",) if rot_4d else ())


def _setup(kind, P, dev, seed, quat_norms=True):
    """A random model of P Gaussians with populated moments and statistics, raw quaternions of norm 0.1 ... 10, and the same
    state as the oracle's dict."""
    from fdgs import harness, train_host
    shd, shdt, rot_4d, gdim = KINDS[kind]
    cfg = synth.SceneConfig("d", P, 64, 48, shd, shdt, 0.05, 10.0 if rot_4d else 1.0, rot_4d, gdim, gdim == 4 and not rot_4d)
    scene = synth.make_scene(cfg, seed=seed)
    model = train_host.GaussianParams(scene, dev)
    opt = train_host.make_optimizer(model)
    g = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        if quat_norms:
            for n in ("_rotation", "_rotation_r"):
                model.params[n].mul_((10.0 ** (torch.rand(P, 1, generator=g) * 2 - 1)).to(dev))
        opt.exp_avg.copy_(torch.randn(opt.exp_avg.shape, generator=g) * 1e-3)
        opt.exp_avg_sq.copy_(torch.rand(opt.exp_avg_sq.shape, generator=g) * 1e-6)
    stats = harness.DensificationStats(P, dev, 1)
    stats.denom.copy_(torch.randint(0, 4, (P, 1), generator=g).float())
    stats.xyz_gradient_accum.copy_(torch.rand(P, 1, generator=g) * stats.denom.cpu() * 4 * MAX_GRAD)
    stats.t_gradient_accum.copy_(torch.rand(P, 1, generator=g) * stats.denom.cpu() * 1e-4)
    stats.max_radii2D.copy_(torch.randint(0, 50, (P,), generator=g).float())
    return model, opt, stats


def _oracle_state(kind, model, opt, stats):
    names = _names(kind)
    cut = lambda buf, n: buf[slice(*model.offsets[n])].detach().cpu().numpy().reshape(model.params[n].shape).copy()   # noqa: E731
    st = {"params": {n: cut(model.flat, n) for n in names}, "exp_avg": {n: cut(opt.exp_avg, n) for n in names},
          "exp_avg_sq": {n: cut(opt.exp_avg_sq, n) for n in names},
          "xyz_gradient_accum": stats.xyz_gradient_accum.cpu().numpy().copy(), "denom": stats.denom.cpu().numpy().copy(),
          "max_radii2D": stats.max_radii2D.cpu().numpy().copy()}
    if KINDS[kind][3] == 4:
        st["t_gradient_accum"] = stats.t_gradient_accum.cpu().numpy().copy()
    return st


def _split_selection(st, extent, percent_dense=0.01):
    with np.errstate(divide="ignore", invalid="ignore"):
        grads = np.nan_to_num(st["xyz_gradient_accum"] / st["denom"], nan=0.0, posinf=np.inf)
    return (grads[:, 0] >= MAX_GRAD) & (np.exp(st["params"]["_scaling"]).max(1) > percent_dense * extent)


def _median_extent(st):
    return float(np.median(np.exp(st["params"]["_scaling"]).max(1)) / 0.01)       # half of the Gaussians are 'small'


def _assert_consistent(model, opt, stats):
    """model, optimizer and statistics describe the same number of Gaussians"""
    P, per = model.P, model.floats_per_gaussian()
    assert model.flat.numel() == model.flat_grad.numel() == opt.exp_avg.numel() == opt.exp_avg_sq.numel() == P * per
    assert all(model.params[n].shape[0] == P and model.params[n].grad.shape == model.params[n].shape for n in model.NAMES)
    assert stats.xyz_gradient_accum.shape == stats.t_gradient_accum.shape == stats.denom.shape == (P, 1) and stats.max_radii2D.shape == (P,)
    assert [s["end"] for s in opt.segments][-1] == P * per and all(tuple(model.offsets[s["name"]]) == (s["begin"], s["end"]) for s in opt.named_segments())


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("kind", list(KINDS))
def test_densify_split_counts_and_unnormalised_quaternions(gpu_device, kind, N):
    """densify_and_prune with N = 1 and N = 3 children per parent (inv_split, the arange(N) * k + kept row arithmetic, the order
    copy 1 ... copy N) on 4D-rotation, 4D and 3D models whose raw quaternions have norms 0.1 ... 10 (the split kernel normalises
    them itself), against the numpy oracle fed the same injected samples."""
    from fdgs.densify import densify_and_prune
    from oracle import densify_oracle as do
    _, _, rot_4d, gdim = KINDS[kind]
    model, opt, stats = _setup(kind, 301, gpu_device, 11 + N)
    st = _oracle_state(kind, model, opt, stats)
    extent = _median_extent(st)
    sel = _split_selection(st, extent)
    k = int(sel.sum())
    assert k >= 20
    g = torch.Generator(device="cpu").manual_seed(3)
    cols = [st["params"]["_scaling"]] + ([st["params"]["_scaling_t"]] if rot_4d else [])
    stds = np.exp(np.concatenate(cols, 1))[sel]
    samples = (torch.randn(N * k, stds.shape[1], generator=g).numpy() * np.concatenate([stds] * N, 0)).astype(np.float32)
    samples_t = None
    if gdim == 4 and not rot_4d:
        samples_t = (torch.randn(N * k, 1, generator=g).numpy() * np.concatenate([np.exp(st["params"]["_scaling_t"])[sel]] * N, 0)).astype(np.float32)
    # opacity limit at the lower quartile: some parents lose their children (kept rows != all rows: the row arithmetic matters)
    min_opacity = float(np.quantile(1 / (1 + np.exp(-st["params"]["_opacity"])), 0.25))
    want = do.densify_and_prune(st, MAX_GRAD, min_opacity, extent, 20, MAX_GRAD_T, percent_dense=0.01, N=N, rot_4d=rot_4d, gaussian_dim=gdim,
                                samples=samples, samples_t=samples_t)
    rep = densify_and_prune(model, opt, stats, MAX_GRAD, min_opacity, extent, 20, MAX_GRAD_T, N=N, samples=torch.from_numpy(samples).to(gpu_device),
                            samples_t=None if samples_t is None else torch.from_numpy(samples_t).to(gpu_device))
    torch.cuda.synchronize()
    assert rep["split_parents"] == k and 0 < rep["children"] < N * k and rep["children"] % N == 0 and rep["cloned"] > 0, rep
    assert rep["P_new"] == model.P == want["params"]["_xyz"].shape[0], rep
    _assert_consistent(model, opt, stats)
    assert_state_equal(_state_of(model, opt, stats, want), want, rtol=3e-6, atol=3e-6)


@pytest.mark.parametrize("kind", ["rot4d", "dim4_norot"])
def test_densify_draws_its_samples_from_the_generator(gpu_device, kind):
    """samples=None, the path every run takes: the normal draws come from ``generator`` -- one torch.normal over the N-fold repeated
    standard deviations of all split parents, and a second one for the time axis of a 4D model without rot_4d.  The test repeats
    those calls on an equally seeded generator, hands the draws to the oracle and expects the same model."""
    from fdgs.densify import densify_and_prune
    from oracle import densify_oracle as do
    dev = gpu_device
    _, _, rot_4d, gdim = KINDS[kind]
    N = 2
    model, opt, stats = _setup(kind, 301, dev, 21)
    st = _oracle_state(kind, model, opt, stats)
    extent = _median_extent(st)
    idx_sel = torch.from_numpy(np.nonzero(_split_selection(st, extent))[0]).to(dev)
    assert idx_sel.numel() >= 20
    gen = torch.Generator(device=dev).manual_seed(77)
    if rot_4d:
        stds = torch.exp(torch.cat([model._scaling[idx_sel], model._scaling_t[idx_sel]], 1)).repeat(N, 1).detach()
    else:
        stds = torch.exp(model._scaling[idx_sel]).repeat(N, 1).detach()
    samples = torch.normal(mean=torch.zeros_like(stds), std=stds, generator=gen)
    samples_t = None
    if not rot_4d:
        stds_t = torch.exp(model._scaling_t[idx_sel]).repeat(N, 1).detach()
        samples_t = torch.normal(mean=torch.zeros_like(stds_t), std=stds_t, generator=gen).cpu().numpy()
    assert float(samples.abs().max()) > 0
    want = do.densify_and_prune(st, MAX_GRAD, 0.02, extent, 20, MAX_GRAD_T, percent_dense=0.01, N=N, rot_4d=rot_4d, gaussian_dim=gdim,
                                samples=samples.cpu().numpy(), samples_t=samples_t)
    rep = densify_and_prune(model, opt, stats, MAX_GRAD, 0.02, extent, 20, MAX_GRAD_T, N=N, generator=torch.Generator(device=dev).manual_seed(77))
    torch.cuda.synchronize()
    assert rep["split_parents"] == idx_sel.numel() and rep["children"] > 0 and rep["P_new"] == want["params"]["_xyz"].shape[0], rep
    _assert_consistent(model, opt, stats)
    assert_state_equal(_state_of(model, opt, stats, want), want, rtol=3e-6, atol=3e-6)


def _run_against_oracle(kind, model, opt, stats, dev, min_opacity, extent, screen, prune_only=False, N=2):
    from fdgs.densify import densify_and_prune
    from oracle import densify_oracle as do
    _, _, rot_4d, gdim = KINDS[kind]
    st = _oracle_state(kind, model, opt, stats)
    k = 0 if prune_only else int(_split_selection(st, extent).sum())
    samples = np.full((N * k, 4 if rot_4d else 3), 0.01, np.float32)
    samples_t = np.full((N * k, 1), 0.02, np.float32) if gdim == 4 and not rot_4d else None
    want = do.densify_and_prune(st, MAX_GRAD, min_opacity, extent, screen, MAX_GRAD_T, prune_only=prune_only, percent_dense=0.01, N=N,
                                rot_4d=rot_4d, gaussian_dim=gdim, samples=samples, samples_t=samples_t)
    rep = densify_and_prune(model, opt, stats, MAX_GRAD, min_opacity, extent, screen, MAX_GRAD_T, prune_only=prune_only, N=N,
                            samples=torch.from_numpy(samples).to(dev), samples_t=None if samples_t is None else torch.from_numpy(samples_t).to(dev))
    torch.cuda.synchronize()
    assert rep["P_new"] == model.P == want["params"]["_xyz"].shape[0], rep
    _assert_consistent(model, opt, stats)
    assert_state_equal(_state_of(model, opt, stats, want), want, rtol=3e-6, atol=3e-6)
    return rep, k


def test_densify_with_nothing_to_do_changes_nothing_but_the_statistics(gpu_device):
    """No gradient reaches max_grad, nothing is transparent, no size test: parameters and moments bit-equal, the statistics restart
    from zero (densification_postfix runs even for an empty clone / split)."""
    from fdgs.densify import densify_and_prune
    model, opt, stats = _setup("rot4d", 300, gpu_device, 31)
    stats.xyz_gradient_accum.mul_(0.2)          # accum / denom < 0.8 max_grad
    before = (model.flat.detach().clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone())
    rep = densify_and_prune(model, opt, stats, MAX_GRAD, 0.0, 6.0, None, MAX_GRAD_T)
    torch.cuda.synchronize()
    assert rep == {"P_old": 300, "P_new": 300, "kept": 300, "cloned": 0, "split_parents": 0, "children": 0}
    assert torch.equal(model.flat, before[0]) and torch.equal(opt.exp_avg, before[1]) and torch.equal(opt.exp_avg_sq, before[2])
    _assert_consistent(model, opt, stats)
    for name in ("xyz_gradient_accum", "t_gradient_accum", "denom", "max_radii2D"):
        assert float(getattr(stats, name).abs().max()) == 0.0, name


def test_densify_parents_split_but_every_child_pruned(gpu_device):
    """k > 0, kk == 0: every Gaussian that splits is transparent, so its children go the way it goes; the rest of the plan holds."""
    model, opt, stats = _setup("dim4_norot", 300, gpu_device, 32)
    st = _oracle_state("dim4_norot", model, opt, stats)
    extent = _median_extent(st)
    sel = torch.from_numpy(_split_selection(st, extent)).to(gpu_device)
    with torch.no_grad():
        model._opacity[sel] = -6.0      # sigmoid = 0.0025
        model._opacity[~sel] = 2.0
    rep, k = _run_against_oracle("dim4_norot", model, opt, stats, gpu_device, 0.01, extent, 20)
    assert k >= 20 and rep["split_parents"] == k and rep["children"] == 0 and rep["cloned"] > 0 and rep["P_new"] == rep["kept"] + rep["cloned"], rep


@pytest.mark.parametrize("prune_only", [False, True], ids=["densify", "pruneonly"])
def test_densify_down_to_one_gaussian_and_from_one(gpu_device, prune_only):
    """Everything is pruned but one Gaussian; then a densification of that single-Gaussian model (P = 1)."""
    model, opt, stats = _setup("rot4d", 300, gpu_device, 33)
    with torch.no_grad():
        model._opacity.fill_(-6.0)
        model._opacity[123] = 2.0
        model._scaling[123] = -9.0                   # small: it can only be cloned
        stats.max_radii2D[123] = 3.0
        stats.denom[123] = 0.0
        stats.xyz_gradient_accum[123] = 0.0          # 0 / 0: no gradient, it is neither cloned nor split
    rep, _ = _run_against_oracle("rot4d", model, opt, stats, gpu_device, 0.01, 6.0, 20, prune_only=prune_only)
    assert rep["P_new"] == 1 and rep["kept"] == 1, rep
    stats.denom.fill_(1.0)
    stats.xyz_gradient_accum.fill_(1.0)          # now it clones
    rep, _ = _run_against_oracle("rot4d", model, opt, stats, gpu_device, 0.01, 6.0, 20)
    assert rep == {"P_old": 1, "P_new": 2, "kept": 1, "cloned": 1, "split_parents": 0, "children": 0}


@pytest.mark.parametrize("prune_only", [False, True], ids=["densify", "pruneonly"])
@pytest.mark.parametrize("kind", ["rot4d", "dim3"])
def test_densify_that_prunes_everything_leaves_an_empty_consistent_model(gpu_device, kind, prune_only):
    """P_new == 0.  The reference's prune_points with an all-true mask leaves empty tensors everywhere (parameters, optimizer state,
    statistics), and so does densify_and_prune: P = 0, empty flat buffers and moments, statistics of length 0 -- equal to the
    oracle, and model, optimizer and statistics agree on the size."""
    model, opt, stats = _setup(kind, 300, gpu_device, 34)
    rep, k = _run_against_oracle(kind, model, opt, stats, gpu_device, 1.5, _median_extent(_oracle_state(kind, model, opt, stats)), 20,
                                 prune_only=prune_only)
    assert rep["P_new"] == 0 and model.P == 0 and model.flat.numel() == 0 and opt.exp_avg.numel() == 0, rep
    assert prune_only or (k >= 20 and rep["split_parents"] == k and rep["children"] == 0)
    assert stats.denom.shape == (0, 1) and stats.max_radii2D.shape == (0,)


@pytest.mark.parametrize("with_t", [False, True], ids=["no-t-grad", "t-grad"])
@pytest.mark.parametrize("P", [1, 257, 5000])
@pytest.mark.parametrize("B", [1, 16, 17, 33])
def test_stats_update_view_counts(gpu_device, B, P, with_t):
    """DensificationStats.update on the GPU against the PyTorch statement on the CPU with 1, 16 (one kernel call, full), 17 and 33
    (two and three calls, the groups combined) views, P below, across and far above a workgroup, dL/dt given or not."""
    from fdgs import harness
    g = torch.Generator().manual_seed(100 * B + P)
    gpu = harness.DensificationStats(P, gpu_device, 1)
    cpu = harness.DensificationStats(P, "cpu", 1)
    for _ in range(2):
        radii = [torch.randint(-3, 12, (P,), generator=g).clamp(min=0).to(torch.int32) for _ in range(B)]
        grads = [torch.randn(P, 3, generator=g) for _ in range(B)]
        t_grad = torch.randn(P, 1, generator=g) if with_t else None
        cpu.update([{"radii": r, "viewspace_grad": x} for r, x in zip(radii, grads)], t_grad, B)
        gpu.update([{"radii": r.to(gpu_device), "viewspace_grad": x.to(gpu_device)} for r, x in zip(radii, grads)],
                   None if t_grad is None else t_grad.to(gpu_device), B)
    torch.cuda.synchronize()
    for name in ("xyz_gradient_accum", "t_gradient_accum", "denom", "max_radii2D"):
        np.testing.assert_allclose(getattr(gpu, name).cpu().numpy(), getattr(cpu, name).numpy(), rtol=2e-6, atol=1e-7, err_msg=name)
    assert with_t or float(gpu.t_gradient_accum.abs().max()) == 0.0
    assert float(gpu.denom.max()) > 0 or P == 1
