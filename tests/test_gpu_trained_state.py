"""GPU: the HIP product on the state a training run leaves behind (tests/golden/trained_*.npz, recorded once by
tests/golden/make_golden_trained.py: raw quaternions far from unit, scales Adam has moved, split children on top of their siblings,
clones, opacities pinned at 0.01 after a reset, colours clamped at 0, SH degrees part-way up the ramp, densification statistics of
real steps) -- against the reference's stored outputs, the port oracle and the numpy densification oracle, at the bars the synthetic
scenes are held to.  tests/test_trained_state_host.py checks on the CPU that the fixtures are what they claim and that the reference
itself is well conditioned on them."""
import math

import numpy as np
import pytest
import torch

import golden_util
from test_gpu_densify import NAMES, _state_of
from test_gpu_golden import check_forward_vs_fixture
from test_gpu_parity import _timed_path_vs_oracle
from test_oracle_densify import assert_state_equal
from util import CHAIN_ACTIVATED, check_backward_noise_aware, check_forward, fmt_noise_rep, oracle_four_modes, pyoracle, run_hip

pytestmark = pytest.mark.gpu

TRAINED = golden_util.TRAINED
_REF = {}


def _reference(name, v):
    """The port oracle's forward and its backward in the four accumulation modes on view ``v`` of a fixture: computed once, shared."""
    if (name, v) not in _REF:
        scene, up, fw, bw = golden_util.load_trained(name)["views"][v]
        o = pyoracle.Oracle(scene, kind="port")
        ref = dict(o.forward())
        ref["R"] = o.R
        modes = oracle_four_modes(o, up)
        o.close()
        _REF[(name, v)] = (ref, modes)
    return _REF[(name, v)]


# ----------------------------------------------------------------------------------------------------------------------------
# a. activated inputs, the reference's lists and tile_cull
# ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile_cull", [False, True])
@pytest.mark.parametrize("name", TRAINED)
def test_activated_inputs_vs_reference(name, tile_cull, gpu_device):
    f = golden_util.load_trained(name)
    for v, (scene, up, fw, bw) in enumerate(f["views"]):
        label = "%s view %d%s" % (name, v, " tile_cull" if tile_cull else "")
        P, W, H = int(scene["means3D"].shape[0]), scene["W"], scene["H"]
        hip, hipg = run_hip(scene, gpu_device, up, tile_cull=tile_cull)
        ref, (refg, refg_rev, refg_f64, refg_probe) = _reference(name, v)
        if not tile_cull:
            check_forward_vs_fixture(label, scene, fw, hip)
        rep = check_forward(hip, ref, label, tile_cull=tile_cull, WH=(W, H))
        repg = check_backward_noise_aware(hipg, refg, refg_rev, refg_f64, refg_probe, label, chain=CHAIN_ACTIVATED)
        print(label, "R", ref["R"], {k: ("%.2e" % x if isinstance(x, float) else x) for k, x in rep.items()})
        print(label, fmt_noise_rep(repg))
        print("%s: worst |hip - f64| / bound %.2f, Gaussians beyond the plain bar %d of %d" % (
            label, max(r[4] for r in repg.values()), max(r[3] for r in repg.values()), P))
        for k, r in repg.items():
            assert r[3] <= 0.02 * P, "%s: %s beyond the plain bar on %d of %d Gaussians" % (label, k, r[3], P)
        if name.endswith("_reset"):
            # opacities of 0.01: a splat reaches alpha >= 1/255 only next to its centre -- nearly every tile-list entry is dead weight
            ok = ~ref["border"].astype(bool)
            np.testing.assert_array_equal((hip["n_contrib"] == 0)[ok], (ref["n_contrib"] == 0)[ok], err_msg=label + ": pixels nothing contributes to")
            assert (ref["n_contrib"] == 0)[ok].any() and (ref["n_contrib"] > 0)[ok].any()
            if tile_cull:
                kept, total = (int(x) for x in rep["instances"].split(" of "))
                print("%s: tile_cull keeps %d of %d instances (%.1f %%)" % (label, kept, total, 100.0 * kept / total))
                assert kept < total, label + ": tile_cull took nothing out of lists of 0.01-opacity splats"


# ----------------------------------------------------------------------------------------------------------------------------
# b. raw parameters through the path the trainer runs
# ----------------------------------------------------------------------------------------------------------------------------

def _model_from_fixture(f, device):
    from fdgs import train_host
    meta = f["meta"]
    tensors = {n: torch.from_numpy(f["raw"][n].copy()) for n in NAMES}
    return train_host.GaussianParams.from_raw(
        tensors, device, max_sh_degree=int(meta["max_sh_degree"]), max_sh_degree_t=int(meta["max_sh_degree_t"]),
        active_sh_degree=int(meta["active_sh_degree"]), active_sh_degree_t=int(meta["active_sh_degree_t"]),
        time_duration=(0.0, float(meta["time_duration"])), rot_4d=bool(meta["rot_4d"]), gaussian_dim=int(meta["gaussian_dim"]),
        force_sh_3d=bool(meta["force_sh_3d"]))


@pytest.mark.parametrize("tile_cull", [False, True])
@pytest.mark.parametrize("name", TRAINED)
def test_raw_parameters_timed_path_vs_oracle(name, tile_cull, gpu_device):
    """The fused activations and their float64 chain rule at |q| far from 1 and opacities of 0.01, the L1 + SSIM upstream gradient,
    the accumulation over two views and the all-zero blend accumulator: test_gpu_parity._timed_path_vs_oracle on the recorded model."""
    from fdgs import _capi
    f = golden_util.load_trained(name)
    model = _model_from_fixture(f, gpu_device)
    # The helper feeds the oracle the kernels' OWN activations (fdgs_debug_activations), so only the chain rule is checked independently
    # there.  The forward activations themselves, at |q| up to 2.3 and opacities of 0.01, against the torch values the fixture stores:
    # the bars tests/test_gpu_api.py::test_render_raw_matches_render holds them to on near-unit quaternions (an ulp or two).
    act = _capi.debug_activations(model._opacity.detach(), model._scaling.detach(), model._scaling_t.detach(), model._rotation.detach(),
                                  model._rotation_r.detach())
    torch.cuda.synchronize()
    a_op, a_sc, a_sct, a_rot, a_rotr = [t.cpu().numpy() for t in act]
    ext = {k: golden_util.trained_input(name, k) for k in ("opacities", "scales", "scales_t", "rotations", "rotations_r")}
    err = {"opacities": float(np.abs(a_op - ext["opacities"]).max()), "scales": float((np.abs(a_sc - ext["scales"]) / ext["scales"]).max()),
           "rotations": float(np.abs(a_rot - ext["rotations"]).max())}
    if f["meta"]["gaussian_dim"] == 4:
        err["scales_t"] = float((np.abs(a_sct - ext["scales_t"]) / ext["scales_t"]).max())
    if f["meta"]["rot_4d"]:
        err["rotations_r"] = float(np.abs(a_rotr - ext["rotations_r"]).max())
    print("trained %s: kernel activations against torch's:" % name, {k: "%.2e" % e for k, e in err.items()})
    for k, e in err.items():
        assert e <= (3e-7 if k.startswith("scales") else 2e-7), "%s: activated %s differs from torch's by %g" % (name, k, e)
    cams = []
    for scene, up, fw, bw in f["views"]:
        cam = {k: scene[k] for k in ("world_view_transform", "full_proj_transform", "camera_center")}
        # (the field of view is what a camera holds; both sides take the tangent from it)
        cam["FoVx"], cam["FoVy"] = 2.0 * math.atan(scene["tanfovx"]), 2.0 * math.atan(scene["tanfovy"])
        cam["tanfovx"], cam["tanfovy"] = math.tan(0.5 * cam["FoVx"]), math.tan(0.5 * cam["FoVy"])
        cams.append((cam, float(scene["timestamp"])))
    _timed_path_vs_oracle(None, gpu_device, 2, "trained %s" % name, 1e-3, tile_cull=tile_cull, ready=(model, dict(f["views"][0][0]), cams))


# ----------------------------------------------------------------------------------------------------------------------------
# c. densification on real statistics
# ----------------------------------------------------------------------------------------------------------------------------

def _densify_setup(f, device):
    """Model / optimizer / statistics holding a fixture's arrays (seeded random Adam moments), and the same as an oracle state."""
    from fdgs import harness, train_host
    meta = f["meta"]
    model = _model_from_fixture(f, device)
    opt = train_host.make_optimizer(model)
    g = torch.Generator(device="cpu").manual_seed(5)
    opt.exp_avg.copy_(torch.randn(opt.exp_avg.shape, generator=g) * 1e-3)
    opt.exp_avg_sq.copy_(torch.rand(opt.exp_avg_sq.shape, generator=g) * 1e-6)
    stats = harness.DensificationStats(model.P, device, 1)
    for k in ("xyz_gradient_accum", "t_gradient_accum", "denom", "max_radii2D"):
        getattr(stats, k).copy_(torch.from_numpy(f["stats"][k]))
    names = [n for n in NAMES if not ((n in ("_t", "_scaling_t") and meta["gaussian_dim"] == 3) or (n == "_rotation_r" and not meta["rot_4d"]))]
    st = {"params": {n: model.params[n].detach().cpu().numpy().copy() for n in names},
          "exp_avg": {n: opt.exp_avg[slice(*model.offsets[n])].cpu().numpy().reshape(model.params[n].shape).copy() for n in names},
          "exp_avg_sq": {n: opt.exp_avg_sq[slice(*model.offsets[n])].cpu().numpy().reshape(model.params[n].shape).copy() for n in names},
          "xyz_gradient_accum": f["stats"]["xyz_gradient_accum"].copy(), "denom": f["stats"]["denom"].copy(),
          "max_radii2D": f["stats"]["max_radii2D"].copy()}
    if meta["gaussian_dim"] == 4:
        st["t_gradient_accum"] = f["stats"]["t_gradient_accum"].copy()
    return model, opt, stats, st, g


@pytest.mark.parametrize("name,N", [("rot4d_reset", 2), ("rot4d_end", 2), ("rot4d_end", 3), ("dim3_end", 2)])
def test_densify_on_recorded_statistics_vs_oracle(name, N, gpu_device):
    """densify_and_prune(max_screen_size=20) on the recorded model and statistics against the numpy oracle.  The thresholds are chosen
    from the fixture so that every decision of densify_classify is taken both ways: max_grad = the 70th percentile of the mean view-space
    gradients (Gaussians with denom == 0 give NaN -> 0), the clone / split limit the recorded run's (percent_dense * extent = 0.07), and
    the extent such that the children of the largest tenth of the split parents are still larger than 0.1 * extent."""
    from fdgs.densify import densify_and_prune
    from oracle import densify_oracle as do
    f = golden_util.load_trained(name)
    meta = f["meta"]
    model, opt, stats, st, g = _densify_setup(f, gpu_device)
    P = model.P
    with np.errstate(divide="ignore", invalid="ignore"):
        grads = (st["xyz_gradient_accum"] / st["denom"]).astype(np.float32)
    assert np.isnan(grads).any(), "no Gaussian with denom == 0: the NaN -> 0 branch is not exercised"
    grads[np.isnan(grads)] = 0.0
    max_grad = float(np.percentile(grads[:, 0], 70))
    smax = np.exp(st["params"]["_scaling"]).max(1)
    hot = grads[:, 0] >= max_grad
    small_limit = 0.07
    extent = float(np.percentile(smax[hot & (smax > small_limit)], 90)) / (0.1 * 0.8 * N)
    percent_dense = small_limit / extent
    # the split parents, counted the oracle's way; the samples of ALL of them drawn once and handed to both
    sel = hot & (smax > np.float32(percent_dense * extent))
    k = int(sel.sum())
    child_big = np.exp(np.log(smax[sel] / np.float32(0.8 * N))) > 0.1 * extent
    n_clone = int((hot & ~sel).sum())
    assert k > 10 and n_clone > 0 and 0 < int(child_big.sum()) < k, (k, n_clone, int(child_big.sum()))
    rot_4d, dim = bool(meta["rot_4d"]), int(meta["gaussian_dim"])
    stds = np.exp(np.concatenate([st["params"]["_scaling"], st["params"]["_scaling_t"]], 1) if rot_4d else st["params"]["_scaling"])[sel]
    samples = (torch.randn(N * k, stds.shape[1], generator=g).numpy() * np.concatenate([stds] * N, 0)).astype(np.float32)
    want = do.densify_and_prune(st, max_grad, 0.005, extent, 20, None, percent_dense=percent_dense, N=N, rot_4d=rot_4d, gaussian_dim=dim, samples=samples)
    rep = densify_and_prune(model, opt, stats, max_grad, 0.005, extent, 20, None, percent_dense=percent_dense, N=N,
                            samples=torch.from_numpy(samples).to(gpu_device))
    torch.cuda.synchronize()
    print("%s N %d: %s; children too large for the scene: %d parents; extent %.3f max_grad %.2e" % (name, N, rep, int(child_big.sum()), extent, max_grad))
    assert rep["split_parents"] == k and rep["cloned"] > 0 and rep["children"] < N * k, rep
    assert rep["P_new"] == want["params"]["_xyz"].shape[0] != P, rep
    assert_state_equal(_state_of(model, opt, stats, want), want, rtol=3e-6, atol=3e-6)


def test_prune_only_on_state_after_reset_vs_oracle(gpu_device):
    """prune_only with max_screen_size = 20 and min_opacity = 0.005 two iterations after an opacity reset: the statistics survive, the
    rows whose recorded max_radii2D exceeds 20 px go (the one place the screen-size test acts, as in the reference)."""
    from fdgs.densify import densify_and_prune
    from oracle import densify_oracle as do
    f = golden_util.load_trained("rot4d_reset")
    model, opt, stats, st, _ = _densify_setup(f, gpu_device)
    extent = float(f["meta"]["recipe_cameras_extent"])
    big_vs = int((st["max_radii2D"] > 20).sum())
    big_ws = int((np.exp(st["params"]["_scaling"]).max(1) > 0.1 * extent).sum())
    assert 0 < big_vs < model.P, big_vs
    want = do.densify_and_prune(st, 1.0, 0.005, extent, 20, None, prune_only=True, rot_4d=True, gaussian_dim=4)
    rep = densify_and_prune(model, opt, stats, 1.0, 0.005, extent, 20, None, prune_only=True)
    torch.cuda.synchronize()
    print("prune_only after reset: %s; max_radii2D > 20 on %d rows, scale > 0.1 extent on %d" % (rep, big_vs, big_ws))
    assert rep["P_new"] == want["params"]["_xyz"].shape[0] and rep["P_old"] - rep["P_new"] >= big_vs
    assert_state_equal(_state_of(model, opt, stats, want), want, rtol=3e-6, atol=3e-6)
