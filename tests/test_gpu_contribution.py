"""GPU: the contribution statistics and the ID map (csrc/contribution.hip, fdgs_contribution, fdgs.importance) against the numpy
restatement of the port oracle's forward (tests/contribution_oracle.py, pinned to the oracle by tests/test_contribution_oracle_host.py).

The oracle's ``border`` pixels (a decision within 1e-5 of the alpha = 1/255 or the T = 1e-4 cliff) and the restatement's ``near_tie``
pixels (the two largest w within 1e-5 relative) get weight 0 in ``pix_weight`` ON BOTH SIDES; nothing else is excluded, and every
case asserts that they are at most 1 % of the pixels.  Bars: hits, dominant and dominant_id exact; weight_max within PIX_TOL;
weight_sum within GRAD_TOL * max(1, max |ref|); hits, dominant, dominant_id and weight_max bit-identical between two runs."""
import numpy as np
import pytest
import torch

from util import GRAD_TOL, PIX_TOL, native_args_fwd, run_oracle, scene_to_device, synth

import contribution_cases as cases
import contribution_oracle as co

pytestmark = pytest.mark.gpu


def _fwd(sc, **kw):
    from fdgs.gaussian_renderer.diff_gaussian_rasterization import _C
    return _C.rasterize_gaussians(*native_args_fwd(sc), **kw)


def _fresh(P, W, H, dev):
    return {"weight_sum": torch.zeros(P, dtype=torch.float32, device=dev), "weight_max": torch.zeros(P, dtype=torch.float32, device=dev),
            "hits": torch.zeros(P, dtype=torch.int32, device=dev), "dominant": torch.zeros(P, dtype=torch.int32, device=dev),
            "dominant_id": torch.full((H, W), -7, dtype=torch.int32, device=dev)}


def _pass(res, P, W, H, pw, dev, into=None):
    """The statistics pass behind the forward ``res``; returns the five outputs as device tensors."""
    from fdgs import importance
    out = _fresh(P, W, H, dev) if into is None else into
    importance.contribution_pass(P, W, H, res[6], res[7], res[8], res[0], pix_weight=None if pw is None else torch.from_numpy(pw).to(dev), **out)
    return out


def _np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check(got, want, label):
    np.testing.assert_array_equal(got["dominant_id"], want["dominant_id"], err_msg=label + " dominant_id")
    np.testing.assert_array_equal(got["hits"].astype(np.int64), want["hits"], err_msg=label + " hits")
    np.testing.assert_array_equal(got["dominant"].astype(np.int64), want["dominant"], err_msg=label + " dominant")
    e_max = float(np.abs(got["weight_max"] - want["weight_max"]).max()) if want["weight_max"].size else 0.0
    scale = max(1.0, float(np.abs(want["weight_sum"]).max()) if want["weight_sum"].size else 1.0)
    e_sum = float(np.abs(got["weight_sum"] - want["weight_sum"]).max()) if want["weight_sum"].size else 0.0
    print("%s: weight_max err %.3g (bar %.1g)  weight_sum err %.3g (bar %.3g)" % (label, e_max, PIX_TOL, e_sum, GRAD_TOL * scale))
    assert e_max <= PIX_TOL, (label, e_max)
    assert e_sum <= GRAD_TOL * scale, (label, e_sum, scale)


def _weights(name, kind, excl, H, W):
    """``pix_weight`` of a case: NULL where nothing is flagged, otherwise the exclusion map only ("exclusion"); a random map with
    about 30 % zeros, times the exclusion map ("random")."""
    if kind == "exclusion":
        return None if not excl.any() else (~excl).astype(np.float32)
    return cases.random_weights(H, W, 11) * (~excl).astype(np.float32)


@pytest.mark.parametrize("tile_cull", [False, True], ids=["reference-lists", "tile-cull"])
@pytest.mark.parametrize("kind", ["exclusion", "random"])
@pytest.mark.parametrize("name", ["a", "b", "c", "d", "opaque", "1x1", "8x8", "17x9"])
def test_statistics_against_the_oracle(name, kind, tile_cull, gpu_device):
    scene, ref, wk, excl = cases.oracle(name)
    P, W, H = int(scene["means3D"].shape[0]), int(scene["W"]), int(scene["H"])
    assert float(excl.mean()) <= 0.01, "%s: %g of the pixels are cliff or near-tie pixels by the oracle" % (name, excl.mean())
    if name == "opaque":
        early = float(wk["ended_early"].mean())
        assert early >= 0.05, "the opaque scene ends only %g of its pixels early: the early-termination path is not tested" % early
    pw = _weights(name, kind, excl, H, W)
    if kind == "random":
        assert pw is not None and (0.2 < float((pw == 0).mean()) < 0.45 or H * W < 1000)
    want = co.reduce(wk, P, pw)
    res = _fwd(scene_to_device(scene, gpu_device), tile_cull=tile_cull)
    first = _np(_pass(res, P, W, H, pw, gpu_device))
    _check(first, want, "%s/%s/%s" % (name, kind, "cull" if tile_cull else "ref"))
    # the same forward once more: everything but the float sum is bit-identical
    again = _np(_pass(res, P, W, H, pw, gpu_device))
    for k in ("hits", "dominant", "dominant_id"):
        np.testing.assert_array_equal(first[k], again[k], err_msg=k + " differs run to run")
    np.testing.assert_array_equal(first["weight_max"].view(np.uint32), again["weight_max"].view(np.uint32), err_msg="weight_max differs run to run")


def test_any_output_may_be_left_out(gpu_device):
    from fdgs import importance
    scene, ref, wk, excl = cases.oracle("c")
    P, W, H = int(scene["means3D"].shape[0]), int(scene["W"]), int(scene["H"])
    assert not excl.any()
    want = co.reduce(wk, P)
    res = _fwd(scene_to_device(scene, gpu_device))
    full = _fresh(P, W, H, gpu_device)
    for k in full:
        importance.contribution_pass(P, W, H, res[6], res[7], res[8], res[0], **{k: full[k]})
    _check(_np(full), want, "one output per call")
    with pytest.raises(Exception, match="every output is NULL"):
        importance.contribution_pass(P, W, H, res[6], res[7], res[8], res[0])


def _maps(kind, H, W):
    """The two weight maps every case runs with, for a case without flagged pixels: NULL, or the random map with about 30 % zeros."""
    return None if kind == "exclusion" else cases.random_weights(H, W, 11)


@pytest.mark.parametrize("tile_cull", [False, True], ids=["reference-lists", "tile-cull"])
@pytest.mark.parametrize("kind", ["exclusion", "random"])
def test_empty_model(kind, tile_cull, gpu_device):
    from fdgs import importance
    scene = cases.make("a")
    for k in synth.PER_GAUSSIAN_KEYS:
        scene[k] = scene[k][:0].contiguous()
    W, H = int(scene["W"]), int(scene["H"])
    pw = _maps(kind, H, W)
    res = _fwd(scene_to_device(scene, gpu_device), tile_cull=tile_cull)
    out = _np(_pass(res, 0, W, H, pw, gpu_device))
    assert (out["dominant_id"] == -1).all() and out["hits"].size == 0
    model = _Model(scene, gpu_device)
    masks = None if pw is None else [torch.from_numpy(pw).to(gpu_device)]
    st = importance.accumulate(model, [_camera(scene, gpu_device)], _pipe(), scene["bg"].to(gpu_device), masks=masks, tile_cull=tile_cull)
    assert st.P == 0 and st.views == 1
    ids = importance.id_map(model, _camera(scene, gpu_device), _pipe(), scene["bg"].to(gpu_device))
    assert ids.shape == (H, W) and bool((ids == -1).all())


@pytest.mark.parametrize("tile_cull", [False, True], ids=["reference-lists", "tile-cull"])
@pytest.mark.parametrize("kind", ["exclusion", "random"])
def test_camera_that_sees_nothing(kind, tile_cull, gpu_device):
    from fdgs import _capi
    scene = cases.make("a")
    scene["means3D"] = scene["means3D"].clone()
    scene["means3D"][:, 2] -= 100.0     # everything far behind the camera
    P, W, H = int(scene["means3D"].shape[0]), int(scene["W"]), int(scene["H"])
    pw = _maps(kind, H, W)
    _capi.forward_lazy_status(gpu_device, wait=True)
    for lazy in (False, True):      # num_rendered = 0 (nothing is launched), then -1 (the pass walks empty lists)
        res = _fwd(scene_to_device(scene, gpu_device), tile_cull=tile_cull, lazy=lazy)
        assert res[0] in (0, -1)
        out = _fresh(P, W, H, gpu_device)
        out["weight_sum"].fill_(3.0); out["weight_max"].fill_(0.25); out["hits"].fill_(5); out["dominant"].fill_(2)
        got = _np(_pass(res, P, W, H, pw, gpu_device, into=out))
        assert (got["weight_sum"] == 3.0).all() and (got["weight_max"] == 0.25).all() and (got["hits"] == 5).all() and (got["dominant"] == 2).all()
        assert (got["dominant_id"] == -1).all()
    _capi.forward_lazy_status(gpu_device, wait=True)


@pytest.mark.parametrize("name,sparse", [("b", True), ("d", False)], ids=["sparse-lists", "lazy-compact"])
def test_lazy_forwards_with_unknown_num_rendered(name, sparse, gpu_device):
    """The lists of a lazy forward -- num_rendered = -1, compact or at fixed per-tile offsets (ranges (t cap, t cap + n_t)) -- through
    the entry points tests/test_gpu_sparse_lists.py uses."""
    from fdgs import _capi
    scene, ref, wk, excl = cases.oracle(name)
    P, W, H = int(scene["means3D"].shape[0]), int(scene["W"]), int(scene["H"])
    sc = scene_to_device(scene, gpu_device)
    pw = _weights(name, "exclusion", excl, H, W)
    _capi.forward_lazy_status(gpu_device, wait=True)
    first = _fwd(sc, tile_cull=True)          # the waiting forward leaves the run-ahead guess behind
    s0 = _capi.sparse_lists_stats()
    res = _fwd(sc, tile_cull=True, lazy=True, sparse_lists=sparse)
    assert res[0] == -1, "the second forward of a configuration must run ahead"
    got = _pass(res, P, W, H, pw, gpu_device)
    pend, failed, reported = _capi.forward_lazy_status(gpu_device, wait=True)
    assert (pend, failed, reported) == (0, 0, [first[0]])
    s1 = _capi.sparse_lists_stats()
    assert s1[0] - s0[0] == (1 if sparse else 0)
    _check(_np(got), co.reduce(wk, P, pw), name + ("/sparse" if sparse else "/lazy"))


# ---- the Python layer ------------------------------------------------------------------------------------------------------------

class _Model:
    """A model that has only the reference's post-activation getters (the duck type render() reads), holding a scene's tensors as
    they are: what the oracle is given, bit for bit."""

    def __init__(self, scene, dev):
        t = {k: scene[k].to(dev) for k in ("means3D", "opacities", "scales", "rotations", "scales_t", "ts", "rotations_r", "shs")}
        self.get_xyz, self.get_opacity, self.get_scaling, self.get_rotation = t["means3D"], t["opacities"], t["scales"], t["rotations"]
        self.get_scaling_t, self.get_t, self.get_rotation_r, self.get_features = t["scales_t"], t["ts"], t["rotations_r"], t["shs"]
        self.active_sh_degree, self.active_sh_degree_t = scene["sh_degree"], scene["sh_degree_t"]
        self.time_duration = [0.0, scene["time_duration"]]
        self.rot_4d, self.gaussian_dim, self.force_sh_3d = scene["rot_4d"], scene["gaussian_dim"], scene["force_sh_3d"]
        self.prefilter_var = -1.0
        self.env_map = None


def _camera(scene, dev, timestamp=None):
    from fdgs import train_host
    return train_host.SyntheticCamera(scene, dev, timestamp=timestamp)


def _pipe():
    from fdgs import train_host
    return train_host.PipelineFlags()


VIEWS = (("rig0", 0.5), ("rig1", 0.3))   # two cameras at two timestamps


def test_accumulate_over_two_cameras_and_timestamps(gpu_device):
    from fdgs import importance
    per_view = [cases.oracle("a", pose, tf) for pose, tf in VIEWS]
    scene = per_view[0][0]
    P, W, H = int(scene["means3D"].shape[0]), int(scene["W"]), int(scene["H"])
    model = _Model(scene, gpu_device)
    cams = [_camera(s, gpu_device) for s, _r, _w, _e in per_view]
    assert cams[0].timestamp != cams[1].timestamp
    masks, wants = [], []
    for s, ref, wk, excl in per_view:
        assert float(excl.mean()) <= 0.01
        pw = None if not excl.any() else (~excl).astype(np.float32)
        masks.append(None if pw is None else torch.from_numpy(pw).to(gpu_device))
        wants.append(co.reduce(wk, P, pw))
    bg = scene["bg"].to(gpu_device)
    st = importance.accumulate(model, cams[:1], _pipe(), bg, masks=masks[:1])
    assert st.views == 1
    st2 = importance.accumulate(model, cams[1:], _pipe(), bg, masks=masks[1:], stats=st)
    assert st2 is st and st.views == 2 and st.scales.shape == (P, 3)
    got = _np({"weight_sum": st.weight_sum, "weight_max": st.weight_max, "hits": st.hits, "dominant": st.dominant})
    want = {"weight_sum": wants[0]["weight_sum"] + wants[1]["weight_sum"], "weight_max": np.maximum(wants[0]["weight_max"], wants[1]["weight_max"]),
            "hits": wants[0]["hits"] + wants[1]["hits"], "dominant": wants[0]["dominant"] + wants[1]["dominant"]}
    assert not np.array_equal(wants[0]["hits"], wants[1]["hits"])
    got["dominant_id"] = want["dominant_id"] = np.zeros(0)
    _check(got, want, "two views accumulated")
    # both views in one call, tile_cull off: the same statistics
    both = importance.accumulate(model, cams, _pipe(), bg, masks=masks, tile_cull=False)
    assert torch.equal(both.hits, st.hits) and torch.equal(both.dominant, st.dominant) and torch.equal(both.weight_max, st.weight_max)
    # the ID map of the second view
    ids = importance.id_map(model, cams[1], _pipe(), bg).cpu().numpy()
    ok = ~per_view[1][3]
    np.testing.assert_array_equal(ids[ok], per_view[1][2]["dominant_id"][ok])


PRUNE_CFG = synth.SceneConfig("cp", 2500, 96, 64, 1, 0, 0.05, 1.0, True, 4, False)
PRUNE_VIEWS = (("axis", 0.5), ("rig0", 0.35), ("rig1", 0.65))


def _prune_setup(dev):
    from fdgs import train_host
    scenes = [synth.make_scene(PRUNE_CFG, seed=4, pose=pose, timestamp_frac=tf) for pose, tf in PRUNE_VIEWS]
    for s in scenes:
        # Gaussians that no view uses: every 5th too faint to reach alpha = 1/255 anywhere, every 7th outside every frustum
        s["opacities"][::5] = 0.002
        s["means3D"][::7, 0] += 40.0
    model = train_host.GaussianParams(scenes[0], dev)
    opt = train_host.make_optimizer(model)
    g = torch.Generator().manual_seed(2)
    opt.exp_avg.copy_(torch.randn(opt.exp_avg.numel(), generator=g))
    opt.exp_avg_sq.copy_(torch.rand(opt.exp_avg_sq.numel(), generator=g))
    cams = [_camera(s, dev) for s in scenes]
    return scenes, model, opt, cams


def _renders(model, cams, bg):
    from fdgs.fused import render_raw
    with torch.no_grad():
        return [render_raw(c, model, _pipe(), bg)["render"].clone() for c in cams]


def test_prune_what_never_contributes_then_by_fraction(gpu_device):
    from fdgs import harness, importance
    from fdgs.pipeline import StepPipeline
    scenes, model, opt, cams = _prune_setup(gpu_device)
    bg = torch.zeros(3, device=gpu_device)
    P = model.P
    before = _renders(model, cams, bg)
    st = importance.accumulate(model, cams, _pipe(), bg)
    assert st.views == 3
    keep = (st.hits > 0)
    n_keep = int(keep.sum())
    assert 0.2 * P < n_keep < 0.98 * P, n_keep
    old = {n: model.params[n].detach().clone() for n in model.NAMES}
    old_off = dict(model.offsets)
    old_m, old_v = opt.exp_avg.clone(), opt.exp_avg_sq.clone()
    dens = harness.DensificationStats(P, gpu_device, 1)
    dens.denom.copy_(torch.arange(P, device=gpu_device, dtype=torch.float32).unsqueeze(1))
    # a finished model, no optimizer: the same rows by a plain index-select
    from fdgs import train_host
    bare = train_host.GaussianParams(scenes[0], gpu_device)
    bare._bind(model.flat.detach().clone(), torch.zeros_like(model.flat), P)
    bare_st = importance.ContributionStats(P, gpu_device)
    bare_st.weight_sum, bare_st.weight_max, bare_st.hits, bare_st.dominant = (t.clone() for t in (st.weight_sum, st.weight_max, st.hits, st.dominant))
    rep = importance.prune_by_contribution(model, opt, st, min_hits=1, dens_stats=dens)
    assert importance.prune_by_contribution(bare, None, bare_st, min_hits=1) == rep and torch.equal(bare.flat, model.flat) and bare.P == model.P
    assert rep == {"P_old": P, "P_new": n_keep} and model.P == n_keep and st.P == n_keep and bool((st.hits > 0).all())
    for n, rf in zip(model.NAMES, model.row_floats()):
        assert torch.equal(model.params[n].detach(), old[n][keep]), n + ": surviving rows are not the gathered originals"
        b, e = model.offsets[n]
        ob, oe = old_off[n]
        for new, was in ((opt.exp_avg, old_m), (opt.exp_avg_sq, old_v)):
            assert torch.equal(new[b:e].view(n_keep, rf), was[ob:oe].view(P, rf)[keep]), n + ": Adam moments are not the gathered originals"
    assert torch.equal(dens.denom[:, 0], torch.arange(P, device=gpu_device, dtype=torch.float32)[keep]) and dens.max_radii2D.shape[0] == n_keep
    # the pruned model renders the same images wherever, by the oracle, the pixel did not end early (a Gaussian that never
    # contributes can still be the one that ends a pixel)
    after = _renders(model, cams, bg)
    for s, a, b in zip(scenes, before, after):
        ref, _ = run_oracle(s, None, kind="port")
        ok = ~co.walk(ref, int(s["W"]), int(s["H"]))["ended_early"]
        err = float((a - b).abs().cpu().numpy()[:, ok].max())
        print("pruned %d -> %d: max render difference %.3g on %.3f of the pixels" % (P, n_keep, err, ok.mean()))
        assert err <= PIX_TOL, err
    # keep_fraction = 0.5 halves the model, up to ties at the cut
    score = st.score("sum")
    k = -(-n_keep // 2)
    cut = torch.topk(score, k).values[-1]
    want = int((score >= cut).sum())
    rep = importance.prune_by_contribution(model, opt, st, keep_fraction=0.5)
    assert rep["P_new"] == want == model.P and k <= want <= k + int((score == cut).sum()), (rep, k, want)
    # ... and the model trains on
    gts = [b.clone() for b in before[:2]]
    sp = StepPipeline(model, opt)
    flat0 = model.flat.clone()
    results, losses = sp.step(cams[:2], gts, _pipe(), bg)
    torch.cuda.synchronize()
    assert results[0]["radii"].shape[0] == model.P and bool(torch.isfinite(model.flat).all()) and not torch.equal(flat0, model.flat)


def test_training_loop_prunes_at_the_given_iterations(gpu_device):
    from fdgs import harness
    scenes, model, opt, cams = _prune_setup(gpu_device)
    bg = torch.zeros(3, device=gpu_device)
    gts = _renders(model, cams, bg)
    P = model.P
    lines = []
    harness.train(model, opt, cams, gts, _pipe(), bg, iterations=3, batch_size=1, densify_until_iter=0, contribution_prune={2: 0.5},
                  log_every=1, log=lines.append)
    assert -(-P // 2) <= model.P < 0.75 * P and opt.exp_avg.numel() == model.flat.numel()
    assert any("contribution prune: %d -> %d" % (P, model.P) in ln for ln in lines), lines
    assert bool(torch.isfinite(model.flat).all())
