"""CPU: fdgs.checkpoint -- the reference's checkpoint files (tests/golden/checkpoint, written by the reference's own GaussianModel:
tests/golden/make_golden_checkpoint.py) read into GaussianParams / FlatAdam / DensificationStats, our files read by
torch.optim.Adam, interrupted runs, and the resume parameters of the harness."""
import glob
import inspect
import os

import numpy as np
import pytest
import torch

import util  # noqa: F401  (sys.path for the package)
from fdgs import checkpoint, harness, synth, train_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "checkpoint", "*.ckpt")))
IDS = [os.path.basename(p)[:-5] for p in FIXTURES]
CPU = torch.device("cpu")
# the reference's tuple index of every group's tensor (scene/gaussian_model.py:99-136)
TUPLE_AT = {3: {"xyz": 1, "f_dc": 2, "f_rest": 3, "scaling": 4, "rotation": 5, "opacity": 6},
            4: {"xyz": 1, "f_dc": 2, "f_rest": 3, "scaling": 4, "rotation": 5, "opacity": 6, "t": 13, "scaling_t": 14, "rotation_r": 15}}
OURS = dict(checkpoint.GROUPS_3D + checkpoint.GROUPS_4D + checkpoint.GROUP_ROT4D)


def _kw(path):
    d = np.load(path[:-5] + ".npz")
    sh, sh_t, dim, rot, f3d, it = (int(x) for x in d["cfg"])
    return d, dict(sh_degree=sh, sh_degree_t=sh_t, time_duration=[0.0, float(d["duration"][0])], force_sh_3d=bool(f3d)), dim, bool(rot), it


def _group_view(model, flat, gname):
    """The slice of a flat buffer (parameters or moments) that the reference's group ``gname`` holds."""
    pname = OURS[gname]
    b, e = model.offsets[pname]
    return checkpoint._split(gname, flat[b:e].view(model.params[pname].shape))


def test_fixtures_exist():
    assert IDS == ["dim3", "dim4_norot", "rot4d"]


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_restoring_a_reference_checkpoint(path):
    d, kw, dim, rot, it = _kw(path)
    args, saved_it = torch.load(path, map_location="cpu", weights_only=True)
    assert len(args) == (12 if dim == 3 else 19) and saved_it == it
    model, opt, stats, iteration = checkpoint.load(path, CPU, **kw)
    assert iteration == it and model.gaussian_dim == dim and model.rot_4d == rot
    assert (model.max_sh_degree, model.max_sh_degree_t) == (kw["sh_degree"], kw["sh_degree_t"])
    assert model.active_sh_degree == args[0] and model.active_sh_degree_t == (args[18] if dim == 4 else 0)
    assert model.time_duration == kw["time_duration"] and model.force_sh_3d == kw["force_sh_3d"]
    names = [g for g, _ in checkpoint.group_table(dim, rot)]
    assert names == [g["name"] for g in args[10 if dim == 3 else 11]["param_groups"]]
    # parameters: bit for bit the tuple's tensors, _features the concatenation
    for g in names:
        assert torch.equal(_group_view(model, model.flat.detach(), g), args[TUPLE_AT[dim][g]].detach()), g
    assert torch.equal(model.get_features.detach(), torch.cat((args[2], args[3]), 1).detach())
    assert model.M == args[2].shape[1] + args[3].shape[1]
    if dim == 4 and not rot:   # allocated all the same, a unit quaternion
        assert torch.equal(model.params["_rotation_r"].detach(), torch.tensor([1.0, 0, 0, 0]).expand(model.P, 4))
    # statistics
    assert torch.equal(stats.max_radii2D, args[7]) and torch.equal(stats.xyz_gradient_accum, args[8])
    assert torch.equal(stats.denom, args[9 if dim == 3 else 10]) and float(stats.denom.sum()) > 0
    if dim == 4:
        assert torch.equal(stats.t_gradient_accum, args[9]) and float(args[9].abs().sum()) > 0
    # optimizer: step count, moments, learning rates from the file
    od = args[10 if dim == 3 else 11]
    assert opt.step_count == 2 and opt.betas == (0.9, 0.999) and opt.eps == 1e-15
    seg = {s["name"]: s for s in opt.named_segments()}
    for k, g in enumerate(od["param_groups"]):
        assert torch.equal(_group_view(model, opt.exp_avg, g["name"]), od["state"][k]["exp_avg"]), g["name"]
        assert torch.equal(_group_view(model, opt.exp_avg_sq, g["name"]), od["state"][k]["exp_avg_sq"]), g["name"]
        s = seg[OURS[g["name"]]]
        assert (s["lr_head"] if g["name"] == "f_dc" else s["lr"]) == g["lr"], g["name"]
    assert seg["_xyz"]["lr"] == 1.234e-4   # the run's current xyz rate, not training_setup's initial one
    # one step with the recorded gradients against the reference's restore() + optimizer.step().  Tolerance: the absolute 1e-6 of
    # tests/test_gpu_loss.py::test_fused_adam_matches_torch_adam (FlatAdam against torch.optim.Adam; five steps there, one here)
    for g in names:
        _group_view(model, model.flat_grad, g).copy_(torch.from_numpy(d["grad." + g]))
    before = model.flat.detach().clone()
    opt.step()
    assert opt.step_count == 3
    for g in names:
        got, want = _group_view(model, model.flat.detach(), g), torch.from_numpy(d["after." + g])
        err = float((got - want).abs().max())
        assert err <= 1e-6, (g, err)
        assert float((got - _group_view(model, before, g)).abs().max()) > 1e-5, g   # it did move


def _scene_model(cfg, seed=0, alloc=None):
    scene = synth.make_scene(cfg, seed=seed, alloc=alloc)
    m = train_host.GaussianParams(scene, CPU)
    return scene, m, train_host.FlatAdam(m)


CONFIGS = {"rot4d": (synth.SceneConfig("k", 40, 32, 32, 3, 1, 0.05, 10.0, True, 4, False), (3, 2)),
           "dim4_norot": (synth.SceneConfig("k", 40, 32, 32, 1, 0, 0.05, 1.0, False, 4, True), (2, 0)),
           "dim3": (synth.SceneConfig("k", 40, 32, 32, 2, 0, 0.05, 1.0, False, 3, False), (2, 0))}


def _restore_kw(cfg, alloc):
    return dict(sh_degree=alloc[0], sh_degree_t=alloc[1], time_duration=[0.0, cfg.duration], force_sh_3d=cfg.force_sh_3d)


def _present(model):
    """The parameter tensors the reference's model has (the others are allocated here and never trained)."""
    return sorted({p for _, p in checkpoint.group_table(model.gaussian_dim, model.rot_4d)})


def _fixed_steps(model, opt, gen, n):
    for _ in range(n):
        model.flat_grad.zero_()
        for p in _present(model):
            model.params[p].grad.copy_(1e-3 * torch.randn(model.params[p].shape, generator=gen))
        opt.step()


def _equal_entries(a, b, path=""):
    assert type(a) is type(b), (path, type(a), type(b))
    if isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), path
    elif isinstance(a, dict):
        assert list(a.keys()) == list(b.keys()), path
        for k in a:
            _equal_entries(a[k], b[k], "%s[%r]" % (path, k))
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), path
        for k, (x, y) in enumerate(zip(a, b)):
            _equal_entries(x, y, "%s[%d]" % (path, k))
    else:
        assert a == b, (path, a, b)


@pytest.mark.parametrize("tag", sorted(CONFIGS))
def test_capture_restore_capture_round_trip(tag):
    cfg, alloc = CONFIGS[tag]
    scene, m, o = _scene_model(cfg, seed=5, alloc=alloc)
    gen = torch.Generator().manual_seed(1)
    _fixed_steps(m, o, gen, 2)
    o.set_lr("_xyz", 7.5e-5)
    st = harness.DensificationStats(m.P, CPU)
    st.max_radii2D.copy_(torch.randint(0, 30, (m.P,), generator=gen).float())
    st.denom.copy_(torch.randint(0, 4, (m.P, 1), generator=gen).float())
    st.xyz_gradient_accum.copy_(torch.rand(m.P, 1, generator=gen))
    st.t_gradient_accum.copy_(torch.rand(m.P, 1, generator=gen))
    if tag == "rot4d":
        m.env_map = torch.rand(3, 8, 8, generator=gen)
    a = checkpoint.capture(m, o, st, spatial_lr_scale=2.5)
    assert len(a) == (12 if cfg.gaussian_dim == 3 else 19)
    od = a[10 if cfg.gaussian_dim == 3 else 11]
    want = ["xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"] + (["t", "scaling_t"] if cfg.gaussian_dim == 4 else []) + (
        ["rotation_r"] if cfg.rot_4d else [])
    assert [g["name"] for g in od["param_groups"]] == want and [g["params"] for g in od["param_groups"]] == [[k] for k in range(len(want))]
    lrs = {g["name"]: g["lr"] for g in od["param_groups"]}
    assert lrs["xyz"] == 7.5e-5 and lrs["f_dc"] == 2.5e-3 and lrs["f_rest"] == 2.5e-3 / 20.0 and lrs["opacity"] == 5e-2
    assert a[2].shape == (m.P, 1, 3) and a[3].shape == (m.P, m.M - 1, 3) and all(float(s["step"]) == 2.0 for s in od["state"].values())
    # detached clones: nothing aliases the flat bucket or the moments
    keep = a[1].clone()
    m.flat.detach().add_(1.0)
    o.exp_avg.add_(1.0)
    assert torch.equal(a[1], keep) and not a[1].requires_grad
    m2, o2, st2 = checkpoint.restore(a, CPU, **_restore_kw(cfg, alloc))
    b = checkpoint.capture(m2, o2, st2, spatial_lr_scale=2.5)
    _equal_entries(a, b)
    assert (m2.active_sh_degree, m2.active_sh_degree_t) == (cfg.sh_degree, cfg.sh_degree_t)
    # without an optimizer (the reference's training_args = None)
    m3, o3, st3 = checkpoint.restore(a, CPU, with_optimizer=False, **_restore_kw(cfg, alloc))
    assert o3 is None and torch.equal(m3.flat, m2.flat) and torch.equal(st3.denom, st.denom)


def test_our_file_loads_into_the_reference_optimizer(tmp_path):
    cfg, alloc = CONFIGS["rot4d"]
    scene, m, o = _scene_model(cfg, seed=6, alloc=alloc)
    _fixed_steps(m, o, torch.Generator().manual_seed(2), 3)
    path = str(tmp_path / "chkpnt7.pth")
    checkpoint.save(path, m, o, 7)
    m2, o2, st2, it = checkpoint.load(path, CPU, **_restore_kw(cfg, alloc))
    assert it == 7 and torch.equal(m2.flat, m.flat) and torch.equal(o2.exp_avg_sq, o.exp_avg_sq) and o2.step_count == 3
    assert float(st2.denom.abs().sum()) == 0.0 and st2.max_radii2D.shape == (m.P,)
    # the reference's side: training_setup's nine groups (scene/gaussian_model.py:336-353) over the file's tensors, load_state_dict
    args, _ = torch.load(path, map_location="cpu", weights_only=True)
    at = TUPLE_AT[4]
    groups = [{"params": [torch.nn.Parameter(args[at[g]].clone())], "lr": 123.0, "name": g}
              for g in ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "t", "scaling_t", "rotation_r")]
    ref = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    ref.load_state_dict(args[11])
    for grp in ref.param_groups:
        st = ref.state[grp["params"][0]]
        assert float(st["step"]) == 3.0
        assert torch.equal(st["exp_avg"], _group_view(m, o.exp_avg, grp["name"])), grp["name"]
        assert torch.equal(st["exp_avg_sq"], _group_view(m, o.exp_avg_sq, grp["name"])), grp["name"]
    assert [g["lr"] for g in ref.param_groups] == [1.6e-4, 2.5e-3, 2.5e-3 / 20.0, 5e-2, 5e-3, 1e-3, 1.6e-4, 5e-3, 1e-3]
    for grp in ref.param_groups:   # and it steps
        grp["params"][0].grad = torch.ones_like(grp["params"][0])
    ref.step()


@pytest.mark.parametrize("tag", sorted(CONFIGS))
def test_interrupted_run_equals_straight_run(tag, tmp_path):
    cfg, alloc = CONFIGS[tag]
    _, ma, oa = _scene_model(cfg, seed=7, alloc=alloc)
    _fixed_steps(ma, oa, torch.Generator().manual_seed(3), 4)
    _, mb, ob = _scene_model(cfg, seed=7, alloc=alloc)
    gen = torch.Generator().manual_seed(3)
    _fixed_steps(mb, ob, gen, 2)
    path = str(tmp_path / "half.pth")
    checkpoint.save(path, mb, ob, 2)
    mc, oc, _, it = checkpoint.load(path, CPU, **_restore_kw(cfg, alloc))
    assert it == 2 and oc.step_count == 2
    _fixed_steps(mc, oc, gen, 2)
    for p in _present(ma):
        assert torch.equal(mc.params[p].detach(), ma.params[p].detach()), p
    for gname in [g for g, _ in checkpoint.group_table(cfg.gaussian_dim, cfg.rot_4d)]:
        assert torch.equal(_group_view(mc, oc.exp_avg, gname), _group_view(ma, oa.exp_avg, gname)), gname
        assert torch.equal(_group_view(mc, oc.exp_avg_sq, gname), _group_view(ma, oa.exp_avg_sq, gname)), gname
    assert oc.step_count == oa.step_count == 4


def test_frame_shard_started_at_batch_n():
    sh = harness.FrameShard(23, 2, 2, 1, seed=5)
    nb = sh.batches_per_epoch()
    assert nb == 5
    it = iter(sh)
    whole = [next(it) for _ in range(3 * nb + 2)]
    assert whole[:nb] == sh.epoch(0) and whole[nb:2 * nb] == sh.epoch(1)
    for n in (0, 1, nb - 1, nb, nb + 3, 2 * nb, 3 * nb + 1):    # inside an epoch, at and across its boundary
        it = sh.iter_from(n)
        assert [next(it) for _ in range(3 * nb + 2 - n)] == whole[n:], n
    with pytest.raises(ValueError, match="start"):
        next(sh.iter_from(-1))


def test_train_has_resume_parameters_that_default_to_the_old_behaviour():
    sig = inspect.signature(harness.train)
    p = sig.parameters
    assert p["start_iteration"].default == 0 and p["stats"].default is None
    assert tuple(p["save_iterations"].default) == () and p["on_save"].default is None
    # the parameters that were there keep their order and defaults: the new ones come last
    names = list(p)
    assert names[-4:] == ["start_iteration", "stats", "save_iterations", "on_save"] and names[names.index("on_evaluate") + 1] == "start_iteration"
    assert names[:8] == ["model", "optimizer", "cameras", "gts", "pipe", "bg", "iterations", "batch_size"]
    assert p["spatial_order"].default is True and p["batch_size"].default == 4


def test_error_cases():
    cfg, alloc = CONFIGS["rot4d"]
    scene, m, o = _scene_model(cfg, seed=8, alloc=alloc)
    _fixed_steps(m, o, torch.Generator().manual_seed(4), 1)
    a = checkpoint.capture(m, o)
    kw = _restore_kw(cfg, alloc)
    with pytest.raises(ValueError, match="12 .3D. or 19 .4D. entries"):
        checkpoint.restore(a[:-1], CPU, **kw)
    with pytest.raises(ValueError, match="SH coefficients"):
        checkpoint.restore(a, CPU, **dict(kw, sh_degree_t=1))           # M = 48 is (3, 2); (3, 1) allocates 32
    with pytest.raises(ValueError, match="SH coefficients"):
        checkpoint.restore(a, CPU, **dict(kw, force_sh_3d=True))        # 16
    with pytest.raises(ValueError, match="beyond the maximal"):
        checkpoint.restore((5,) + a[1:], CPU, **kw)
    a[11]["state"][4]["step"] = torch.tensor(9.0)
    with pytest.raises(ValueError, match="steps differ.*scaling = 9"):
        checkpoint.restore(a, CPU, **kw)
    c3, al3 = CONFIGS["dim3"]
    _, m3, o3 = _scene_model(c3, seed=8, alloc=al3)
    with pytest.raises(ValueError, match="4D model"):
        checkpoint.restore(checkpoint.capture(m3, o3), CPU, **dict(_restore_kw(c3, al3), force_sh_3d=True))
    # a model that never stepped: an optimizer state without moments, step 0
    a3 = checkpoint.capture(m3, o3)
    assert a3[10]["state"] == {} and len(a3) == 12
    _, o4, _ = checkpoint.restore(a3, CPU, **_restore_kw(c3, al3))
    assert o4.step_count == 0 and float(o4.exp_avg.abs().sum()) == 0.0
