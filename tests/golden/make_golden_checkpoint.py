"""Golden fixtures for checkpoints, produced by the REFERENCE's own ``GaussianModel`` (scene/gaussian_model.py) on the CPU of the
build container: ``capture()`` written as the reference's trainer writes it (train.py:224-228), and what the reference's own
``restore()`` followed by one ``optimizer.step()`` makes of it.  The module's CUDA-only imports are stubbed and ``device="cuda"`` is
redirected to the CPU, as in make_golden_densify.py.

    python tests/golden/make_golden_checkpoint.py   ->   tests/golden/checkpoint/<tag>.ckpt, <tag>.npz

<tag>.ckpt  torch.save((g.capture(), iteration)) after two Adam steps; the accumulators hold random statistics
            (the reference names its files chkpnt<iteration>.pth; the fixtures carry another suffix because a ``.pth`` file in a source
            tree reads as one of Python's path-configuration files -- torch.load does not look at the name)
<tag>.npz   grad.<group>   a fixed gradient per parameter group
            after.<group>  the parameters after GaussianModel(...).restore(model_args, training_args) and ONE optimizer.step() with
                           those gradients -- ``training_args`` with learning rates that differ from the saved ones, so that a
                           loader which takes them from anywhere but the file shows
            cfg            sh_degree, sh_degree_t, gaussian_dim, rot_4d, force_sh_3d, iteration;  duration

The reference's ``restore`` reads ``t_gradient_accum`` for every model and therefore raises for a 3D one when ``training_args`` is
given (scene/gaussian_model.py:172-177); for the 3D fixture its remaining lines (training_setup, the accumulators,
``optimizer.load_state_dict``) are carried out here one by one.
"""
import os, sys, types
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

for name in ("pointops2", "pointops2.functions", "pointops2.functions.pointops", "simple_knn", "simple_knn._C", "plyfile"):
    sys.modules[name] = types.ModuleType(name)
sys.modules["pointops2.functions.pointops"].furthestsampling = None
sys.modules["pointops2.functions.pointops"].knnquery = None
sys.modules["simple_knn._C"].distCUDA2 = None
sys.modules["plyfile"].PlyData = None
sys.modules["plyfile"].PlyElement = None
sys.path.insert(0, "/root/reference")


def _cpu(fn):
    def wrapped(*a, **k):
        if k.get("device", None) is not None and str(k["device"]).startswith("cuda"):
            k["device"] = "cpu"
        return fn(*a, **k)
    return wrapped


for fname in ("zeros", "ones", "empty", "tensor", "full", "rand", "randn"):
    setattr(torch, fname, _cpu(getattr(torch, fname)))

import importlib.util  # noqa: E402
_spec = importlib.util.spec_from_file_location("ref_gaussian_model", "/root/reference/scene/gaussian_model.py")
_mod = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_mod)   # the reference module itself (scene/__init__.py would pull in the dataset readers)
GaussianModel = _mod.GaussianModel
from fdgs import synth  # noqa: E402

OUT = os.path.join(HERE, "checkpoint")


def training_args(scale=1.0):
    return types.SimpleNamespace(percent_dense=0.01, position_lr_init=1.6e-4 * scale, position_lr_final=1.6e-6, position_lr_delay_mult=0.01,
                                 position_lr_max_steps=30000, feature_lr=2.5e-3 * scale, opacity_lr=0.05 * scale, scaling_lr=5e-3 * scale,
                                 rotation_lr=1e-3 * scale, position_t_lr_init=-1.0)


def run(tag, cfg, alloc, seed, iteration, warm_steps=2):
    scene = synth.make_scene(cfg, seed=seed, alloc=alloc)
    P = scene["means3D"].shape[0]
    kw = dict(sh_degree=alloc[0], gaussian_dim=cfg.gaussian_dim, time_duration=[0.0, scene["time_duration"]], rot_4d=cfg.rot_4d,
              force_sh_3d=cfg.force_sh_3d, sh_degree_t=alloc[1])
    g = GaussianModel(**kw)
    assert g.get_max_sh_channels == scene["M"], (g.get_max_sh_channels, scene["M"])
    nn = torch.nn
    inv_sig = lambda x: torch.log(x / (1 - x))
    g._xyz = nn.Parameter(scene["means3D"].clone().requires_grad_(True))
    g._features_dc = nn.Parameter(scene["shs"][:, :1].clone().contiguous().requires_grad_(True))
    g._features_rest = nn.Parameter(scene["shs"][:, 1:].clone().contiguous().requires_grad_(True))
    g._opacity = nn.Parameter(inv_sig(scene["opacities"].clamp(1e-6, 1 - 1e-6)).requires_grad_(True))
    g._scaling = nn.Parameter(torch.log(scene["scales"]).requires_grad_(True))
    g._rotation = nn.Parameter(scene["rotations"].clone().requires_grad_(True))
    if cfg.gaussian_dim == 4:
        g._t = nn.Parameter(scene["ts"].clone().requires_grad_(True))
        g._scaling_t = nn.Parameter(torch.log(scene["scales_t"]).requires_grad_(True))
        if cfg.rot_4d:
            g._rotation_r = nn.Parameter(scene["rotations_r"].clone().requires_grad_(True))
    g.active_sh_degree, g.active_sh_degree_t = cfg.sh_degree, cfg.sh_degree_t
    g.spatial_lr_scale = 1.0
    g.training_setup(training_args())
    gen = torch.Generator().manual_seed(2000 + seed)
    for _ in range(warm_steps):  # populate Adam's exp_avg / exp_avg_sq
        for grp in g.optimizer.param_groups:
            p = grp["params"][0]
            p.grad = 1e-3 * torch.randn(p.shape, generator=gen)
        g.optimizer.step()
    for grp in g.optimizer.param_groups:   # the xyz learning rate of a run in progress (update_learning_rate)
        if grp["name"] == "xyz":
            grp["lr"] = 1.234e-4
    g.max_radii2D = torch.randint(0, 40, (P,), generator=gen).float()
    g.denom = torch.randint(0, 5, (P, 1), generator=gen).float()
    g.xyz_gradient_accum = torch.rand(P, 1, generator=gen) * g.denom * 8e-4
    if cfg.gaussian_dim == 4:
        g.t_gradient_accum = torch.rand(P, 1, generator=gen) * g.denom * 1e-4
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, tag + ".ckpt")
    torch.save((g.capture(), iteration), path)

    # the reference's way back (train.py:50-52), with other learning rates in training_args than the file holds
    model_args, first_iter = torch.load(path, weights_only=False)
    h = GaussianModel(**kw)
    other = training_args(scale=3.0)
    if cfg.gaussian_dim == 4:
        h.restore(model_args, other)
    else:
        h.restore(model_args, None)
        h.training_setup(other)
        h.xyz_gradient_accum, h.denom = model_args[8], model_args[9]
        h.optimizer.load_state_dict(model_args[10])
    assert first_iter == iteration
    out = {}
    for grp in h.optimizer.param_groups:
        p = grp["params"][0]
        p.grad = 1e-3 * torch.randn(p.shape, generator=gen)
        out["grad." + grp["name"]] = p.grad.numpy().copy()
    h.optimizer.step()
    for grp in h.optimizer.param_groups:
        out["after." + grp["name"]] = grp["params"][0].detach().numpy().copy()
    out["cfg"] = np.array([alloc[0], alloc[1], cfg.gaussian_dim, int(cfg.rot_4d), int(cfg.force_sh_3d), iteration], dtype=np.int64)
    out["duration"] = np.array([scene["time_duration"]], dtype=np.float64)
    np.savez_compressed(os.path.join(OUT, tag + ".npz"), **out)
    print(tag, "P %d M %d, %d groups, %d bytes" % (P, scene["M"], len(h.optimizer.param_groups), os.path.getsize(path)))


SC = synth.SceneConfig
# active degrees below the allocated ones where the model has a ramp: the state of a run in progress
run("rot4d", SC("c", 48, 64, 48, 3, 1, 0.05, 10.0, True, 4, False), (3, 2), 1, 4000)
run("dim4_norot", SC("c", 48, 64, 48, 1, 0, 0.05, 1.0, False, 4, True), (1, 0), 2, 700)
run("dim3", SC("c", 48, 64, 48, 1, 0, 0.05, 1.0, False, 3, False), (2, 0), 3, 1500)
