"""What the flat-bucket model says about its own layout, as plain JSON data: shared by tests/golden/make_golden_model_layout.py (which
records it from the commit BEFORE a change to the model's description) and tests/test_model_layout_host.py (which holds the package to
the record).  Only names that exist on both sides of such a change are used.  CPU only."""
import hashlib

import torch

import util  # noqa: F401  (sys.path for the package)
from fdgs import checkpoint, compress, optim, synth, train_host

CPU = torch.device("cpu")
P = 5
# name -> (config, gaussian_dim, rot_4d): M = 1, 16 and 48
MODES = {"3d_M1": synth.SceneConfig("k", P, 32, 32, 0, 0, 0.05, 1.0, False, 3, False),
         "4d_M16": synth.SceneConfig("k", P, 32, 32, 3, 0, 0.05, 1.0, False, 4, False),
         "rot4d_M48": synth.SceneConfig("k", P, 32, 32, 3, 2, 0.05, 10.0, True, 4, False)}


def _groups(param_groups):
    return [[g["name"], float(g["lr"])] for g in param_groups]


def _home_shapes(scene):
    """fdgs.optim.Adam's homing of a reference-style model: per group the shapes of the (data, grad, exp_avg, exp_avg_sq) views and
    where the data view starts in the bucket."""
    ref = train_host.ReferenceStyleModel(scene, CPU, optimizer="fdgs")
    ref.optimizer._home()
    return {g: dict(shapes=[list(t.shape) for t in v], offset=v[0].storage_offset(), stride=list(v[0].stride()))
            for g, v in ref.optimizer._views.items()}


def _from_raw_sha(M):
    """``from_raw`` with ``_t`` / ``_scaling_t`` / ``_rotation_r`` missing: the placeholders are part of the bucket."""
    ramp = lambda *shape: (torch.arange(int(torch.tensor(shape).prod()), dtype=torch.float32) * 0.125 - 1.0).reshape(shape)  # noqa: E731
    raw = {"_xyz": ramp(P, 3), "_features": ramp(P, M, 3), "_opacity": ramp(P, 1), "_scaling": ramp(P, 3), "_rotation": ramp(P, 4)}
    m = train_host.GaussianParams.from_raw(raw, CPU, max_sh_degree=0, gaussian_dim=3)
    return hashlib.sha256(m.flat.detach().numpy().tobytes()).hexdigest()


def record():
    out = {"compress.SEGMENTS": [list(s) for s in compress.SEGMENTS], "modes": {}}
    for mode, cfg in MODES.items():
        scene = synth.make_scene(cfg, seed=0)
        m = train_host.GaussianParams(scene, CPU)
        opt = train_host.FlatAdam(m)
        ref = train_host.ReferenceStyleModel(scene, CPU)
        out["modes"][mode] = {
            "M": m.M,
            "offsets": {n: list(m.offsets[n]) for n in m.NAMES},
            "row_floats": list(m.row_floats()),
            "lr_segments": m.lr_segments(),
            "grad_sink": {k: [g.storage_offset(), list(g.shape)] for k, g in m.grad_sink().items()},
            "geometry_adam_lr": opt.geometry_adam()["lr"],
            "capture_groups": _groups(checkpoint.capture(m, opt)[11 if cfg.gaussian_dim == 4 else 10]["param_groups"]),
            "capture_groups_no_optimizer": _groups(checkpoint.capture(m, None)[11 if cfg.gaussian_dim == 4 else 10]["param_groups"]),
            "home": _home_shapes(scene),
            "group_table": [list(g) for g in checkpoint.group_table(cfg.gaussian_dim, cfg.rot_4d)],
            "reference_style_groups": [[g["name"], float(g["lr"]), list(g["params"][0].shape)] for g in ref.optimizer.param_groups],
            "from_raw_sha256": _from_raw_sha(m.M),
        }
    return out
