"""The flat bucket, stated once: which parameter tensors a model has, in which order they lie in ``GaussianParams.flat``, and every
name each of them goes by -- the reference's param groups, the kernels' arguments, the gradient sinks.  Everything else in the package
derives its view of the model from ``SEGMENTS``; a new segment is a new row here.  No kernels, no ``GaussianParams``: plain data."""
import math
from collections import namedtuple

import torch

M_ = None                                          # in a trailing shape: the model's SH coefficients per Gaussian
ALWAYS, DIM4, ROT4D = "always", "gaussian_dim == 4", "rot_4d"   # when a mode READS a segment (the bucket always holds all of them)
IDENTITY_Q = (1.0, 0.0, 0.0, 0.0)

# name: our attribute (the reference's, scene/gaussian_model.py:70-80).  tail: a row's shape.  groups: the reference's param group(s),
# several = the row is cut after ``head`` floats (f_dc | f_rest).  kernel / sink: the rasterizer's argument and gradient names.
# lr: arguments/__init__.py:84-92 at spatial_lr_scale = 1, one per group.  fill: a placeholder's row (None: zeros).
Segment = namedtuple("Segment", "name tail groups kernel sink lr fill when head", defaults=(None, ALWAYS, 0))

# ORDER IS LOAD-BEARING: the small geometry tensors first (17 floats per Gaussian), the SH coefficients last (3 M): the two parts are
# final at different moments of a backward pass and are all-reduced separately (allreduce_and_step); fdgs_densify_gather walks them so
SEGMENTS = (
    Segment("_xyz", (3,), ("xyz",), "means3D", "dL_dmeans3D", (1.6e-4,)),
    Segment("_opacity", (1,), ("opacity",), "opacities", "dL_dopacity", (5e-2,)),
    Segment("_scaling", (3,), ("scaling",), "scales", "dL_dscales", (5e-3,)),
    Segment("_rotation", (4,), ("rotation",), "rotations", "dL_drotations", (1e-3,)),
    Segment("_t", (1,), ("t",), "ts", "dL_dts", (1.6e-4,), when=DIM4),
    Segment("_scaling_t", (1,), ("scaling_t",), "scales_t", "dL_dscales_t", (5e-3,), when=DIM4),
    Segment("_rotation_r", (4,), ("rotation_r",), "rotations_r", "dL_drotations_r", (1e-3,), fill=IDENTITY_Q, when=ROT4D),
    Segment("_features", (M_, 3), ("f_dc", "f_rest"), "shs", "dL_dsh", (2.5e-3, 2.5e-3 / 20.0), head=3),
)
assert SEGMENTS[-1].name == "_features"
NAMES = tuple(s.name for s in SEGMENTS)
GEOMETRY = SEGMENTS[:-1]
BY_NAME = {s.name: s for s in SEGMENTS}
BY_KERNEL = {s.kernel: s for s in SEGMENTS}
BY_GROUP = {g: s for s in SEGMENTS for g in s.groups}
# the attribute a reference-style model keeps each group's tensor under: our name, _features_dc / _features_rest for the two SH groups
GROUP_ATTR = {g: s.name if len(s.groups) == 1 else s.name + g[1:] for g, s in BY_GROUP.items()}
GROUP_LR = {g: lr for s in SEGMENTS for g, lr in zip(s.groups, s.lr)}
# what a model is besides its tensors: the keywords of GaussianParams.apply_settings / from_raw (settings_of reads them back)
SETTINGS = ("max_sh_degree", "max_sh_degree_t", "active_sh_degree", "active_sh_degree_t", "time_duration", "rot_4d", "gaussian_dim",
            "force_sh_3d", "prefilter_var")


def tail(seg, M):
    return tuple(int(M) if d is M_ else d for d in seg.tail)


def shapes(P, M):
    return {s.name: (int(P),) + tail(s, M) for s in SEGMENTS}


def row_floats(M):
    """floats per Gaussian of every segment, in bucket order"""
    return [math.prod(tail(s, M)) for s in SEGMENTS]


def used(gaussian_dim, rot_4d):
    """The segments a mode reads, in bucket order: a 3D model's time columns and ``_rotation_r`` without ``rot_4d`` are placeholders."""
    four = int(gaussian_dim) == 4
    return tuple(s.name for s in SEGMENTS if s.when == ALWAYS or (four and (s.when == DIM4 or bool(rot_4d))))


def group_table(gaussian_dim, rot_4d):
    """``training_setup``'s parameter groups as (group, our tensor), in its order (scene/gaussian_model.py:336-353): the SH groups
    come right after xyz there."""
    live = used(gaussian_dim, rot_4d)
    return tuple((g, s.name) for s in (SEGMENTS[0], SEGMENTS[-1]) + SEGMENTS[1:-1] if s.name in live for g in s.groups)


def placeholder_(dst, name):
    """Fills a segment no tensor was given for with what ``create_from_pcd`` starts from: t = 0, log-scale 0, the identity quaternion."""
    fill = BY_NAME[name].fill
    if fill is None:
        dst.zero_()
    else:
        dst.copy_(torch.tensor(fill, dtype=dst.dtype, device=dst.device).expand_as(dst))


def segment(buf, model, name):
    """Segment ``name`` of a flat buffer laid out like ``model.flat`` (the parameters, the gradients, an Adam moment), shaped."""
    b, e = model.offsets[name]
    return buf[b:e].view(model.params[name].shape)


def group_view(t, group):
    """A tensor of ours as the reference's ``group`` sees it: itself, or the head / the rest of every ``_features`` row."""
    groups = BY_GROUP[group].groups
    if len(groups) == 1:
        return t
    return t[:, :1, :] if group == groups[0] else t[:, 1:, :]


def settings_of(model):
    """The keyword dict ``GaussianParams.from_raw`` takes, read from any duck-typed model (one without maximal degrees: the active ones)."""
    return dict(max_sh_degree=int(getattr(model, "max_sh_degree", model.active_sh_degree)),
                max_sh_degree_t=int(getattr(model, "max_sh_degree_t", model.active_sh_degree_t)),
                active_sh_degree=int(model.active_sh_degree), active_sh_degree_t=int(model.active_sh_degree_t),
                time_duration=(float(model.time_duration[0]), float(model.time_duration[1])), rot_4d=bool(model.rot_4d),
                gaussian_dim=int(model.gaussian_dim), force_sh_3d=bool(model.force_sh_3d), prefilter_var=float(model.prefilter_var))


def raw_of(model):
    """The raw tensors ``GaussianParams.from_raw`` takes, detached, from any duck-typed model: the four every mode has, ``_features``
    from ``get_features`` where there is one, and whichever of the others the model holds non-empty."""
    P = int(model._xyz.shape[0])
    feats = model.get_features if hasattr(model, "get_features") else model._features
    raw = {}
    for s in SEGMENTS:
        t = feats if s is SEGMENTS[-1] else getattr(model, s.name, None)
        if s.when == ALWAYS:
            raw[s.name] = t.detach().reshape(P, 1) if s.name == "_opacity" else t.detach()
        elif t is not None and t.numel() > 0:
            raw[s.name] = t.detach().reshape((P,) + s.tail)
    return raw
