"""Checkpoints in the reference's layout: save, resume, and load a model trained with the reference.

The reference saves ``torch.save((gaussians.capture(), iteration), path)`` (train.py:224-228, scene/__init__.py:91-92) and resumes
with ``torch.load`` + ``gaussians.restore(model_args, training_args)`` (train.py:50-52).  ``capture()`` is a plain tuple
(scene/gaussian_model.py:99-136), 12 entries for a 3D model and 19 for a 4D one:

    3D: active_sh_degree, _xyz, _features_dc, _features_rest, _scaling, _rotation, _opacity, max_radii2D, xyz_gradient_accum, denom,
        optimizer.state_dict(), spatial_lr_scale
    4D: active_sh_degree, _xyz, _features_dc, _features_rest, _scaling, _rotation, _opacity, max_radii2D, xyz_gradient_accum,
        t_gradient_accum, denom, optimizer.state_dict(), spatial_lr_scale, _t, _scaling_t, _rotation_r, rot_4d, env_map,
        active_sh_degree_t

``capture`` / ``restore`` here write and read exactly that tuple from / into ``GaussianParams`` + ``FlatAdam`` +
``harness.DensificationStats``: the one ``_features`` tensor is split into ``_features_dc`` [P, 1, 3] and ``_features_rest``
[P, M - 1, 3], the flat moments are sliced into a ``torch.optim.Adam.state_dict()`` with the reference's groups in
``training_setup``'s order (:336-353: xyz, f_dc, f_rest, opacity, scaling, rotation[, t, scaling_t[, rotation_r]]).  What the
reference passes to ``GaussianModel(...)`` instead of saving it -- the maximal SH degrees, ``time_duration``, ``force_sh_3d``,
``prefilter_var`` -- is passed to ``restore`` / ``load`` the same way.  Everything works on the CPU as well as on the GPU.

``ReferenceStyleModel`` (the drop-in model of the benchmark's baseline leg) keeps separate parameters and a per-parameter optimizer;
it has no ``capture`` / ``restore`` of its own: its optimizer's ``state_dict()`` already is the reference's.
"""
from typing import Optional, Tuple

import torch

from .layout import group_table, group_view, segment

# the reference's group name -> our parameter tensor, as fdgs.layout has it, under the names this module has always exported
GROUPS_3D = group_table(3, False)
GROUPS_4D = group_table(4, False)[len(GROUPS_3D):]
GROUP_ROT4D = group_table(4, True)[len(GROUPS_3D) + len(GROUPS_4D):]
_split = lambda name, t: group_view(t, name)  # noqa: E731
from .train_host import FlatAdam, GaussianParams


def reference_sh_channels(sh_degree: int, sh_degree_t: int, gaussian_dim: int, force_sh_3d: bool) -> int:
    """``GaussianModel.get_max_sh_channels`` (scene/gaussian_model.py:222-228, utils/sh_utils.py:56)."""
    if gaussian_dim == 3 or force_sh_3d:
        return (sh_degree + 1) ** 2
    if sh_degree_t == 0:
        return [1, 6, 16, 33][sh_degree]
    return (sh_degree + 1) ** 2 * (sh_degree_t + 1)


def capture(model: GaussianParams, optimizer: Optional[FlatAdam], stats=None, spatial_lr_scale: float = 1.0) -> tuple:
    """The reference's ``GaussianModel.capture()`` tuple of ``model`` / ``optimizer`` / ``stats`` (module docstring).  ``stats``: the
    run's ``harness.DensificationStats`` (None: zeros of the reference's shapes).  ``optimizer`` None: an optimizer state without
    moments (what ``torch.optim.Adam`` holds before its first step).  Every tensor is a detached clone: the tuple does not alias the
    flat bucket, saving it later saves what was captured."""
    P, dev = model.P, model.flat.device
    p = {n: model.params[n].detach() for n in model.NAMES}
    clone = lambda t: t.detach().clone().contiguous()  # noqa: E731
    zeros = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
    table = group_table(model.gaussian_dim, model.rot_4d)

    seg = {s["name"]: s for s in optimizer.named_segments()} if optimizer is not None else {
        s_name: dict(lr=s["lr"], lr_head=s["lr_head"]) for s_name, s in zip(model.NAMES, model.lr_segments())}
    betas, eps = (optimizer.betas, optimizer.eps) if optimizer is not None else ((0.9, 0.999), 1e-15)
    groups, state = [], {}
    for k, (gname, pname) in enumerate(table):
        lr = seg[pname]["lr_head"] if gname == "f_dc" else seg[pname]["lr"]
        groups.append(dict(params=[torch.nn.Parameter(torch.empty(0))], lr=float(lr), name=gname))
        if optimizer is not None and optimizer.step_count > 0:
            state[k] = {"step": torch.tensor(float(optimizer.step_count)),
                        "exp_avg": clone(group_view(segment(optimizer.exp_avg, model, pname), gname)),
                        "exp_avg_sq": clone(group_view(segment(optimizer.exp_avg_sq, model, pname), gname))}
    # the remaining keys of a group (amsgrad, weight_decay, foreach ...) as THIS torch's Adam fills them in
    opt_dict = {"state": state, "param_groups": torch.optim.Adam(groups, lr=0.0, betas=tuple(betas), eps=eps).state_dict()["param_groups"]}

    max_radii2D = clone(stats.max_radii2D) if stats is not None else zeros(P)
    xyz_acc = clone(stats.xyz_gradient_accum) if stats is not None else zeros(P, 1)
    denom = clone(stats.denom) if stats is not None else zeros(P, 1)
    head = (int(model.active_sh_degree), clone(p["_xyz"]), clone(group_view(p["_features"], "f_dc")), clone(group_view(p["_features"], "f_rest")),
            clone(p["_scaling"]), clone(p["_rotation"]), clone(p["_opacity"]), max_radii2D, xyz_acc)
    if model.gaussian_dim == 3:
        return head + (denom, opt_dict, float(spatial_lr_scale))
    t_acc = clone(stats.t_gradient_accum) if stats is not None else zeros(P, 1)
    env = getattr(model, "env_map", None)
    return head + (t_acc, denom, opt_dict, float(spatial_lr_scale), clone(p["_t"]), clone(p["_scaling_t"]),
                   clone(model._rotation_r) if model.rot_4d else torch.empty(0, device=dev), bool(model.rot_4d),
                   clone(env) if env is not None and env.numel() else torch.empty(0, device=dev), int(model.active_sh_degree_t))


def restore(model_args: tuple, device, *, sh_degree: int, sh_degree_t: int = 0, time_duration, force_sh_3d: bool = False,
            prefilter_var: float = -1.0, with_optimizer: bool = True) -> Tuple[GaussianParams, Optional[FlatAdam], object]:
    """``GaussianModel(sh_degree, gaussian_dim, time_duration, rot_4d, force_sh_3d, sh_degree_t, prefilter_var).restore(model_args,
    training_args)``: (model, optimizer, stats) on ``device`` from a ``capture()`` tuple -- the reference's or ours.  ``gaussian_dim``
    follows from the tuple's length (12 / 19), ``rot_4d`` and the active degrees come from the tuple; ``sh_degree`` / ``sh_degree_t``
    are the MAXIMAL degrees the coefficients were allocated for, ``time_duration`` the reference's [t0, t1] (or the duration from 0).
    The parameters arrive bit for bit; the moments, the groups' learning rates, betas, eps and the step count go into a ``FlatAdam``
    (``with_optimizer=False``: None, like ``training_args`` None); ``stats``: a ``harness.DensificationStats`` with the tuple's
    accumulators.  ValueError: a tuple of another length, a coefficient count that does not belong to the degrees, per-parameter
    ``step`` values that differ (FlatAdam has one step count)."""
    from .harness import DensificationStats
    from .synth import num_sh_coeffs
    if not isinstance(model_args, (tuple, list)) or len(model_args) not in (12, 19):
        raise ValueError("fdgs.checkpoint.restore: a capture() tuple has 12 (3D) or 19 (4D) entries, got %s" % (
            len(model_args) if isinstance(model_args, (tuple, list)) else type(model_args).__name__))
    if len(model_args) == 12:
        (active, xyz, f_dc, f_rest, scaling, rotation, opacity, max_radii2D, xyz_acc, denom, opt_dict, _scale) = model_args
        dim, rot_4d, active_t, t_acc, env_map = 3, False, 0, None, None
        raw = {}
    else:
        (active, xyz, f_dc, f_rest, scaling, rotation, opacity, max_radii2D, xyz_acc, t_acc, denom, opt_dict, _scale, t, scaling_t,
         rotation_r, rot_4d, env_map, active_t) = model_args
        dim, rot_4d = 4, bool(rot_4d)
        raw = dict(_t=t, _scaling_t=scaling_t, _rotation_r=rotation_r if rot_4d else None)
    if (rot_4d or force_sh_3d) and dim != 4:
        raise ValueError("fdgs.checkpoint.restore: rot_4d / force_sh_3d need a 4D model (scene/gaussian_model.py:88-89)")
    M = int(f_dc.shape[1]) + int(f_rest.shape[1])
    allowed = {reference_sh_channels(sh_degree, sh_degree_t, dim, force_sh_3d), num_sh_coeffs(sh_degree, sh_degree_t, force_sh_3d, dim)}
    if int(f_dc.shape[1]) != 1 or M not in allowed:
        raise ValueError("fdgs.checkpoint.restore: the checkpoint holds M = %d SH coefficients per Gaussian (_features_dc %s, _features_rest "
                         "%s); sh_degree = %d, sh_degree_t = %d%s allocate %s" % (M, tuple(f_dc.shape), tuple(f_rest.shape), sh_degree,
                                                                                  sh_degree_t, ", force_sh_3d" if force_sh_3d else "",
                                                                                  " or ".join(str(a) for a in sorted(allowed))))
    if not 0 <= int(active) <= sh_degree or not 0 <= int(active_t) <= sh_degree_t:
        raise ValueError("fdgs.checkpoint.restore: active SH degrees (%d, %d) beyond the maximal ones (%d, %d)" % (active, active_t, sh_degree, sh_degree_t))
    raw.update({"_xyz": xyz, "_features": torch.cat((f_dc.detach(), f_rest.detach()), dim=1), "_opacity": opacity, "_scaling": scaling,
                "_rotation": rotation})
    duration = [0.0, float(time_duration)] if isinstance(time_duration, (int, float)) else list(time_duration)
    model = GaussianParams.from_raw(raw, device, max_sh_degree=sh_degree, max_sh_degree_t=sh_degree_t, active_sh_degree=int(active),
                                    active_sh_degree_t=int(active_t), time_duration=duration, rot_4d=rot_4d, gaussian_dim=dim,
                                    force_sh_3d=force_sh_3d, prefilter_var=prefilter_var)
    if env_map is not None and env_map.numel():
        model.env_map = env_map.detach().to(device=device, dtype=torch.float32).clone().requires_grad_(True)
    P = model.P
    stats = DensificationStats(P, device)
    fill = [("max_radii2D", max_radii2D, (P,)), ("xyz_gradient_accum", xyz_acc, (P, 1)), ("denom", denom, (P, 1))]
    if t_acc is not None:
        fill.append(("t_gradient_accum", t_acc, (P, 1)))
    for name, src, shape in fill:
        if src is not None and src.numel():     # (a model saved before training_setup has empty accumulators)
            getattr(stats, name).copy_(src.detach().to(device=device, dtype=torch.float32).reshape(shape))
    if not with_optimizer:
        return model, None, stats
    return model, _restore_optimizer(model, opt_dict, group_table(dim, rot_4d)), stats


def _restore_optimizer(model, opt_dict, table) -> FlatAdam:
    groups = opt_dict["param_groups"]
    names = [g.get("name") for g in groups]
    if names != [g for g, _ in table]:
        raise ValueError("fdgs.checkpoint.restore: the optimizer's groups are %s, this model's are %s" % (names, [g for g, _ in table]))
    betas, eps = {tuple(g["betas"]) for g in groups}, {float(g["eps"]) for g in groups}
    if len(betas) != 1 or len(eps) != 1:
        raise ValueError("fdgs.checkpoint.restore: FlatAdam has one betas / eps pair, the groups have %s / %s" % (sorted(betas), sorted(eps)))
    opt = FlatAdam(model, betas=betas.pop(), eps=eps.pop())
    lr = {g["name"]: float(g["lr"]) for g in groups}
    for gname, pname in table:
        if gname == "f_dc":
            continue
        if gname == "f_rest":
            opt.set_lr(pname, lr["f_rest"], lr_head=lr["f_dc"])
        else:
            opt.set_lr(pname, lr[gname])
    steps = {}
    for g, (gname, pname) in zip(groups, table):
        st = opt_dict["state"].get(g["params"][0])
        if st is None:
            steps[gname] = 0
            continue
        steps[gname] = int(float(st["step"]))
        for key, flat in (("exp_avg", opt.exp_avg), ("exp_avg_sq", opt.exp_avg_sq)):
            dst = group_view(segment(flat, model, pname), gname)
            if tuple(st[key].shape) != tuple(dst.shape):
                raise ValueError("fdgs.checkpoint.restore: %s of group %s is %s, the parameter is %s" % (key, gname, tuple(st[key].shape), tuple(dst.shape)))
            dst.copy_(st[key].detach().to(device=flat.device, dtype=torch.float32))
    if len(set(steps.values())) > 1:
        raise ValueError("fdgs.checkpoint.restore: FlatAdam has one step count, the groups' steps differ: %s" % (
            ", ".join("%s = %d" % kv for kv in steps.items())))
    opt.step_count = next(iter(steps.values()))
    return opt


def save(path, model: GaussianParams, optimizer: Optional[FlatAdam], iteration: int, stats=None, spatial_lr_scale: float = 1.0) -> None:
    """``torch.save((capture(...), iteration), path)`` -- the reference's checkpoint file (train.py:224-228)."""
    torch.save((capture(model, optimizer, stats, spatial_lr_scale), int(iteration)), path)


def load(path, device, **kw):
    """(model, optimizer, stats, iteration) from a checkpoint file written by ``save`` or by the reference; ``kw``: ``restore``'s
    keyword arguments.  Loaded with ``weights_only=True``: the file holds tensors, dicts, tuples and numbers only."""
    model_args, iteration = torch.load(path, map_location=device, weights_only=True)
    return restore(model_args, device, **kw) + (int(iteration),)
