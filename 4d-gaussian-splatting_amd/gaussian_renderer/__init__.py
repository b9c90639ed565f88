"""Drop-in for the reference's ``gaussian_renderer`` package: ``render()``.

Same signature, branches and result dict as gaussian_renderer/__init__.py:19-194
of the reference; the rasterizer underneath is the MI355X-native one
(``.diff_gaussian_rasterization`` -> csrc/libfdgs.so).  ``pc`` / ``viewpoint_camera`` /
``pipe`` are duck-typed exactly as in the reference (SURVEY.md section 8b lists the
members that are read).  Unlike the reference, the device is taken from the
model (``pc.get_xyz.device``) instead of the literal "cuda".
"""
import torch
from torch.nn import functional as F

from .diff_gaussian_rasterization import GaussianRasterizer, camera_tensors, view_settings
from ..sh_utils import eval_sh, eval_shfs_4d


def _select(mask, *tensors):
    return tuple(None if t is None else t[mask] for t in tensors)


# Options of the fast path below (process-wide).  tile_cull: fdgs_forward_out.tile_cull -- shorter tile lists, same pixels and
# gradients (off: point_list / ranges / n_contrib are the reference's, bit for bit).
# fast_path: False sends every model through the reference's own sequence (getters -> activations in PyTorch -> rasterizer).
render_options = {"tile_cull": False, "fast_path": True}

_RAW_ATTRS = ("_xyz", "_scaling", "_rotation", "_opacity", "_features_dc", "_features_rest")


def _fast_path(pc, pipe, raster_settings, means2D):
    """A reference-style model (raw ``_scaling`` / ``_rotation`` / ``_opacity`` / ``_features_dc`` / ``_features_rest`` ... attributes,
    scene/gaussian_model.py:70-80) on the default pipeline: the kernels take the RAW parameters and apply the activations of
    :179-209 themselves (no exp / sigmoid / normalize kernels forward and backward; ``fdgs.fused._RasterizeRaw``).  With an
    ``fdgs.optim.Adam`` that owns the parameters as ``pc.optimizer`` also no ``torch.cat`` of the SH coefficients and no gradient
    accumulation pass: the backward writes the parameter gradients straight into the optimizer's flat gradient bucket behind ``p.grad``
    and returns nothing for them (see fdgs/optim.py).  None: not applicable."""
    if pipe.compute_cov3D_python or pipe.convert_SHs_python or pipe.debug or not render_options["fast_path"]:
        return None
    if not all(isinstance(getattr(pc, a, None), torch.Tensor) for a in _RAW_ATTRS):
        return None
    xyz = pc._xyz
    if not xyz.is_cuda or xyz.dtype != torch.float32 or pc._features_dc.dim() != 3:
        return None
    is_4d = pc.gaussian_dim == 4
    if is_4d and not (isinstance(getattr(pc, "_t", None), torch.Tensor) and isinstance(getattr(pc, "_scaling_t", None), torch.Tensor)):
        return None
    if is_4d and pc.rot_4d and not isinstance(getattr(pc, "_rotation_r", None), torch.Tensor):
        return None
    from ..fused import _RasterizeRaw, raw_tensors
    from ..optim import Adam as _FdgsAdam
    opt = getattr(pc, "optimizer", None)
    if isinstance(opt, _FdgsAdam) and opt.ensure_homed() and opt._homed["xyz"][0] is xyz:
        tensors, lazy = opt.model_tensors(pc), opt.lazy_forward
    else:
        tensors, opt, lazy = raw_tensors(pc), None, False
    return _RasterizeRaw.apply(tensors[0], means2D, *tensors[1:], raster_settings, opt, bool(render_options["tile_cull"]), lazy)


def render(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, scaling_modifier=1.0, override_color=None, *, flow_to=None):
    """Render the scene seen by ``viewpoint_camera``.  ``bg_color`` must live on the model's device.
    ``flow_to``: a camera of the same image size (``fdgs.playback.with_timestamp(viewpoint_camera, t1)``: the same camera at another
    time).  The rasterizer's ``flow_2d`` is then every Gaussian's screen motion from this view to that one (``fdgs.flow.gaussian_flow``
    of the activated getters) instead of zeros, and ``"flow"`` is the blended image ``sum_i flow_i alpha_i T_i`` in pixels -- NOT
    divided by alpha: divide by ``"alpha"`` for the mean motion of what a pixel shows.  A loss on ``"flow"`` reaches the parameters
    through the rasterizer (alpha, T) and through the flow itself."""
    xyz = pc.get_xyz
    device = xyz.device

    # zero tensor whose .grad receives the screen-space mean gradients (densification statistics)
    screenspace_points = torch.zeros_like(xyz, dtype=xyz.dtype, requires_grad=True, device=device) + 0
    try:
        screenspace_points.retain_grad()
    except Exception:
        pass

    # a camera under optimisation (fdgs.camera.LearnableCamera): its matrices are differentiable torch expressions and its timestamp a
    # 0-d tensor; the rasterizer returns their gradients when they require one
    raster_settings, timestamp_tensor = view_settings(viewpoint_camera, pc, pipe, bg_color, scaling_modifier)
    rasterizer = GaussianRasterizer(raster_settings=raster_settings, timestamp_tensor=timestamp_tensor)
    _, camera_grad = camera_tensors(raster_settings, timestamp_tensor)

    # (the fast path has no flow input and no camera gradients: with flow_to, or a camera tensor that requires a gradient, the model goes
    # through the reference's own sequence below)
    fast = _fast_path(pc, pipe, raster_settings, screenspace_points) if (override_color is None and flow_to is None and not camera_grad) else None
    if fast is not None:
        rendered_image, radii, depth, alpha, flow = fast
        return _finish(viewpoint_camera, pc, pipe, screenspace_points, rendered_image, radii, depth, alpha, flow, None)

    means3D, means2D, opacity = xyz, screenspace_points, pc.get_opacity
    scales = scales_t = rotations = rotations_r = ts = cov3D_precomp = None
    prefilter_var = -1.0
    marginal_t = None
    is_4d = pc.gaussian_dim == 4

    # covariance: Python-side (pipe.compute_cov3D_python) or inside the preprocess kernel
    if pipe.compute_cov3D_python:
        if pc.rot_4d:
            cov3D_precomp, delta_mean = pc.get_current_covariance_and_mean_offset(scaling_modifier, viewpoint_camera.timestamp)
            means3D = means3D + delta_mean
        else:
            cov3D_precomp = pc.get_covariance(scaling_modifier)
        if is_4d:
            marginal_t = pc.get_marginal_t(viewpoint_camera.timestamp)
            opacity = opacity * marginal_t
    else:
        scales, rotations = pc.get_scaling, pc.get_rotation
        if is_4d:
            scales_t, ts = pc.get_scaling_t, pc.get_t
            if pc.rot_4d:
                rotations_r = pc.get_rotation_r
            if pc.prefilter_var > 0.0:
                prefilter_var = pc.prefilter_var

    # colour: override > Python SH (pipe.convert_SHs_python) > SH inside the preprocess kernel
    shs = colors_precomp = None
    if override_color is not None:
        colors_precomp = override_color
    elif pipe.convert_SHs_python:
        feats = pc.get_features
        shs_view = feats.transpose(1, 2).view(-1, 3, pc.get_max_sh_channels)
        cam = viewpoint_camera.camera_center.repeat(feats.shape[0], 1)
        if pipe.compute_cov3D_python:
            dir_pp = (means3D - cam).detach()
        else:
            _, delta_mean = pc.get_current_covariance_and_mean_offset(scaling_modifier, viewpoint_camera.timestamp)
            dir_pp = ((means3D + delta_mean) - cam).detach()
        dir_pp = dir_pp / dir_pp.norm(dim=1, keepdim=True)
        if pc.gaussian_dim == 3 or pc.force_sh_3d:
            sh2rgb = eval_sh(pc.active_sh_degree, shs_view, dir_pp)
        elif is_4d:
            dir_t = (pc.get_t - viewpoint_camera.timestamp).detach()
            sh2rgb = eval_shfs_4d(pc.active_sh_degree, pc.active_sh_degree_t, shs_view, dir_pp, dir_t,
                                  pc.time_duration[1] - pc.time_duration[0])
        colors_precomp = torch.clamp_min(sh2rgb + 0.5, 0.0)
    else:
        shs = pc.get_features
        if is_4d and ts is None:
            ts = pc.get_t

    if flow_to is None:
        flow_2d = torch.zeros_like(xyz[:, :2])
    else:
        from ..flow import model_flow
        flow_2d = model_flow(viewpoint_camera, flow_to, pc, raw=False, scaling_modifier=scaling_modifier)

    # temporal pre-filter when the marginal was folded into opacity in Python
    mask = None
    if pipe.compute_cov3D_python and is_4d:
        mask = marginal_t[:, 0] > 0.05
        (means2D, means3D, ts, shs, colors_precomp, opacity, scales, scales_t, rotations, rotations_r, cov3D_precomp,
         flow_2d) = _select(mask, means2D, means3D, ts, shs, colors_precomp, opacity, scales, scales_t, rotations,
                            rotations_r, cov3D_precomp, flow_2d)

    rendered_image, radii, depth, alpha, flow, covs_com = rasterizer(
        means3D=means3D, means2D=means2D, shs=shs, colors_precomp=colors_precomp, flow_2d=flow_2d,
        opacities=opacity, ts=ts, scales=scales, scales_t=scales_t, rotations=rotations, rotations_r=rotations_r,
        cov3D_precomp=cov3D_precomp, prefilter_var=prefilter_var)

    return _finish(viewpoint_camera, pc, pipe, screenspace_points, rendered_image, radii, depth, alpha, flow, mask)


def _finish(viewpoint_camera, pc, pipe, screenspace_points, rendered_image, radii, depth, alpha, flow, mask):
    """Environment map behind the Gaussians, radii scattered back through the marginal_t mask, the result dict
    (gaussian_renderer/__init__.py:165-194)."""
    if pipe.env_map_res:
        # composite an environment map behind the Gaussians (sphere of radius 60)
        assert pc.env_map is not None
        sphere_r = 60
        rays_o, rays_d = viewpoint_camera.get_rays()
        od = (rays_o * rays_d).sum(-1)
        dd = (rays_d ** 2).sum(-1)
        delta = od ** 2 - dd * ((rays_o ** 2).sum(-1) - sphere_r ** 2)
        assert (delta > 0).all()
        t_inter = -od + torch.sqrt(delta) / dd
        xyz_inter = rays_o + rays_d * t_inter.unsqueeze(-1)
        tu = torch.atan2(xyz_inter[..., 1:2], xyz_inter[..., 0:1]) / (2 * torch.pi) + 0.5
        tv = torch.acos(xyz_inter[..., 2:3] / sphere_r) / torch.pi
        texcoord = torch.cat([tu, tv], dim=-1) * 2 - 1
        bg_from_envmap = F.grid_sample(pc.env_map[None], texcoord[None])[0]
        rendered_image = rendered_image + (1 - alpha) * bg_from_envmap

    if mask is not None:
        radii_all = radii.new_zeros(mask.shape)
        radii_all[mask] = radii
    else:
        radii_all = radii

    # Gaussians that were culled or had radius 0 were not visible (excluded from densification statistics)
    return {"render": rendered_image,
            "viewspace_points": screenspace_points,
            "visibility_filter": radii_all > 0,
            "radii": radii_all,
            "depth": depth,
            "alpha": alpha,
            "flow": flow}
