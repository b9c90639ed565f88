"""Fused-activation rendering: ``render_raw``.

``render()`` (gaussian_renderer/__init__.py, the drop-in) receives post-activation tensors from the model's
getters, exactly like the reference: exp / sigmoid / normalize run as separate PyTorch kernels forward and
backward, and autograd then accumulates every parameter gradient with one more pass.  ``render_raw`` feeds the
model's RAW parameters (the reference's attribute names ``_xyz, _opacity, _scaling, _rotation, _t, _scaling_t,
_rotation_r`` and ``get_features``) to the same kernels with ``fdgs_scene.raw_params = 1``: the activations of
scene/gaussian_model.py:179-219 are applied inside preprocess and their derivatives inside preprocess-backward.
With ``grad_sink`` (e.g. ``GaussianParams.grad_sink()``) the backward writes each gradient straight into the
caller's buffers -- the slices of the flat data-parallel bucket -- and returns no gradient to autograd for those
inputs, so there is no accumulation pass and no zero_grad.  A sink is OVERWRITTEN by a backward with
``accumulate=False`` (the first view of an optimizer step) and ADDED to with ``accumulate=True`` (the following
views of the same step: the reference sums ``loss / batch_size`` over ``batch_size`` views, train.py:104-166).

Covers the default pipeline (in-kernel covariance and SH, rot_4d or not) and the environment map (``pipe.env_map_res``:
rasterized over black, then ``fdgs.envmap.env_composite``); the Python covariance / SH branches go through ``render()``.  Same
result dict as ``render()``.
"""
import math

import torch

from .gaussian_renderer.diff_gaussian_rasterization import GaussianRasterizationSettings, _C, _is_given, camera_tensors, detached_settings


def _raw_forward_args(rs, means3D, sh, opacity_raw, ts, scaling_raw, scaling_t_raw, rotation_raw, rotation_r_raw, prefilter_var, flows=None):
    e = torch.Tensor([])
    return (rs.bg, means3D, e, e if flows is None else flows, opacity_raw, ts, scaling_raw, scaling_t_raw, rotation_raw, rotation_r_raw,
            rs.scale_modifier, e, prefilter_var, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy,
            rs.image_height, rs.image_width, sh, rs.sh_degree, rs.sh_degree_t, rs.campos, rs.timestamp,
            rs.time_duration, rs.rot_4d, rs.gaussian_dim, rs.force_sh_3d, rs.prefiltered, rs.debug)


def raw_forward(rs, means3D, sh, opacity_raw, ts, scaling_raw, scaling_t_raw, rotation_raw, rotation_r_raw, prefilter_var,
                split_colour=False, preprocessed=None, tile_cull=False, lazy=False, sparse_lists=False, colour_stream=None, flows=None):
    """Native forward on RAW parameters (fdgs_scene.raw_params = 1); the reference binding's 11-tuple.  ``flows``: the rasterizer's
    per-Gaussian ``flow_2d`` input [P, 2] (default: none, the flow image is zero).
    ``preprocessed``: the view's handle from ``raw_preprocess_batch``; ``tile_cull``: fdgs_forward_out.tile_cull; ``lazy``:
    fdgs_forward_out.lazy (num_rendered comes back as -1, the host does not wait); ``sparse_lists``: fdgs_forward_out.sparse_lists; ``colour_stream``: fdgs_forward_out.colour_stream (a torch.cuda.Stream)."""
    args = _raw_forward_args(rs, means3D, sh, opacity_raw, ts, scaling_raw, scaling_t_raw, rotation_raw, rotation_r_raw, prefilter_var, flows)
    return _C.rasterize_gaussians(*args, raw_params=True, split_colour=split_colour, preprocessed=preprocessed, tile_cull=tile_cull, lazy=lazy,
                                  sparse_lists=sparse_lists, colour_stream=colour_stream)


def raw_preprocess_batch(settings, means3D, sh, opacity_raw, ts, scaling_raw, scaling_t_raw, rotation_raw, rotation_r_raw, prefilter_var,
                         tile_cull=False):
    """View-batched preprocess on RAW parameters (fdgs_preprocess_batch): ``settings`` = the views' raster settings (the views of
    one optimizer step share every parameter tensor).  One handle per view for ``raw_forward(..., preprocessed=handle)``."""
    views = [_raw_forward_args(rs, means3D, sh, opacity_raw, ts, scaling_raw, scaling_t_raw, rotation_raw, rotation_r_raw, prefilter_var)
             for rs in settings]
    return _C.preprocess_batch(views, raw_params=True, tile_cull=tile_cull)


def raw_backward(rs, means3D, out_means3D, radii, sh, opacity_raw, ts, scaling_raw, scaling_t_raw, rotation_raw, rotation_r_raw,
                 prefilter_var, geom, R, binb, img, g_color, g_depth, g_alpha, g_flow, sink, accumulate, grad_accum=None, after_sh=None,
                 sh_stage=None, begin_only=False, per_view_outputs=True, geometry_adam=None, flows=None, camera=None):
    """Native backward on RAW parameters; gradients go into ``sink`` where given; the binding's 12-tuple.  ``flows``: the forward's.
    ``begin_only``: only the blend backward (``_C.backward_begin``): returns the pending call for ``_C.sh_backward_batch`` /
    ``_C.backward_finish``.  ``per_view_outputs=False``: dL_dcolors / dL_dcov3D / dL_dflows are not written (None in the tuple).
    ``geometry_adam``: see ``_C.rasterize_gaussians_backward`` (the geometry parameters' Adam step inside the geometry backward);
    ``camera``: as there (the camera gradients, computed between the two halves of the backward)."""
    e = torch.Tensor([])
    args = (rs.bg, means3D, out_means3D, radii, e, e if flows is None else flows, opacity_raw, ts, scaling_raw, scaling_t_raw, rotation_raw,
            rotation_r_raw, rs.scale_modifier, e, prefilter_var, rs.viewmatrix, rs.projmatrix, rs.tanfovx,
            rs.tanfovy, g_color, g_depth, g_alpha, g_flow, sh, rs.sh_degree, rs.sh_degree_t, rs.campos,
            rs.timestamp, rs.time_duration, rs.rot_4d, rs.gaussian_dim, rs.force_sh_3d, geom, R, binb, img, rs.debug)
    if begin_only:
        return _C.backward_begin(*args, raw_params=True, grad_out=sink, accumulate=accumulate, grad_accum=grad_accum, sh_stage=sh_stage,
                                 per_view_outputs=per_view_outputs)
    return _C.rasterize_gaussians_backward(*args, raw_params=True, grad_out=sink, accumulate=accumulate, grad_accum=grad_accum,
                                           after_sh=after_sh, sh_stage=sh_stage, per_view_outputs=per_view_outputs, geometry_adam=geometry_adam,
                                           camera=camera)


_BLACK = {}


def _black(device):
    """A zero background per device, made once (and waited for once: it is read on whichever stream renders)."""
    z = _BLACK.get(device)
    if z is None:
        z = _BLACK[device] = torch.zeros(3, dtype=torch.float32, device=device)
        torch.cuda.current_stream(device).synchronize()
    return z


def raw_settings(viewpoint_camera, pc, pipe, bg_color, scaling_modifier=1.0):
    """GaussianRasterizationSettings + the raw parameter tensors of ``pc`` for the default pipeline (with ``pipe.env_map_res`` the
    background is black whatever ``bg_color`` says: the environment map is composited behind the Gaussians afterwards)."""
    if pipe.compute_cov3D_python or pipe.convert_SHs_python:
        raise ValueError("render_raw covers the default pipeline only; use render() for the Python covariance / SH branches")
    if getattr(pipe, "env_map_res", 0):
        bg_color = _black(pc._xyz.device)   # the environment is composited behind a black background (gaussian_renderer/__init__.py:41)
    rs = GaussianRasterizationSettings(
        image_height=int(viewpoint_camera.image_height), image_width=int(viewpoint_camera.image_width),
        tanfovx=math.tan(viewpoint_camera.FoVx * 0.5), tanfovy=math.tan(viewpoint_camera.FoVy * 0.5),
        bg=bg_color, scale_modifier=scaling_modifier, viewmatrix=viewpoint_camera.world_view_transform,
        projmatrix=viewpoint_camera.full_proj_transform, sh_degree=pc.active_sh_degree,
        sh_degree_t=pc.active_sh_degree_t, campos=viewpoint_camera.camera_center, timestamp=viewpoint_camera.timestamp,
        time_duration=pc.time_duration[1] - pc.time_duration[0], rot_4d=pc.rot_4d, gaussian_dim=pc.gaussian_dim,
        force_sh_3d=pc.force_sh_3d, prefiltered=False, debug=pipe.debug)
    e = torch.Tensor([])
    is_4d = pc.gaussian_dim == 4
    ts = pc._t if is_4d else e
    scaling_t = pc._scaling_t if is_4d else e
    rotation_r = pc._rotation_r if (is_4d and pc.rot_4d) else e
    prefilter_var = pc.prefilter_var if (is_4d and pc.prefilter_var > 0.0) else -1.0
    return rs, (pc._xyz, pc.get_features, pc._opacity, ts, pc._scaling, scaling_t, pc._rotation, rotation_r, prefilter_var)


class _RasterizeRaw(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, opacity_raw, ts, scaling_raw, scaling_t_raw, rotation_raw, rotation_r_raw,
                prefilter_var, raster_settings, grad_sink, accumulate, tile_cull=False, flows=None, *cam):
        # cam: () or (viewmatrix, projmatrix, campos, timestamp tensor or None) as explicit inputs: a camera under optimisation
        rs = raster_settings
        ctx.cam_meta = None
        if cam:
            rs = detached_settings(rs._replace(viewmatrix=cam[0], projmatrix=cam[1], campos=cam[2]), cam[3])
            ctx.cam_meta = [None if t is None else (t.shape, t.dtype) for t in cam]
        (R, color, flow, depth, T, radii, geom, binb, img, covs_com, out_means3D) = raw_forward(
            rs, means3D, sh, opacity_raw, ts, scaling_raw, scaling_t_raw, rotation_raw, rotation_r_raw, prefilter_var, tile_cull=tile_cull,
            flows=flows)
        ctx.rs, ctx.R, ctx.prefilter_var, ctx.sink, ctx.accumulate = rs, R, prefilter_var, grad_sink, bool(accumulate)
        ctx.has_flows = flows is not None
        ctx.save_for_backward(means3D, out_means3D, scaling_raw, rotation_raw, radii, sh, opacity_raw, ts, scaling_t_raw,
                              rotation_r_raw, geom, binb, img, *((flows,) if flows is not None else ()))
        ctx.mark_non_differentiable(radii)
        ctx.set_materialize_grads(False)  # unused outputs -> None gradients -> colour-only backward
        return color, radii, depth, 1 - T, flow

    @staticmethod
    def backward(ctx, g_color, g_radii, g_depth, g_alpha, g_flow):
        rs = ctx.rs
        (means3D, out_means3D, scaling_raw, rotation_raw, radii, sh, opacity_raw, ts, scaling_t_raw, rotation_r_raw,
         geom, binb, img) = ctx.saved_tensors[:13]
        flows = ctx.saved_tensors[13] if ctx.has_flows else None
        sink = ctx.sink
        camera = {"want": tuple(bool(n) for n in ctx.needs_input_grad[15:19])} if ctx.cam_meta is not None else None
        (d_means2D, _d_colors, d_opacity, d_means3D, _d_cov3D, d_sh, d_flows, d_ts, d_scales, d_scales_t, d_rot,
         d_rot_r) = raw_backward(rs, means3D, out_means3D, radii, sh, opacity_raw, ts, scaling_raw, scaling_t_raw, rotation_raw,
                                 rotation_r_raw, ctx.prefilter_var, geom, ctx.R, binb, img, g_color, g_depth, g_alpha, g_flow,
                                 sink, ctx.accumulate, flows=flows, camera=camera)

        cam_grads = ()
        if camera is not None:
            for need, name, meta in zip(camera["want"], ("viewmatrix", "projmatrix", "campos", "timestamp"), ctx.cam_meta):
                g = camera["grads"].get(name) if (need and meta is not None) else None
                cam_grads += (None if g is None else g.reshape(meta[0]).to(meta[1]),)

        def ret(name, given, g):
            if not _is_given(given):
                return None
            if sink and sink.get(name) is not None:
                return None  # already written into the caller's buffer
            return g.reshape(given.shape)

        return (ret("dL_dmeans3D", means3D, d_means3D), d_means2D, ret("dL_dsh", sh, d_sh),
                ret("dL_dopacity", opacity_raw, d_opacity), ret("dL_dts", ts, d_ts),
                ret("dL_dscales", scaling_raw, d_scales), ret("dL_dscales_t", scaling_t_raw, d_scales_t),
                ret("dL_drotations", rotation_raw, d_rot), ret("dL_drotations_r", rotation_r_raw, d_rot_r),
                None, None, None, None, None) + ((d_flows.reshape(flows.shape),) if ctx.has_flows else ((None,) if camera else ())) + cam_grads


def render_raw(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, scaling_modifier=1.0, grad_sink=None, accumulate=False, tile_cull=False,
               *, flow_to=None):
    """``render()`` with the activations fused into the kernels; see the module docstring.  ``tile_cull``:
    fdgs_forward_out.tile_cull (shorter tile lists, same pixels and gradients).  ``flow_to``: a camera of the same image size
    (``fdgs.playback.with_timestamp(viewpoint_camera, t1)``: the same camera at another time); the rasterizer's per-Gaussian flow input
    is then every Gaussian's screen motion from this view to that one (``fdgs.flow.gaussian_flow`` of the raw parameters) instead of
    zeros and ``"flow"`` is the blended image ``sum_i flow_i alpha_i T_i`` in pixels, NOT divided by alpha (divide by ``"alpha"`` for
    the mean motion of what a pixel shows).  A loss on ``"flow"`` reaches the parameters through the rasterizer and through the flow
    itself, both by autograd: not together with ``grad_sink``."""
    rs, (xyz, feats, opacity, ts, scaling, scaling_t, rotation, rotation_r, prefilter_var) = raw_settings(
        viewpoint_camera, pc, pipe, bg_color, scaling_modifier)
    screenspace_points = torch.zeros_like(xyz, requires_grad=True)
    # a camera under optimisation (fdgs.camera.LearnableCamera): its tensors become inputs of the autograd function
    cam_time = viewpoint_camera.timestamp
    cam, camera_grad = camera_tensors(rs, cam_time if isinstance(cam_time, torch.Tensor) else None)
    cam = cam if camera_grad else ()
    if isinstance(cam_time, torch.Tensor) and not camera_grad:
        rs = rs._replace(timestamp=float(cam_time.detach()))
    if flow_to is None:
        color, radii, depth, alpha, flow = _RasterizeRaw.apply(
            xyz, screenspace_points, feats, opacity, ts, scaling, scaling_t, rotation, rotation_r,
            prefilter_var, rs, grad_sink, accumulate, tile_cull, *((None,) + cam if cam else ()))
    else:
        if grad_sink:
            raise ValueError("render_raw: flow_to with grad_sink is not supported: the gradients of the flow arrive through autograd")
        from .flow import model_flow
        flows = model_flow(viewpoint_camera, flow_to, pc, raw=True, scaling_modifier=scaling_modifier)
        color, radii, depth, alpha, flow = _RasterizeRaw.apply(
            xyz, screenspace_points, feats, opacity, ts, scaling, scaling_t, rotation, rotation_r,
            prefilter_var, rs, grad_sink, accumulate, tile_cull, flows, *cam)
    if getattr(pipe, "env_map_res", 0):
        from .envmap import env_composite
        if getattr(pc, "env_map", None) is None:
            raise ValueError("render_raw: pipe.env_map_res > 0 needs the model's env_map [3, R, R]")
        color = env_composite(color, alpha, pc.env_map, viewpoint_camera)
    return {"render": color, "viewspace_points": screenspace_points, "visibility_filter": radii > 0, "radii": radii,
            "depth": depth, "alpha": alpha, "flow": flow}
