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
import torch

from .gaussian_renderer.diff_gaussian_rasterization import (_C, backward_args, camera_gradients, camera_inputs, camera_tensors, forward_args,
                                                             image_gradients, shaped, time_inputs, view_settings)


def raw_forward(rs, means3D, sh, opacity_raw, ts, scaling_raw, scaling_t_raw, rotation_raw, rotation_r_raw, prefilter_var,
                split_colour=False, preprocessed=None, tile_cull=False, lazy=False, sparse_lists=False, colour_stream=None, flows=None):
    """Native forward on RAW parameters (fdgs_scene.raw_params = 1); the reference binding's 11-tuple.  ``flows``: the rasterizer's
    per-Gaussian ``flow_2d`` input [P, 2] (default: none, the flow image is zero).
    ``preprocessed``: the view's handle from ``raw_preprocess_batch``; ``tile_cull``: fdgs_forward_out.tile_cull; ``lazy``:
    fdgs_forward_out.lazy (num_rendered comes back as -1, the host does not wait); ``sparse_lists``: fdgs_forward_out.sparse_lists; ``colour_stream``: fdgs_forward_out.colour_stream (a torch.cuda.Stream)."""
    args = forward_args(rs, means3D, sh, opacity_raw, ts, scaling_raw, scaling_t_raw, rotation_raw, rotation_r_raw, prefilter_var,
                        **({} if flows is None else {"flow_2d": flows}))
    return _C.rasterize_gaussians(*args, raw_params=True, split_colour=split_colour, preprocessed=preprocessed, tile_cull=tile_cull, lazy=lazy,
                                  sparse_lists=sparse_lists, colour_stream=colour_stream)


def raw_preprocess_batch(settings, means3D, sh, opacity_raw, ts, scaling_raw, scaling_t_raw, rotation_raw, rotation_r_raw, prefilter_var,
                         tile_cull=False):
    """View-batched preprocess on RAW parameters (fdgs_preprocess_batch): ``settings`` = the views' raster settings (the views of
    one optimizer step share every parameter tensor).  One handle per view for ``raw_forward(..., preprocessed=handle)``."""
    views = [forward_args(rs, means3D, sh, opacity_raw, ts, scaling_raw, scaling_t_raw, rotation_raw, rotation_r_raw, prefilter_var)
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
    args = backward_args(rs, means3D, out_means3D, radii, sh, opacity_raw, ts, scaling_raw, scaling_t_raw, rotation_raw, rotation_r_raw,
                         prefilter_var, geom, R, binb, img, g_color, g_depth, g_alpha, g_flow, **({} if flows is None else {"flow_2d": flows}))
    if begin_only:
        return _C.backward_begin(*args, raw_params=True, grad_out=sink, accumulate=accumulate, grad_accum=grad_accum, sh_stage=sh_stage,
                                 per_view_outputs=per_view_outputs)
    return _C.rasterize_gaussians_backward(*args, raw_params=True, grad_out=sink, accumulate=accumulate, grad_accum=grad_accum,
                                           after_sh=after_sh, sh_stage=sh_stage, per_view_outputs=per_view_outputs, geometry_adam=geometry_adam,
                                           camera=camera)


def raw_tensors(pc):
    """(xyz, features, opacity, t, scaling, scaling_t, rotation, rotation_r, prefilter_var): the raw parameters of ``pc`` (the reference's
    attribute names) as the kernels take them."""
    ts, scaling_t, rotation_r, prefilter_var = time_inputs(pc, lambda name: getattr(pc, "_" + name))
    return (pc._xyz, pc.get_features, pc._opacity, ts, pc._scaling, scaling_t, pc._rotation, rotation_r, prefilter_var)


def _raw_view(viewpoint_camera, pc, pipe, bg_color, scaling_modifier):
    if pipe.compute_cov3D_python or pipe.convert_SHs_python:
        raise ValueError("render_raw covers the default pipeline only; use render() for the Python covariance / SH branches")
    return view_settings(viewpoint_camera, pc, pipe, bg_color, scaling_modifier) + (raw_tensors(pc),)


def raw_settings(viewpoint_camera, pc, pipe, bg_color, scaling_modifier=1.0):
    """GaussianRasterizationSettings + the raw parameter tensors of ``pc`` for the default pipeline (``view_settings`` and
    ``raw_tensors``)."""
    rs, _timestamp_tensor, tensors = _raw_view(viewpoint_camera, pc, pipe, bg_color, scaling_modifier)
    return rs, tensors


class _RasterizeRaw(torch.autograd.Function):
    """The rasterizer on a model's RAW parameters (fdgs_scene.raw_params: activations inside the kernels).  ``grad_to`` says where the
    parameter gradients go: None -- back to autograd; ``(sink, accumulate)`` -- into the caller's buffers (see the module docstring);
    an ``fdgs.optim.Adam`` that owns the parameters -- into the flat gradient bucket behind ``p.grad`` and its SH stage, asked for at
    backward time (``backward_begin(rs)``).  An input whose gradient went there gets None from autograd.  ``lazy``: the forward does
    not wait for num_rendered (such a forward never hands its lists out: they may as well sit at fixed offsets -- no count / scan
    launch).  ``cam``: () or (viewmatrix, projmatrix, campos, timestamp tensor or None) as explicit inputs: a camera under optimisation."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, opacity_raw, ts, scaling_raw, scaling_t_raw, rotation_raw, rotation_r_raw,
                prefilter_var, rs, grad_to, tile_cull, lazy=False, flows=None, *cam):
        ctx.cam_meta = None
        if cam:
            rs = camera_inputs(ctx, rs, *cam)
        (R, color, flow, depth, T, radii, geom, binb, img, covs_com, out_means3D) = raw_forward(
            rs, means3D, sh, opacity_raw, ts, scaling_raw, scaling_t_raw, rotation_raw, rotation_r_raw, prefilter_var, tile_cull=tile_cull,
            lazy=lazy, sparse_lists=lazy, flows=flows)
        ctx.rs, ctx.R, ctx.prefilter_var, ctx.grad_to = rs, R, prefilter_var, grad_to
        ctx.has_flows = flows is not None
        ctx.save_for_backward(means3D, out_means3D, scaling_raw, rotation_raw, radii, sh, opacity_raw, ts, scaling_t_raw,
                              rotation_r_raw, geom, binb, img, *((flows,) if flows is not None else ()))
        ctx.mark_non_differentiable(radii)
        ctx.set_materialize_grads(False)  # unused outputs -> None gradients -> colour-only backward
        if not (grad_to is None or isinstance(grad_to, tuple)):
            grad_to.note_forward(R < 0)
        return color, radii, depth, 1 - T, flow

    @staticmethod
    def backward(ctx, g_color, g_radii, g_depth, g_alpha, g_flow):
        rs, grad_to = ctx.rs, ctx.grad_to
        (means3D, out_means3D, scaling_raw, rotation_raw, radii, sh, opacity_raw, ts, scaling_t_raw, rotation_r_raw,
         geom, binb, img) = ctx.saved_tensors[:13]
        flows = ctx.saved_tensors[13] if ctx.has_flows else None
        grads = image_gradients(rs, means3D.device, g_color, g_depth, g_alpha, g_flow)
        sink, accumulate, gacc, stage = None, False, None, None
        if isinstance(grad_to, tuple):
            sink, accumulate = grad_to
        elif grad_to is not None:
            if not (grad_to.is_homed() and grad_to.features().data_ptr() == sh.data_ptr()):
                # the forward was handed the optimizer's bucket views (plain tensors, no requires_grad): returning gradients for them
                # would be dropped by autograd without a word and no parameter would receive anything
                raise RuntimeError("fdgs render(): the optimizer's parameters or Adam state were replaced between this view's forward and its "
                                   "backward (densification / prune / load_state_dict); the gradients of this view have nowhere to go -- "
                                   "run backward() before editing the optimizer, as the reference's loop does (train.py:160-249)")
            sink, accumulate, gacc, stage = grad_to.backward_begin(rs)
        camera = {"want": tuple(bool(n) for n in ctx.needs_input_grad[15:19])} if ctx.cam_meta is not None else None
        (d_means2D, _d_colors, d_opacity, d_means3D, _d_cov3D, d_sh, d_flows, d_ts, d_scales, d_scales_t, d_rot,
         d_rot_r) = raw_backward(rs, means3D, out_means3D, radii, sh, opacity_raw, ts, scaling_raw, scaling_t_raw, rotation_raw,
                                 rotation_r_raw, ctx.prefilter_var, geom, ctx.R, binb, img, *grads, sink, bool(accumulate),
                                 grad_accum=gacc, sh_stage=stage, flows=flows, camera=camera)

        def ret(name, given, g):
            if (sink and sink.get(name) is not None) or (stage is not None and name == "dL_dsh"):
                return None  # already written into the caller's buffer / staged
            return shaped(given, g)

        tail = ()
        if ctx.has_flows or camera:
            tail = (d_flows.reshape(flows.shape) if ctx.has_flows else None,)
        if camera:
            tail += camera_gradients(ctx, camera["want"], camera)
        return (ret("dL_dmeans3D", means3D, d_means3D), d_means2D, ret("dL_dsh", sh, d_sh),
                ret("dL_dopacity", opacity_raw, d_opacity), ret("dL_dts", ts, d_ts),
                ret("dL_dscales", scaling_raw, d_scales), ret("dL_dscales_t", scaling_t_raw, d_scales_t),
                ret("dL_drotations", rotation_raw, d_rot), ret("dL_drotations_r", rotation_r_raw, d_rot_r),
                None, None, None, None, None) + tail


def render_raw(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, scaling_modifier=1.0, grad_sink=None, accumulate=False, tile_cull=False,
               *, flow_to=None):
    """``render()`` with the activations fused into the kernels; see the module docstring.  ``tile_cull``:
    fdgs_forward_out.tile_cull (shorter tile lists, same pixels and gradients).  ``flow_to``: a camera of the same image size
    (``fdgs.playback.with_timestamp(viewpoint_camera, t1)``: the same camera at another time); the rasterizer's per-Gaussian flow input
    is then every Gaussian's screen motion from this view to that one (``fdgs.flow.gaussian_flow`` of the raw parameters) instead of
    zeros and ``"flow"`` is the blended image ``sum_i flow_i alpha_i T_i`` in pixels, NOT divided by alpha (divide by ``"alpha"`` for
    the mean motion of what a pixel shows).  A loss on ``"flow"`` reaches the parameters through the rasterizer and through the flow
    itself, both by autograd: not together with ``grad_sink``."""
    rs, timestamp_tensor, (xyz, *tensors) = _raw_view(viewpoint_camera, pc, pipe, bg_color, scaling_modifier)
    screenspace_points = torch.zeros_like(xyz, requires_grad=True)
    # a camera under optimisation (fdgs.camera.LearnableCamera): its tensors become inputs of the autograd function
    cam, camera_grad = camera_tensors(rs, timestamp_tensor)
    flows = None
    if flow_to is not None:
        if grad_sink:
            raise ValueError("render_raw: flow_to with grad_sink is not supported: the gradients of the flow arrive through autograd")
        from .flow import model_flow
        flows = model_flow(viewpoint_camera, flow_to, pc, raw=True, scaling_modifier=scaling_modifier)
    extra = (flows,) + (cam if camera_grad else ()) if (camera_grad or flows is not None) else ()
    color, radii, depth, alpha, flow = _RasterizeRaw.apply(
        xyz, screenspace_points, *tensors, rs, (grad_sink, accumulate) if (grad_sink is not None or accumulate) else None, tile_cull, False,
        *extra)
    if getattr(pipe, "env_map_res", 0):
        from .envmap import env_composite
        if getattr(pc, "env_map", None) is None:
            raise ValueError("render_raw: pipe.env_map_res > 0 needs the model's env_map [3, R, R]")
        color = env_composite(color, alpha, pc.env_map, viewpoint_camera)
    return {"render": color, "viewspace_points": screenspace_points, "visibility_filter": radii > 0, "radii": radii,
            "depth": depth, "alpha": alpha, "flow": flow}
