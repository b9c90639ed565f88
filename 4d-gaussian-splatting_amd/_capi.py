"""ctypes binding of libfdgs.so (C ABI: include/fdgs.h).

This is the thin host glue the north star asks for: PyTorch owns every tensor
and the current HIP stream; the library only borrows raw device pointers.  It
plays the role of the reference's pybind module ``_C``
(diff-gaussian-rasterization/ext.cpp:15-19) and of the tensor allocation code in
rasterize_points.cu:36-149, 151-270.

There is NO fallback: if the shared library has not been built
(``4d-gaussian-splatting_amd/csrc/build.sh`` or ``__graft_entry__.build()``) the
import of this module raises, and every entry point raises if handed CPU tensors.
"""
import ctypes as C
import os

import torch  # must be imported before libfdgs.so so both share one HIP runtime (same SONAME)

_HERE = os.path.dirname(os.path.abspath(__file__))
# FDGS_LIB: another build of the same library (A/B timing of kernel variants, tools/ab_build.sh); default: the in-tree build
LIB_PATH = os.environ.get("FDGS_LIB") or os.path.join(_HERE, "csrc", "libfdgs.so")

FDGS_BUF_GEOMETRY, FDGS_BUF_BINNING, FDGS_BUF_IMAGE = 0, 1, 2

_fp = C.c_void_p  # all device pointers travel as void*


FDGS_VERSION = 502  # include/fdgs.h; checked against fdgs_version() at import


class _Sized(C.Structure):
    """Every struct of the ABI starts with ``struct_size`` = sizeof(struct) (include/fdgs.h: the library rejects any other value);
    filled in here so that the call sites keep passing the remaining fields positionally."""

    def __init__(self, *args, **kw):
        super().__init__(C.sizeof(type(self)), *args, **kw)


class FdgsScene(_Sized):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("P", C.c_int32), ("D", C.c_int32), ("D_t", C.c_int32), ("M", C.c_int32), ("W", C.c_int32), ("H", C.c_int32),
        ("bg", _fp), ("means3D", _fp), ("shs", _fp), ("colors_precomp", _fp), ("flows", _fp), ("opacities", _fp),
        ("ts", _fp), ("scales", _fp), ("scales_t", _fp), ("rotations", _fp), ("rotations_r", _fp),
        ("cov3D_precomp", _fp), ("viewmatrix", _fp), ("projmatrix", _fp), ("campos", _fp),
        ("scale_modifier", C.c_float), ("prefilter_var", C.c_float),
        ("tan_fovx", C.c_float), ("tan_fovy", C.c_float),
        ("timestamp", C.c_float), ("time_duration", C.c_float),
        ("rot_4d", C.c_int32), ("gaussian_dim", C.c_int32), ("force_sh_3d", C.c_int32),
        ("prefiltered", C.c_int32), ("debug", C.c_int32), ("raw_params", C.c_int32), ("analytic_sh_grad", C.c_int32),
    ]


class FdgsForwardOut(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("out_color", _fp), ("out_flow", _fp), ("out_depth", _fp), ("out_T", _fp), ("radii", _fp),
                ("out_means3D", _fp), ("covs_com", _fp), ("preprocessed", C.c_int32), ("split_colour", C.c_int32), ("tile_cull", C.c_int32),
                ("lazy", C.c_int32), ("sparse_lists", C.c_int32), ("colour_stream", C.c_void_p)]


class FdgsBackwardIn(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("dL_dout_color", _fp), ("dL_dout_depth", _fp), ("dL_dout_alpha", _fp), ("dL_dout_flow", _fp),
                ("radii", _fp), ("out_means3D", _fp), ("geom_buffer", _fp), ("binning_buffer", _fp),
                ("image_buffer", _fp), ("num_rendered", C.c_int32)]


class FdgsGeometryAdam(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("flat", _fp), ("exp_avg", _fp), ("exp_avg_sq", _fp),
                ("lr_means3D", C.c_float), ("lr_opacities", C.c_float), ("lr_ts", C.c_float), ("lr_scales", C.c_float), ("lr_scales_t", C.c_float),
                ("lr_rotations", C.c_float), ("lr_rotations_r", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("step", C.c_int32)]


class FdgsBackwardOut(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("dL_dmeans2D", _fp), ("dL_dcolors", _fp), ("dL_dopacity", _fp), ("dL_dmeans3D", _fp),
                ("dL_dcov3D", _fp), ("dL_dsh", _fp), ("dL_dflows", _fp), ("dL_dts", _fp), ("dL_dscales", _fp),
                ("dL_dscales_t", _fp), ("dL_drotations", _fp), ("dL_drotations_r", _fp), ("accumulate", C.c_int32),
                ("grad_accum", _fp), ("grad_accum_clean", C.c_int32), ("sh_stage", _fp), ("stage_mask", C.c_int32), ("adam", C.POINTER(FdgsGeometryAdam))]


class FdgsDebugView(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("depths", _fp), ("records", _fp), ("cov3D", _fp), ("tiles_touched", _fp), ("clamped", _fp),
                ("point_list", _fp), ("ranges", _fp), ("n_contrib", _fp),
                ("final_T", _fp), ("tile_order", _fp)]


class FdgsSliceIn(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("P", C.c_int32), ("D", C.c_int32), ("D_t", C.c_int32), ("M", C.c_int32),
                ("means3D", _fp), ("shs", _fp), ("opacities", _fp), ("ts", _fp), ("scales", _fp), ("scales_t", _fp), ("rotations", _fp),
                ("rotations_r", _fp), ("scale_modifier", C.c_float), ("prefilter_var", C.c_float), ("timestamp", C.c_float),
                ("time_duration", C.c_float), ("rot_4d", C.c_int32), ("force_sh_3d", C.c_int32)]


class FdgsSliceOut(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("capacity", C.c_int32), ("index", _fp), ("xyz", _fp), ("cov3D", _fp), ("opacity", _fp),
                ("shs", _fp), ("scales", _fp), ("rotations", _fp), ("n_live", _fp)]


class FdgsTransformIn(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("P", C.c_int32), ("M", C.c_int32), ("gaussian_dim", C.c_int32), ("rot_4d", C.c_int32),
                ("means3D", _fp), ("ts", _fp), ("scales", _fp), ("scales_t", _fp), ("rotations", _fp), ("rotations_r", _fp), ("shs", _fp),
                ("rotation", C.c_double * 9), ("translation", C.c_double * 3), ("scale", C.c_double), ("time_scale", C.c_double),
                ("time_shift", C.c_double), ("quat", C.c_double * 4), ("iso_u", C.c_double * 4), ("iso_v", C.c_double * 4),
                ("log_scale", C.c_double), ("log_time_scale", C.c_double), ("sh_rot", C.c_float * 83)]


class FdgsTransformOut(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("means3D", _fp), ("ts", _fp), ("scales", _fp), ("scales_t", _fp), ("rotations", _fp),
                ("rotations_r", _fp), ("shs", _fp)]


class FdgsFlowIn(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("P", C.c_int32), ("W", C.c_int32), ("H", C.c_int32), ("means3D", _fp), ("ts", _fp),
                ("scales", _fp), ("scales_t", _fp), ("rotations", _fp), ("rotations_r", _fp), ("viewmatrix", _fp), ("projmatrix", _fp),
                ("viewmatrix_to", _fp), ("projmatrix_to", _fp), ("timestamp", C.c_float), ("timestamp_to", C.c_float),
                ("scale_modifier", C.c_float), ("rot_4d", C.c_int32), ("gaussian_dim", C.c_int32), ("raw_params", C.c_int32)]


class FdgsFlowGrads(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("d_means3D", _fp), ("d_ts", _fp), ("d_scales", _fp), ("d_scales_t", _fp),
                ("d_rotations", _fp), ("d_rotations_r", _fp)]


class FdgsContributionIn(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("P", C.c_int32), ("W", C.c_int32), ("H", C.c_int32), ("geom_buffer", _fp),
                ("binning_buffer", _fp), ("image_buffer", _fp), ("num_rendered", C.c_int32), ("pix_weight", _fp)]


class FdgsContributionOut(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("weight_sum", _fp), ("weight_max", _fp), ("hits", _fp), ("dominant", _fp),
                ("dominant_id", _fp)]


class FdgsFeatureIn(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("P", C.c_int32), ("W", C.c_int32), ("H", C.c_int32), ("C", C.c_int32), ("geom_buffer", _fp),
                ("binning_buffer", _fp), ("image_buffer", _fp), ("num_rendered", C.c_int32), ("features", _fp)]


FDGS_FEATURE_MAX_CHANNELS = 256  # include/fdgs.h


class FdgsCameraGrads(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("dL_dviewmatrix", _fp), ("dL_dprojmatrix", _fp), ("dL_dcampos", _fp),
                ("dL_dtimestamp", _fp), ("scale", C.c_float), ("accumulate", C.c_int32)]


class FdgsDepthIn(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("H", C.c_int32), ("W", C.c_int32), ("depth", _fp), ("alpha", _fp), ("mask", _fp),
                ("alpha_min", C.c_float)]


class FdgsDepthGrads(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("d_depth", _fp), ("d_alpha", _fp), ("g_upstream", _fp), ("scale", C.c_float),
                ("accumulate", C.c_int32)]


FDGS_DEPTH_PEARSON, FDGS_DEPTH_SSI = 0, 1  # include/fdgs.h


class FdgsTsdfVolume(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("ox", C.c_float), ("oy", C.c_float),
                ("oz", C.c_float), ("voxel_size", C.c_float), ("trunc", C.c_float), ("tsdf", _fp), ("weight", _fp), ("color", _fp),
                ("cweight", _fp)]   # (ox, oy, oz): float origin[3]


class FdgsTsdfView(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("H", C.c_int32), ("W", C.c_int32), ("depth", _fp), ("alpha", _fp), ("mask", _fp),
                ("image", _fp), ("viewmatrix", _fp), ("alpha_min", C.c_float), ("fl_x", C.c_float), ("fl_y", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("view_weight", C.c_float)]


class FdgsSurfaceOut(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("vertex_capacity", C.c_int32), ("face_capacity", C.c_int32), ("vertices", _fp),
                ("normals", _fp), ("colors", _fp), ("faces", _fp), ("n_vertices", _fp), ("n_faces", _fp)]


class FdgsMeshIn(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("V", C.c_int32), ("F", C.c_int32), ("vertices", _fp), ("normals", _fp), ("colors", _fp),
                ("faces", _fp)]


class FdgsMeshComponentsOut(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("capacity", C.c_int32), ("labelled", C.c_int32), ("vertex_component", _fp), ("n_components", _fp),
                ("component_vertices", _fp), ("component_faces", _fp), ("rounds", C.POINTER(C.c_int32))]   # rounds: host memory


class FdgsMeshSmoothOut(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("iterations", C.c_int32), ("lam", C.c_float), ("mu", C.c_float), ("pin_boundary", C.c_int32),
                ("vertices", _fp), ("normals", _fp), ("boundary", _fp)]   # lam: float lambda


class FdgsMeshSimplifyParams(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("ox", C.c_float), ("oy", C.c_float),
                ("oz", C.c_float), ("cell", C.c_float), ("placement", C.c_int32), ("stabilise", C.c_float), ("vertex_map", _fp)]   # (ox, oy, oz): float origin[3]


FDGS_SIMPLIFY_MEAN, FDGS_SIMPLIFY_QUADRIC = 0, 1  # include/fdgs.h


class FdgsAdamSegment(C.Structure):
    _fields_ = [("begin", C.c_int64), ("end", C.c_int64), ("lr", C.c_float), ("lr_head", C.c_float),
                ("period", C.c_int32), ("head", C.c_int32)]


ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_int, C.c_size_t)

_i, _i64, _f, _p, _sz = C.c_int32, C.c_int64, C.c_float, C.c_void_p, C.c_size_t
_P = C.POINTER
_mesh_scratch = (_sz, [_i, _i])
# every symbol include/fdgs.h declares: name -> (restype, argtypes).  The one place a new entry point is bound (EXPORTED and _load follow it)
SIGNATURES = {
    "fdgs_rasterize_forward": (C.c_int, [_P(FdgsScene), _P(FdgsForwardOut), ALLOC_FN, _p, _p, _P(_i)]),
    "fdgs_forward_lazy_status": (C.c_int, [_i, _p, _P(_i), _P(_i), _P(_i), _i, _P(_i)]),
    "fdgs_rasterize_backward": (C.c_int, [_P(FdgsScene), _P(FdgsBackwardIn), _P(FdgsBackwardOut), _p]),
    "fdgs_preprocess_batch": (C.c_int, [_i, _P(_P(FdgsScene)), _P(_P(FdgsForwardOut)), ALLOC_FN, _P(_p), _p]),
    "fdgs_sh_backward_batch": (C.c_int, [_i, _P(_P(FdgsScene)), _P(_P(FdgsBackwardIn)), _P(_P(FdgsBackwardOut)), _p]),
    "fdgs_mark_visible": (C.c_int, [_i] + [_p] * 5),
    "fdgs_geometry_bytes": (_sz, [_i]),
    "fdgs_image_bytes": (_sz, [_i, _i]),
    "fdgs_binning_bytes": (_sz, [_i] * 3),
    "fdgs_debug_views": (C.c_int, [_i] * 4 + [_p] * 3 + [_P(FdgsDebugView)]),
    "fdgs_debug_activations": (C.c_int, [_i] + [_p] * 11),
    "fdgs_debug_radix_sort_scratch_bytes": (_sz, [_i]),
    "fdgs_debug_radix_sort_pairs": (C.c_int, [_i] * 3 + [_p] * 4),
    "fdgs_debug_knn_stage_offsets": (C.c_int, [_i] * 3 + [_P(_i64)]),
    "fdgs_debug_tile_sort_limits": (None, [_i, _i]),
    "fdgs_debug_tile_bin_scratch_bytes": (_sz, [_i, _i]),
    "fdgs_debug_tile_bin": (C.c_int, [_i, _p, _p] + [_i] * 5 + [_p] * 9),
    "fdgs_debug_block_reaches": (C.c_int, [_i, _p, _p, _p]),
    "fdgs_debug_run_ahead_stats": (None, [_P(_i64)]),
    "fdgs_set_run_ahead": (None, [_i]),
    "fdgs_set_sparse_lists_budget": (C.c_int, [_i64, _i]),
    "fdgs_debug_sparse_lists_stats": (None, [_P(_i64)]),
    "fdgs_debug_clock_sample": (C.c_int, [_p, C.c_double, _p]),
    "fdgs_sh_flush": (C.c_int, [_i] * 8 + [_p, _p, _i, _p]),
    "fdgs_profile_enable": (C.c_int, [C.c_int]),
    "fdgs_profile_sample_every": (C.c_int, [_i]),
    "fdgs_profile_read": (C.c_int, [C.c_int, _P(C.c_double), _P(_i64)]),
    "fdgs_profile_reset": (C.c_int, []),
    "fdgs_stage_name": (C.c_char_p, [C.c_int]),
    "fdgs_l1_ssim_forward": (C.c_int, [_p, _p, _i, _i, _i] + [_p] * 6),
    "fdgs_l1_ssim_backward": (C.c_int, [_p, _p, _i, _i, _i] + [_p] * 4 + [_f, _p, _p]),
    "fdgs_l1_ssim_loss": (C.c_int, [_p, _p] + [_i] * 4 + [_f, _p, _p]),
    "fdgs_l1_ssim_loss_batch": (C.c_int, [_p] + [_i] * 5 + [_f, _p, _p]),
    "fdgs_l1_ssim_num_partials": (C.c_int, [_i] * 3),
    "fdgs_l1_ssim_value_and_grad": (C.c_int, [_p, _p, _i, _i, _i, _p, _f] + [_p] * 4),
    "fdgs_adam_step": (C.c_int, [_p] * 4 + [_i64, _P(FdgsAdamSegment), _i, _f, _f, _f, _i, _p]),
    "fdgs_adam_step_sh": (C.c_int, [_p] * 4 + [_i] * 8 + [_p] + [_f] * 5 + [_i, _p]),
    "fdgs_densify_classify": (C.c_int, [_i] + [_p] * 5 + [_f] * 5 + [_i, _i, _p, _p]),
    "fdgs_densify_gather": (C.c_int, [_i, _P(_i), _i64, _i64] + [_p] * 9),
    "fdgs_densify_split": (C.c_int, [_i] * 4 + [_p] * 14),
    "fdgs_densify_stats_local": (C.c_int, [_i, _i, _P(_p), _P(_p)] + [_p] * 4),
    "fdgs_densify_stats_apply": (C.c_int, [_i] + [_p] * 4 + [_f] + [_p] * 5),
    "fdgs_knn_scratch_bytes": (_sz, [_i]),
    "fdgs_dist2_knn3": (C.c_int, [_i] + [_p] * 4),
    "fdgs_knn_query_scratch_bytes": (_sz, [_i, _i]),
    "fdgs_knn_query": (C.c_int, [_i] * 4 + [_p] * 6),
    "fdgs_rigid_motion_scratch_bytes": (_sz, [_i, _i]),
    "fdgs_rigid_motion_forward": (C.c_int, [_i, _i] + [_p] * 11),
    "fdgs_rigid_motion_backward": (C.c_int, [_i, _i] + [_p] * 9 + [_f] + [_p] * 6),
    "fdgs_opa_mask_num_partials": (C.c_int, [_i, _i]),
    "fdgs_opa_mask_loss": (C.c_int, [_i, _i, _p, _i, _p, _p, _f, _p, _i, _p, _p, _p]),
    "fdgs_env_composite": (C.c_int, [_i, _i, _p, _p] + [_f] * 4 + [_p, _i, _i, _f] + [_p] * 4),
    "fdgs_env_composite_backward": (C.c_int, [_i, _i, _p, _p] + [_f] * 4 + [_p, _i, _i, _f, _p, _p, _p, _i, _p, _i, _p]),
    "fdgs_eval_metrics_scratch_bytes": (C.c_int, [_i] * 3),
    "fdgs_eval_metrics": (C.c_int, [_p, _p] + [_i] * 4 + [_p] * 3),
    "fdgs_frames_decode": (C.c_int, [_p] + [_i] * 4 + [_p, _i, _p, _i64, _p, _i64, _p]),
    "fdgs_frames_encode": (C.c_int, [_p, _i64, _p, _i64] + [_i] * 4 + [_p, _i, _p, _p]),
    "fdgs_frames_encode_gray_scratch_bytes": (_i64, [_i] * 3),
    "fdgs_frames_encode_gray": (C.c_int, [_p, _i64] + [_i] * 3 + [_p, _i, _p, _p, _p]),
    "fdgs_frames_resize": (C.c_int, [_p] + [_i] * 4 + [_p, _i, _p] + [_i] * 3 + [_p, _p, _i, _p, _p, _i, _p, _p]),
    "fdgs_frames_resize_scratch_bytes": (_i64, [_i] * 6),
    "fdgs_debug_frames_resize_path": (None, [_i]),
    "fdgs_frames_composite": (C.c_int, [_p] + [_i] * 5 + [_p, _p]),
    "fdgs_time_slice_scratch_bytes": (_sz, [_i]),
    "fdgs_time_slice": (C.c_int, [_P(FdgsSliceIn), _P(FdgsSliceOut), _p, _p]),
    "fdgs_gaussian_flow_forward": (C.c_int, [_P(FdgsFlowIn), _p, _p]),
    "fdgs_gaussian_flow_backward": (C.c_int, [_P(FdgsFlowIn), _p, _f, _P(FdgsFlowGrads), _p]),
    "fdgs_contribution": (C.c_int, [_P(FdgsContributionIn), _P(FdgsContributionOut), _p]),
    "fdgs_feature_blend": (C.c_int, [_P(FdgsFeatureIn), _p, _p]),
    "fdgs_feature_blend_backward": (C.c_int, [_P(FdgsFeatureIn), _p, _p, _p]),
    "fdgs_camera_backward_scratch": (_sz, [_i]),
    "fdgs_camera_backward": (C.c_int, [_P(FdgsScene), _P(FdgsBackwardIn), _p, _P(FdgsCameraGrads), _p, _sz, _p]),
    "fdgs_kmeans_scratch_bytes": (_sz, [_i, _i]),
    "fdgs_kmeans_assign": (C.c_int, [_i] * 3 + [_p] * 6),
    "fdgs_kmeans_update": (C.c_int, [_i] * 3 + [_p] * 7),
    "fdgs_quantize_columns": (C.c_int, [_i, _i, _p, _p, _p, _i, _p, _p]),
    "fdgs_compact_decode": (C.c_int, [_i] * 3 + [_p] * 3 + [_i, _p, _p, _i, _p, _p]),
    "fdgs_model_transform": (C.c_int, [_P(FdgsTransformIn), _P(FdgsTransformOut), _p]),
    "fdgs_depth_loss_num_partials": (C.c_int, [_i, _i]),
    "fdgs_depth_loss": (C.c_int, [_P(FdgsDepthIn), _p, _i, _P(FdgsDepthGrads), _p, _p, _p]),
    "fdgs_depth_normals": (C.c_int, [_P(FdgsDepthIn)] + [_f] * 4 + [_p] * 4),
    "fdgs_depth_normals_backward": (C.c_int, [_P(FdgsDepthIn)] + [_f] * 4 + [_p, _p, _P(FdgsDepthGrads), _p]),
    "fdgs_tsdf_integrate": (C.c_int, [_P(FdgsTsdfVolume), _i, _P(FdgsTsdfView), _p]),
    "fdgs_surface_extract_scratch_bytes": (_sz, [_i] * 3),
    "fdgs_surface_extract": (C.c_int, [_P(FdgsTsdfVolume), _f, _P(FdgsSurfaceOut), _p, _p]),
    "fdgs_mesh_components_scratch_bytes": _mesh_scratch,
    "fdgs_mesh_components": (C.c_int, [_P(FdgsMeshIn), _P(FdgsMeshComponentsOut), _p, _p]),
    "fdgs_mesh_compact_scratch_bytes": _mesh_scratch,
    "fdgs_mesh_compact": (C.c_int, [_P(FdgsMeshIn), _p, _p, _i, _P(FdgsSurfaceOut), _p, _p]),
    "fdgs_mesh_smooth_scratch_bytes": _mesh_scratch,
    "fdgs_mesh_smooth": (C.c_int, [_P(FdgsMeshIn), _P(FdgsMeshSmoothOut), _p, _p]),
    "fdgs_mesh_simplify_scratch_bytes": _mesh_scratch,
    "fdgs_mesh_simplify": (C.c_int, [_P(FdgsMeshIn), _P(FdgsMeshSimplifyParams), _P(FdgsSurfaceOut), _p, _p]),
    "fdgs_last_error": (C.c_char_p, []),
    "fdgs_version": (C.c_int, []),
}
EXPORTED = tuple(SIGNATURES)
NUM_STAGES = 12
# offsets[] of fdgs_debug_knn_stage_offsets (include/fdgs.h FDGS_KNN_STAGE_*)
KNN_STAGE_BOUNDS, KNN_STAGE_BOXES, KNN_STAGE_SRC_CODES, KNN_STAGE_SRC_ORDER, KNN_STAGE_QUERY_CODES, KNN_STAGE_QUERY_ORDER, \
    KNN_STAGE_NBOXES, KNN_STAGE_BOX, KNN_NUM_STAGES = range(9)


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libfdgs.so not found at %s -- build it with 4d-gaussian-splatting_amd/csrc/build.sh "
            "(or __graft_entry__.build()); there is no CPU / PyTorch fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if lib.fdgs_version() != FDGS_VERSION:
        raise ImportError("%s is version %d, this binding was written for FDGS_VERSION %d (include/fdgs.h): rebuild the library "
                          "(4d-gaussian-splatting_amd/csrc/build.sh)" % (LIB_PATH, lib.fdgs_version(), FDGS_VERSION))
    return lib


lib = _load()


def last_error() -> str:
    return lib.fdgs_last_error().decode()


def _check(rc: int, what: str, arg_error=Exception):
    """``arg_error``: what an argument error (code 1) raises; modules whose own checks raise ValueError pass that."""
    if rc != 0:
        msg = last_error()
        if rc == 1:
            # argument errors keep the reference's Python-level wording / type
            # (gaussian_renderer/diff_gaussian_rasterization.py:271-280 raise plain Exception)
            raise arg_error(msg)
        raise RuntimeError("%s failed (code %d): %s" % (what, rc, msg))


def current_stream_handle(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def call(name, dev, *args, guard=True, stream=None, arg_error=Exception):
    """The one way a launching entry point is called: ``lib.<name>(*args, stream)`` with ``dev`` current and ``stream`` the current
    stream of ``dev`` (the last argument of every such entry point), then ``_check``.  ``guard=False``: the caller is inside
    ``torch.cuda.device(dev)`` already (several calls under one guard, a ``torch.cuda.stream`` block) and it is not entered again.
    ``stream``: a handle of the caller's instead (``ClockSample``'s own stream; one look-up for back-to-back calls).  The two entry
    points that take their stream in the middle are written out below: ``rasterize_forward``, ``forward_lazy_status``."""
    fn = getattr(lib, name)
    if stream is None:
        stream = current_stream_handle(dev)
    if guard:
        with torch.cuda.device(dev):
            rc = fn(*args, stream)
    else:
        rc = fn(*args, stream)
    if rc != 0:
        _check(rc, name, arg_error)


def need_gpu(t, name, what=None, got=True):
    """The one refusal of a CPU tensor; ``what``: what the message calls it where that is not "tensor '<name>'"; ``got=False``: the
    rasterizer's older wording, which does not say where the tensor is."""
    if not t.is_cuda:
        raise RuntimeError("fdgs: %s must live on the GPU%s; there is no CPU path" % (what or "tensor '%s'" % name, " (got %s)" % t.device if got else ""))


def scratch(nbytes, dev, floor=0):
    """``nbytes`` of device scratch as a uint8 tensor; ``floor``: the least it allocates (an entry point that wants a pointer even
    where it needs no bytes)."""
    return torch.empty(max(int(nbytes), floor), dtype=torch.uint8, device=dev)


def _ptr(t):
    """Device pointer of a tensor; None / empty tensor -> NULL (the reference's absent-tensor convention)."""
    if t is None or t.numel() == 0:
        return None
    return t.data_ptr()


def _dev_f32(t, name):
    if t is None or t.numel() == 0:
        return None
    need_gpu(t, name)
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _common_device(named):
    """The common device of the tensors ``named`` ((name, tensor) pairs; None and empty tensors are skipped: an empty model leaves
    buffers out), or None; a CPU tensor raises."""
    dev = None
    for name, t in named:
        if t is None or t.numel() == 0:
            continue
        need_gpu(t, name)
        if dev is not None and t.device != dev:
            raise RuntimeError("fdgs: '%s' lives on %s, the forward's buffers on %s" % (name, t.device, dev))
        dev = t.device
    return dev


def debug_activations(opacity_raw=None, scales_raw=None, scales_t_raw=None, rotations_raw=None, rotations_r_raw=None):
    """The activated tensors the kernels derive from raw parameters (fdgs_debug_activations): bit-identical to what
    preprocess computes in flight with fdgs_scene.raw_params = 1.  Returns a 5-tuple (None where the input was None)."""
    ins = [opacity_raw, scales_raw, scales_t_raw, rotations_raw, rotations_r_raw]
    ref = next(t for t in ins if t is not None)
    ins = [_dev_f32(t, "raw parameter") for t in ins]
    outs = [None if t is None else torch.empty_like(t) for t in ins]
    P = int(ref.shape[0])
    call("fdgs_debug_activations", ref.device, P, *[_ptr(t) for t in ins], *[_ptr(t) for t in outs])
    return tuple(outs)


def sh_flush(stages, dL_dsh, sh_degree, sh_degree_t, gaussian_dim, force_sh_3d, analytic_sh_grad=False, accumulate=False):
    """dL_dsh from the staged views of the deferred SH backward (fdgs_sh_flush); ``stages``: [num_views, P, 8] float32
    tensor whose slices stages[v] were the ``sh_stage`` of the views' backward calls; ``analytic_sh_grad``: the mode those
    calls ran in (set_analytic_sh_gradients)."""
    P, M = int(dL_dsh.shape[0]), int(dL_dsh.shape[1])
    if stages.dim() != 3 or stages.shape[1] != P or stages.shape[2] != 8 or not stages.is_contiguous() or stages.dtype != torch.float32:
        raise RuntimeError("fdgs: stages must be a contiguous float32 tensor [num_views, %d, 8]" % P)
    call("fdgs_sh_flush", dL_dsh.device, P, int(sh_degree), int(sh_degree_t), M, int(gaussian_dim), int(bool(force_sh_3d)),
         int(bool(analytic_sh_grad)), int(stages.shape[0]), stages.data_ptr(), dL_dsh.data_ptr(), int(bool(accumulate)))


def adam_step_sh(params, exp_avg, exp_avg_sq, stages, sh_degree, sh_degree_t, gaussian_dim, force_sh_3d, analytic_sh_grad,
                 lr, lr_dc, beta1, beta2, eps, step, dL_dsh=None) -> bool:
    """Adam over the SH coefficients ``params`` [P, M, 3] with the gradient built from the staged views (fdgs_adam_step_sh).
    Returns False -- nothing done -- if the shape / alignment is not supported (the caller then uses sh_flush + the plain step)."""
    P, M = int(params.shape[0]), int(params.shape[1])
    if stages.dim() != 3 or stages.shape[1] != P or stages.shape[2] != 8 or not stages.is_contiguous() or stages.dtype != torch.float32:
        raise RuntimeError("fdgs: stages must be a contiguous float32 tensor [num_views, %d, 8]" % P)
    ptrs = [params.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr()] + ([dL_dsh.data_ptr()] if dL_dsh is not None else [])
    if (3 * M) % 4 != 0 or any(q % 16 for q in ptrs):
        return False
    call("fdgs_adam_step_sh", params.device, params.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
         dL_dsh.data_ptr() if dL_dsh is not None else None, P, int(sh_degree), int(sh_degree_t), M, int(gaussian_dim),
         int(bool(force_sh_3d)), int(bool(analytic_sh_grad)), int(stages.shape[0]), stages.data_ptr(), float(lr), float(lr_dc),
         float(beta1), float(beta2), float(eps), int(step))
    return True


def rasterize_forward(dev, scene, out, alloc, num_rendered):
    """fdgs_rasterize_forward on the current stream of ``dev`` (its stream argument is not the last one); ``num_rendered``: a c_int32."""
    with torch.cuda.device(dev):
        rc = lib.fdgs_rasterize_forward(C.byref(scene), C.byref(out), alloc, None, current_stream_handle(dev), C.byref(num_rendered))
    _check(rc, "fdgs_rasterize_forward")


def forward_lazy_status(device, wait=True):
    """fdgs_forward_lazy_status for the calling thread on ``device``: (pending, failed, [num_rendered of the reported forwards])."""
    pend, failed, n = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    rs = (C.c_int32 * 64)()
    with torch.cuda.device(device):
        rc = lib.fdgs_forward_lazy_status(int(bool(wait)), current_stream_handle(device), C.byref(pend), C.byref(failed), rs, 64, C.byref(n))
    _check(rc, "fdgs_forward_lazy_status")
    return int(pend.value), int(failed.value), [int(rs[i]) for i in range(n.value)]


def run_ahead_stats():
    """(kept, sorted again, exact) counts of this process's forward calls (fdgs_debug_run_ahead_stats)."""
    a = (C.c_int64 * 3)()
    lib.fdgs_debug_run_ahead_stats(a)
    return tuple(int(x) for x in a)


def sparse_lists_stats():
    """(forwards with sparse lists, forwards that asked for them and kept compact lists because of the byte budget, bytes of the last
    run-ahead binning buffer) -- fdgs_debug_sparse_lists_stats."""
    a = (C.c_int64 * 3)()
    lib.fdgs_debug_sparse_lists_stats(a)
    return tuple(int(x) for x in a)


class ClockSample:
    """Shader clock sustained over an interval (fdgs_debug_clock_sample): start() enqueues the one-wave sampler on its own stream,
    ghz() waits for it and returns the measured clock in GHz."""

    def __init__(self, device):
        self.dev = device
        self.stream = torch.cuda.Stream(device)
        self.out = torch.zeros(5, dtype=torch.int64, device=device)

    def start(self, span_ms: float):
        call("fdgs_debug_clock_sample", self.dev, self.out.data_ptr(), float(span_ms), stream=C.c_void_p(self.stream.cuda_stream))

    def ghz(self):
        self.stream.synchronize()
        w0, s0, w1, s1, khz = [int(x) for x in self.out.cpu().tolist()]
        if w1 <= w0 or khz <= 0:
            return None
        return (s1 - s0) / (w1 - w0) * khz * 1e-6


class ClockPair:
    """The same measurement without a stream of its own (a step that uses four streams leaves no hardware queue for a sampler that
    sits in one for the whole interval): two short samples on the CALLER's stream, mark() where the interval starts and mark() where it
    ends; s_memtime is one chip-wide counter, so the shader cycles between the first sample's start and the second one's end over the
    constant-rate ticks between them is the clock sustained in between (bench.py checks it against ClockSample: FDGS_BENCH_CLOCK=both)."""

    def __init__(self, device):
        self.dev = device
        self.out = torch.zeros((2, 5), dtype=torch.int64, device=device)
        self.n = 0

    def mark(self):
        call("fdgs_debug_clock_sample", self.dev, self.out[self.n].data_ptr(), 0.002)
        self.n += 1

    def ghz(self):
        if self.n != 2:
            return None
        torch.cuda.synchronize(self.dev)
        (w0, s0, _w, _s, khz), (_w2, _s2, w1, s1, _k) = [[int(x) for x in row] for row in self.out.cpu().tolist()]
        if w1 <= w0 or khz <= 0:
            return None
        return (s1 - s0) / (w1 - w0) * khz * 1e-6


def profile_enable(on: bool = True, stages=None, every: int = 1):
    """Bracket stages with HIP events on the caller's stream (fdgs_profile_enable).  ``stages``: iterable of stage
    names to restrict the events to; ``every``: only every n-th launch of a stage gets its event pair (fdgs_profile_sample_every: a
    pair costs the stream ~13 us of idle time around the launch)."""
    lib.fdgs_profile_sample_every(max(1, int(every)))
    if not on:
        mask = 0
    elif stages is None:
        mask = -1
    else:
        names = [lib.fdgs_stage_name(i).decode() for i in range(NUM_STAGES)]
        mask = 0
        for s in stages:
            mask |= 1 << names.index(s)
    lib.fdgs_profile_enable(mask)


def profile_reset():
    lib.fdgs_profile_reset()


def profile_read():
    """{stage name: (total_ms, samples)} accumulated since the last reset; synchronises pending events."""
    out = {}
    for st in range(NUM_STAGES):
        ms, n = C.c_double(0.0), C.c_int64(0)
        lib.fdgs_profile_read(st, C.byref(ms), C.byref(n))
        out[lib.fdgs_stage_name(st).decode()] = (ms.value, int(n.value))
    return out
