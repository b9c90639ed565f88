"""Every public function that turns CPU tensors away before it allocates or launches anything on the GPU, with the call that makes it
do so.  tests/golden/make_golden_cpu_rejections.py records the exception type and text of every row from the commit BEFORE a change
to the binding's glue; tests/test_capi_host.py::test_cpu_rejections_did_not_move holds the code to them.  No row needs a GPU."""
from types import SimpleNamespace as NS

import torch


def cases():
    """[(id "module.function[-variant]", callable without arguments that must raise)]"""
    from fdgs import _capi, compress, densify, depth, edit, envmap, features, flow, frames, importance, knn, loss, metrics, resize, surface
    from fdgs import slice as time_slicing
    from fdgs.gaussian_renderer.diff_gaussian_rasterization import _C

    f = torch.zeros
    img, plane = f(3, 16, 16), f(1, 16, 16)
    pts, u8 = f(4, 3), f(8, dtype=torch.uint8)
    mesh = surface.Mesh(f(3, 3), f(3, 3), f(3, 3), f(1, 3, dtype=torch.int32))
    rgb, rgba = f((1, 2, 2, 3), dtype=torch.uint8), f((1, 2, 2, 4), dtype=torch.uint8)
    idx = f(1, dtype=torch.int32)
    flat_model = NS(flat=f(8), P=4)
    model4d = NS(gaussian_dim=4, rot_4d=True, _xyz=pts, _features=f(4, 1, 3), get_xyz=pts, env_map=None)
    cam = NS(camera_center=f(3))
    e = torch.Tensor([])
    raster = (f(3), pts, f(4, 3), e, f(4, 1), e, f(4, 3), e, f(4, 4), e, 1.0, e, -1.0, torch.eye(4), torch.eye(4), 0.5, 0.5, 16, 16, e, 0, 0,
              f(3), 0.0, 1.0, False, 3, False, False, False)
    return [
        ("_capi._dev_f32", lambda: _capi._dev_f32(pts, "means3D")),
        ("_capi._common_device", lambda: _capi._common_device((("geom", None), ("binb", u8)))),
        ("_capi.debug_activations", lambda: _capi.debug_activations(opacity_raw=f(4, 1))),
        ("rasterizer.rasterize_gaussians", lambda: _C.rasterize_gaussians(*raster)),
        ("rasterizer.preprocess_batch", lambda: _C.preprocess_batch([raster])),
        ("rasterizer.mark_visible", lambda: _C.mark_visible(pts, torch.eye(4), torch.eye(4))),
        ("depth.depth_loss", lambda: depth.depth_loss(plane, None, plane)),
        ("depth.depth_normals", lambda: depth.depth_normals(plane, None, (1.0, 1.0, 8.0, 8.0))),
        ("features.blend_pass-geom", lambda: features.blend_pass(4, 16, 16, u8, u8, u8, 0, f(4, 2))),
        ("features.blend_pass-features", lambda: features.blend_pass(4, 16, 16, None, None, None, 0, f(4, 2))),
        ("features.blend_backward_pass", lambda: features.blend_backward_pass(4, 16, 16, None, None, None, 0, f(2, 16, 16), f(4, 2))),
        ("features.render_features", lambda: features.render_features(None, model4d, None, f(4, 2))),
        ("flow.gaussian_flow", lambda: flow.gaussian_flow(None, None, pts, None, None, None, None, None, rot_4d=False, gaussian_dim=3, raw=True)),
        ("surface.TSDFVolume", lambda: surface.TSDFVolume((0, 0, 0), 0.1, (2, 2, 2), device="cpu")),
        ("surface.prepare_views", lambda: surface.prepare_views([{"depth": plane}], "cuda:0")),
        ("surface.components", lambda: surface.components(mesh)),
        ("surface.clean", lambda: surface.clean(mesh)),
        ("surface.smooth", lambda: surface.smooth(mesh)),
        ("surface.simplify", lambda: surface.simplify(mesh, 0.5)),
        ("surface.cell_for_target", lambda: surface.cell_for_target(mesh, 1)),
        ("compress.assign", lambda: compress.assign(f(4, 3), f(2, 3))),
        ("compress.update", lambda: compress.update(f(4, 3), f(4, dtype=torch.int32), f(2, 3))),
        ("compress.kmeans", lambda: compress.kmeans(f(4, 3), 2)),
        ("compress.quantize_columns", lambda: compress.quantize_columns(f(4, 3), [0, 0, 0], [1, 1, 1], 8)),
        ("compress.decode_into", lambda: compress.decode_into(f(12), 4, 3, 32, f(4, 3))),
        ("compress.compress", lambda: compress.compress(flat_model)),
        ("compress.decompress", lambda: compress.decompress(compress.CompressedModel(), "cpu")),
        ("knn.distCUDA2", lambda: knn.distCUDA2(pts)),
        ("knn.knn", lambda: knn.knn(pts[None], pts[None], 3)),
        ("loss.fused_l1_ssim", lambda: loss.fused_l1_ssim(img, img)),
        ("loss.l1_ssim_grad", lambda: loss.l1_ssim_grad(img, img, 0.2, f(1))),
        ("loss.rigid_motion_loss", lambda: loss.rigid_motion_loss(model4d)),
        ("loss.opa_mask_loss", lambda: loss.opa_mask_loss(plane, plane)),
        ("metrics.image_metrics", lambda: metrics.image_metrics(img, img, msssim=False)),
        ("metrics.psnr", lambda: metrics.psnr(img, img)),
        ("envmap.env_composite", lambda: envmap.env_composite(img, plane, f(3, 8, 8), cam)),
        ("envmap.composite_", lambda: envmap.composite_(img, plane, f(3, 8, 8), cam)),
        ("envmap.EnvMapAdam", lambda: envmap.EnvMapAdam(f(3, 8, 8))),
        ("slice.time_slice", lambda: time_slicing.time_slice(model4d, 0.5)),
        ("edit.transform", lambda: edit.transform(model4d, None)),
        ("importance.contribution_pass-geom", lambda: importance.contribution_pass(4, 16, 16, u8, u8, u8, 0, weight_sum=f(4))),
        ("importance.contribution_pass-out", lambda: importance.contribution_pass(4, 16, 16, None, None, None, 0, weight_sum=f(4))),
        ("importance.prune_by_contribution", lambda: importance.prune_by_contribution(flat_model, None, None)),
        ("frames.decode_frames", lambda: frames.decode_frames(rgb, idx, f(1, 3, 2, 2))),
        ("frames.encode_frames", lambda: frames.encode_frames(f(1, 3, 2, 2), idx, rgb)),
        ("frames.encode_gray", lambda: frames.encode_gray(f(1, 1, 2, 2), idx, f((1, 2, 2, 1), dtype=torch.uint8))),
        ("resize.resize_frames", lambda: resize.resize_frames(rgb, (2, 2))),
        ("resize.composite", lambda: resize.composite(rgba, True)),
        ("densify.densify_and_prune", lambda: densify.densify_and_prune(flat_model, None, None, 0.1, 0.1, 1.0, None)),
    ]
