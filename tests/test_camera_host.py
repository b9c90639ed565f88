"""CPU: the camera-gradient entry point's host side (fdgs_camera_backward: export, struct sizes, argument errors -- nothing is
launched), fdgs.camera.LearnableCamera (bit-equal to its base at zero delta, Jacobians against float64 central differences, the
closed-form centre) and the identity the reference for dL/dtimestamp rests on (tests/camera_oracle.py)."""
import ctypes as C
import os
import re
import types

import numpy as np
import torch

import camera_oracle as co
from util import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_exported_and_struct_sizes_agree_with_the_header():
    from fdgs import _capi
    for sym in ("fdgs_camera_backward", "fdgs_camera_backward_scratch"):
        assert sym in _capi.EXPORTED and hasattr(_capi.lib, sym)
    with open(os.path.join(ROOT, "include", "fdgs.h")) as f:
        text = f.read()
    body = re.search(r"typedef struct fdgs_camera_grads\s*\{(.*?)\}\s*fdgs_camera_grads;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.sub(r"\s+", " ", x).strip() for x in body.split(";") if x.strip()]
    assert fields == ["uint32_t struct_size", "float* dL_dviewmatrix", "float* dL_dprojmatrix", "float* dL_dcampos", "float* dL_dtimestamp",
                      "float scale", "int32_t accumulate"]
    assert [n for n, _ in _capi.FdgsCameraGrads._fields_] == [x.split()[-1].lstrip("*") for x in fields]
    # uint32 + pad, four pointers, float, int32: the C layout of those fields on an LP64 target
    assert C.sizeof(_capi.FdgsCameraGrads) == 8 + 4 * 8 + 8 and _capi.FdgsCameraGrads().struct_size == 48
    assert _capi.lib.fdgs_camera_backward_scratch(0) >= 36 * 4
    assert _capi.lib.fdgs_camera_backward_scratch(257) >= 2 * 36 * 4
    assert _capi.lib.fdgs_camera_backward_scratch(1 << 20) >= 4096 * 36 * 4
    assert "camera_bwd" in [_capi.lib.fdgs_stage_name(i).decode() for i in range(_capi.NUM_STAGES)]


def test_argument_errors_are_reported_without_touching_the_gpu():
    from fdgs import _capi
    scene, bi, cg = _capi.FdgsScene(), _capi.FdgsBackwardIn(), _capi.FdgsCameraGrads()
    scene.P, scene.W, scene.H = 0, 16, 16
    buf = (C.c_float * 64)()
    big = C.c_size_t(1 << 20)
    call = lambda s, i, g, scr, n: _capi.lib.fdgs_camera_backward(s, i, None, g, scr, n, None)   # noqa: E731
    assert call(None, C.byref(bi), C.byref(cg), buf, big) == 1
    # every output NULL
    assert call(C.byref(scene), C.byref(bi), C.byref(cg), buf, big) == 1 and "every output is NULL" in _capi.last_error()
    cg.dL_dcampos = C.cast(buf, C.c_void_p)
    # scratch missing / too small (decided before anything is launched: P = 0 needs one row of 36 floats)
    assert call(C.byref(scene), C.byref(bi), C.byref(cg), None, big) == 1 and "scratch" in _capi.last_error()
    assert call(C.byref(scene), C.byref(bi), C.byref(cg), buf, C.c_size_t(8)) == 1 and "scratch" in _capi.last_error()
    # wrong struct_size, each struct
    cg.struct_size -= 4
    assert call(C.byref(scene), C.byref(bi), C.byref(cg), buf, big) == 1 and "fdgs_camera_grads" in _capi.last_error()
    cg.struct_size += 4
    bi.struct_size += 8
    assert call(C.byref(scene), C.byref(bi), C.byref(cg), buf, big) == 1 and "fdgs_backward_in" in _capi.last_error()
    bi.struct_size -= 8
    scene.struct_size = 0
    assert call(C.byref(scene), C.byref(bi), C.byref(cg), buf, big) == 1 and "fdgs_scene" in _capi.last_error()
    scene.struct_size = C.sizeof(_capi.FdgsScene)
    # P > 0: an invalid scene, then missing backward inputs
    scene.P = 10
    assert call(C.byref(scene), C.byref(bi), C.byref(cg), buf, big) == 1 and "must not be NULL" in _capi.last_error()
    # the existing structs keep their sizes (no existing struct changes size or meaning)
    assert C.sizeof(_capi.FdgsBackwardOut) == _capi.FdgsBackwardOut().struct_size and _capi.FDGS_VERSION == 502


def _base_camera(pose="rig0", dtype=torch.float32, W=64, H=40):
    cam = synth.camera_for(pose, W, H)
    return types.SimpleNamespace(world_view_transform=cam["world_view_transform"].to(dtype), full_proj_transform=cam["full_proj_transform"].to(dtype),
                                 camera_center=cam["camera_center"].to(dtype), timestamp=0.7, FoVx=cam["FoVx"], FoVy=cam["FoVy"],
                                 image_width=W, image_height=H)


def test_learnable_camera_at_zero_delta_is_its_base_bit_for_bit():
    from fdgs.camera import LearnableCamera
    for pose in ("rig0", "rig2", "slant"):
        base = _base_camera(pose)
        cam = LearnableCamera(base)
        assert cam.pose_delta.shape == (6,) and cam.time_offset.shape == (1,) and float(cam.pose_delta.detach().abs().sum()) == 0.0
        for k in ("world_view_transform", "full_proj_transform", "camera_center"):
            got, want = getattr(cam, k), getattr(base, k)
            assert got.requires_grad and got.dtype == torch.float32
            assert torch.equal(got.detach().view(torch.int32), want.view(torch.int32)), k
        assert cam.timestamp.dim() == 0 and float(cam.timestamp.detach()) == float(torch.tensor(0.7, dtype=torch.float32)) and cam.timestamp.requires_grad
        assert cam.image_width == 64 and cam.FoVx == base.FoVx   # everything else is the base camera's


def _outputs(cam):
    return torch.cat([cam.world_view_transform.reshape(-1), cam.full_proj_transform.reshape(-1), cam.camera_center.reshape(-1),
                      cam.timestamp.reshape(-1)])


def test_learnable_camera_jacobian_against_central_differences():
    """d(all 36 outputs)/d(pose_delta, time_offset) from autograd against float64 central differences, at zero (the series branch of
    the exponential map: finite and correct there) and at a twist on the closed-form branch."""
    from fdgs.camera import LearnableCamera
    base = _base_camera("rig2", torch.float64)
    for xi in (torch.zeros(6, dtype=torch.float64), torch.tensor([0.11, -0.07, 0.05, 0.03, -0.02, 0.04], dtype=torch.float64)):
        cam = LearnableCamera(base)
        assert cam.pose_delta.dtype == torch.float64
        with torch.no_grad():
            cam.pose_delta.copy_(xi)
            cam.time_offset.fill_(0.013)
        J = torch.stack([torch.cat([g.reshape(-1) for g in torch.autograd.grad(o, [cam.pose_delta, cam.time_offset], retain_graph=True, allow_unused=True,
                                                                              materialize_grads=True)]) for o in _outputs(cam)])
        assert torch.isfinite(J).all()
        h = 1e-6
        for j in range(7):
            d = torch.zeros(7, dtype=torch.float64)
            d[j] = h
            vals = []
            for sgn in (+1, -1):
                with torch.no_grad():
                    cam.pose_delta.copy_(xi + sgn * d[:6])
                    cam.time_offset.fill_(0.013 + sgn * float(d[6]))
                    vals.append(_outputs(cam).clone())
            fd = (vals[0] - vals[1]) / (2 * h)
            assert float((J[:, j] - fd).abs().max()) <= 1e-8 * max(1.0, float(fd.abs().max())), (j, float((J[:, j] - fd).abs().max()))
    # the rotation part really is a rotation, applied on the left of V: V' = exp(xi) V
    E = cam.world_view_transform.detach()[:3, :3].T @ torch.linalg.inv(base.world_view_transform[:3, :3].T)
    R = E
    assert float((R @ R.T - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-12 and abs(float(torch.linalg.det(R)) - 1) < 1e-12


def test_camera_centre_is_the_inverse_translation_and_the_projection_follows_the_pose():
    from fdgs.camera import LearnableCamera
    base = _base_camera("rig0", torch.float64)
    cam = LearnableCamera(base)
    with torch.no_grad():
        cam.pose_delta.copy_(torch.tensor([0.02, -0.3, 0.1, 0.5, -0.2, 0.3], dtype=torch.float64))
    V = cam.world_view_transform.detach()
    assert float((cam.camera_center.detach() - torch.linalg.inv(V)[3, :3]).abs().max()) < 5e-6   # (the base centre is a float32 inverse of a float32 matrix: a few ulp of 4)
    proj = torch.linalg.solve(base.world_view_transform, base.full_proj_transform)
    assert float((cam.full_proj_transform.detach() - V @ proj).abs().max()) < 1e-6


def test_timestamp_gradient_identity_against_a_finite_difference_of_the_oracle():
    """dL/dtimestamp = -sum_i dL/dts_i (camera_oracle's reference) against a central difference of the oracle in ``timestamp`` with the
    lists held, on one small rot_4d scene with 4D SH."""
    cfg = synth.SceneConfig("t", 300, 48, 40, 3, 2, 0.05, 6.0, True, 4, False)
    scene = co.build_scene(cfg, "rig0", seed=3)
    up = synth.make_upstream_grads(scene["W"], scene["H"], seed=2, scale=1e-2)
    lists = co.oracle_lists(scene)
    assert int((lists["radii"] > 0).sum()) > 50
    ref, _ = co.camera_reference(scene, up, lists)
    h = 1e-5
    fd = (co.oracle_loss_at(scene, up, lists, scene["timestamp"] + h) - co.oracle_loss_at(scene, up, lists, scene["timestamp"] - h)) / (2 * h)
    assert abs(float(ref["timestamp"][0])) > 1e-3
    assert abs(fd - float(ref["timestamp"][0])) <= 1e-6 * max(1.0, abs(fd)), (fd, ref["timestamp"])
    # and the structurally zero entries of the two matrices are zero in the reference too
    assert not ref["viewmatrix"].reshape(-1)[co.ZERO_VIEW].any() and not ref["projmatrix"].reshape(-1)[co.ZERO_PROJ].any()
    assert np.abs(ref["campos"]).max() > 0
