"""Golden rays of the environment-map composite, produced by the REFERENCE's own ``Camera.get_rays`` (scene/cameras.py:75-82) on the
CPU, for three DyNeRF-style cameras (cx / cy / fl_x / fl_y given: the centre-shift projection, scene/cameras.py:66-67):
python tests/golden/make_golden_envmap.py <reference checkout>  ->  tests/golden/envmap/rays.npz

``kornia.create_meshgrid`` (the one kornia call of get_rays) is stubbed with the same pixel grid written in torch.  Each case stores
the camera's world_view_transform, camera_center, intrinsics and the rays, so that tests/test_envmap_host.py pins the ray convention
of tests/envmap_oracle.py to the reference's code."""
import importlib.util
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if len(sys.argv) != 2:
    raise SystemExit(__doc__)
sys.path.insert(0, os.path.abspath(sys.argv[1]))


def create_meshgrid(height, width, normalized_coordinates=True, device=None, dtype=torch.float32):
    assert not normalized_coordinates
    ys, xs = torch.meshgrid(torch.arange(height, dtype=dtype), torch.arange(width, dtype=dtype), indexing="ij")
    return torch.stack([xs, ys], -1)[None]   # [1, H, W, 2] in (x, y) order


sys.modules["kornia"] = types.SimpleNamespace(create_meshgrid=create_meshgrid)
# scene/cameras.py alone (scene/__init__.py pulls in the dataset readers and their dependencies)
_spec = importlib.util.spec_from_file_location("ref_scene_cameras", os.path.join(os.path.abspath(sys.argv[1]), "scene", "cameras.py"))
_mod = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_mod)
Camera = _mod.Camera


def rot(yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    return Rz @ Rx @ Ry


# (W, H, camera-to-world rotation angles, centre, focal, principal offset from the image centre)
CASES = {
    "front": (96, 72, (0.0, 0.0, 0.0), (0.0, 0.0, -4.0), 86.4, (3.5, -2.25)),
    "rig": (88, 64, (-0.17, 0.12, -0.08), (0.7, -0.45, -4.3), 79.2, (-6.0, 4.5)),
    "equator": (80, 60, (-1.2, -1.5707963, 0.2), (1.5, 2.0, 0.5), 60.0, (2.25, 1.75)),
}
out = {}
for name, (W, H, ang, centre, focal, off) in CASES.items():
    R = rot(*ang)                                       # camera-to-world, the R Camera receives (getWorld2View2 transposes it)
    T = -R.T @ np.asarray(centre, dtype=np.float64)      # world-to-view translation
    cx, cy = 0.5 * W + off[0], 0.5 * H + off[1]
    fovx, fovy = 2 * math.atan(W / (2 * focal)), 2 * math.atan(H / (2 * focal))
    cam = Camera(0, R, T, fovx, fovy, None, None, name, 0, data_device="cpu", cx=cx, cy=cy, fl_x=focal, fl_y=focal,
                 resolution=(W, H), meta_only=True)
    o, d = cam.get_rays()
    out[name + "_world_view_transform"] = cam.world_view_transform.numpy().astype(np.float32)
    out[name + "_camera_center"] = cam.camera_center.numpy().astype(np.float32)
    out[name + "_intrinsics"] = np.array([focal, focal, cx, cy], dtype=np.float64)
    out[name + "_origin"] = o.reshape(3).numpy().astype(np.float32)
    out[name + "_dirs"] = d.numpy().astype(np.float32)
np.savez_compressed(os.path.join(HERE, "envmap", "rays.npz"), **out)   # (a directory of its own: tests/golden_util.py reads every golden/*.npz as a rasterizer case)
print(len(CASES), "cameras")
