"""Golden fixtures for the frame decode (fdgs.frames, csrc/frames.hip): 8-bit images and the float tensors the REFERENCE's own
loader makes of them on the CPU -- ``utils.general_utils.PILtoTorch`` on a PIL image of the requested resolution (Pillow's resize is
then the identity: asserted below), split into colour and alpha as utils/camera_utils.py:43-48 does, then ``scene.cameras.Camera(...,
image=..., gt_alpha_mask=..., data_device="cpu")`` for ``.image`` and ``.gt_alpha_mask``.  The reference's imports that are not
installed (pointops2, kornia) are stubbed; nothing of them is used here.

Shapes: RGB and RGBA; H*W and W not multiples of 4; an RGB shape with H*W*3 not a multiple of 4 and three frames (frames that do not
start on a dword); every byte value among the colours, and alpha planes holding 0, 255 and everything between.

    python tests/golden/make_golden_frames.py   ->   tests/golden/frames/*.npz
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

for name, attrs in (("pointops2", ()), ("pointops2.functions", ()), ("pointops2.functions.pointops", ("furthestsampling", "knnquery")),
                    ("kornia", ("create_meshgrid",))):
    mod = types.ModuleType(name)
    for a in attrs:
        setattr(mod, a, None)
    sys.modules[name] = mod
sys.path.insert(0, REF)
from utils.general_utils import PILtoTorch  # noqa: E402
# scene/cameras.py by its path: the package's __init__ imports the dataset readers and their dependencies
_spec = importlib.util.spec_from_file_location("ref_scene_cameras", os.path.join(REF, "scene", "cameras.py"))
_cameras = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_cameras)
Camera = _cameras.Camera

# name -> (N, H, W, C, seed)
CASES = {"rgb_3x17x20": (3, 17, 20, 3, 1),      # H*W = 340: dword-aligned frames, the 4-pixel path
         "rgb_3x13x15": (3, 13, 15, 3, 2),      # H*W = 195, H*W*3 = 585: frames 1 and 2 start off a dword, the byte-wise path
         "rgba_2x13x15": (2, 13, 15, 4, 3),     # H*W = 195: the 4-pixel path with a tail of 3 pixels, frame 1 not 16-byte aligned
         "rgba_2x16x18": (2, 16, 18, 4, 4)}     # W = 18 not a multiple of 4, H*W = 288: every alpha value in each plane


def frames(N, H, W, C, seed):
    g = np.random.default_rng(seed)
    n = N * H * W
    u = np.empty((n, C), dtype=np.uint8)
    for c in range(C):   # every byte value in every channel, in an order of its own; the rest random
        col = np.concatenate([np.arange(256), g.integers(0, 256, max(0, n - 256))])[:n] if n >= 256 else g.integers(0, 256, n)
        if c == 3 and H * W >= 256:   # each frame's alpha plane holds all 256 values
            col = np.concatenate([g.permutation(np.concatenate([np.arange(256), g.integers(0, 256, H * W - 256)])) for _ in range(N)])
        else:
            col = g.permutation(col)
        u[:, c] = col.astype(np.uint8)
    return u.reshape(N, H, W, C)


def reference(frame):
    """One uint8 [H, W, C] image through the reference's loader."""
    H, W, C = frame.shape
    pil = Image.fromarray(frame, "RGB" if C == 3 else "RGBA")
    assert np.array_equal(np.array(pil.resize((W, H))), frame), "Pillow's resize to the same size must be the identity"
    t = PILtoTorch(pil, (W, H))
    assert t.dtype == torch.float32 and tuple(t.shape) == (C, H, W)
    image, mask = t[:3, ...], (t[3:4, ...] if C == 4 else None)
    cam = Camera(colmap_id=0, R=np.eye(3), T=np.zeros(3), FoVx=0.8, FoVy=0.6, image=image, gt_alpha_mask=mask, image_name="f", uid=0,
                 data_device="cpu", resolution=(W, H))
    return cam.image.numpy().copy(), (None if mask is None else cam.gt_alpha_mask.numpy().copy())


if __name__ == "__main__":
    os.makedirs(os.path.join(HERE, "frames"), exist_ok=True)
    for name, (N, H, W, C, seed) in CASES.items():
        u8 = frames(N, H, W, C, seed)
        out = [reference(f) for f in u8]
        data = {"u8": u8, "image": np.stack([o[0] for o in out]).astype(np.float32)}
        if C == 4:
            data["mask"] = np.stack([o[1] for o in out]).astype(np.float32)
            assert all(len(np.unique(u8[i, :, :, 3])) == 256 for i in range(N)) or H * W < 256
            assert {0, 255} <= set(np.unique(u8[..., 3]).tolist()) and len(np.unique(u8[..., 3])) == 256
        assert len(np.unique(u8[..., :3])) == 256
        path = os.path.join(HERE, "frames", name + ".npz")
        np.savez_compressed(path, **data)
        print(name, u8.shape, "%d bytes" % os.path.getsize(path))
