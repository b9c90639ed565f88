"""The written definition of the frame decode (fdgs.frames, csrc/frames.hip) in numpy float32: what the reference's loader computes
for an 8-bit image -- utils/general_utils.py:22-28 ``PILtoTorch`` (``np.array(pil) / 255.0``, [H, W, C] -> [C, H, W]) and
scene/cameras.py:53-57 (``image *= gt_alpha_mask``) -- as exactly these IEEE fp32 operations in this order:

    v = float32(u8) / float32(255)            every channel (a division; a product with 1/255 differs for 126 of the 256 bytes)
    C = 4:  mask = a / 255,  rgb = v * mask   ((u * a) / 65025 differs for 37 247 of the 65 536 pairs)

tests/golden/frames/*.npz hold the reference's own results; this file equals them bit for bit (tests/test_frames_host.py).
"""
import numpy as np

F255 = np.float32(255.0)


def decode(frames_u8):
    """uint8 [N, H, W, C] (C = 3 or 4) -> (images float32 [N, 3, H, W], masks float32 [N, 1, H, W] or None)."""
    u = np.asarray(frames_u8)
    if u.dtype != np.uint8 or u.ndim != 4 or u.shape[3] not in (3, 4):
        raise ValueError("frames must be uint8 [N, H, W, 3 or 4]")
    v = (u.astype(np.float32) / F255).astype(np.float32)
    v = np.ascontiguousarray(v.transpose(0, 3, 1, 2))
    if u.shape[3] == 3:
        return v, None
    mask = v[:, 3:4]
    return np.ascontiguousarray((v[:, :3] * mask).astype(np.float32)), np.ascontiguousarray(mask)


def wrong_reciprocal(frames_u8):
    """The kernel one must NOT write: a product with the rounded reciprocal (used by the tests to show that they tell the difference)."""
    u = np.asarray(frames_u8).astype(np.float32)
    return np.ascontiguousarray((u * (np.float32(1.0) / F255)).astype(np.float32).transpose(0, 3, 1, 2))


def wrong_fused(rgb_u8, a_u8):
    """The other one: (u * a) / 65025 instead of two divisions and a product."""
    return ((rgb_u8.astype(np.float32) * a_u8.astype(np.float32)) / np.float32(65025.0)).astype(np.float32)
