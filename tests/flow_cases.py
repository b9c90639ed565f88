"""Scenes and cameras shared by tests/test_flow_host.py and tests/test_gpu_flow.py: 64 x 48 images, at most 1000 Gaussians."""
import numpy as np
import torch

import flow_oracle as fo
from fdgs import synth

W, H = 64, 48
T0, T1 = 0.4, 0.5          # source and target time, duration 1
ROT_SIGMA = 0.3            # far enough from the identity that the Gaussians move by tens of pixels per unit of time


class Cam:
    """The camera members render() and gaussian_flow() read, from a synth scene dict."""

    def __init__(self, scene, dev="cpu", timestamp=None):
        self.FoVx, self.FoVy, self.image_height, self.image_width = scene["FoVx"], scene["FoVy"], scene["H"], scene["W"]
        self.world_view_transform = scene["world_view_transform"].to(dev)
        self.full_proj_transform = scene["full_proj_transform"].to(dev)
        self.camera_center = scene["camera_center"].to(dev)
        self.timestamp = scene["timestamp"] if timestamp is None else float(timestamp)


def make_scene(P, rot_4d, pose, t, seed=3, gaussian_dim=4):
    cfg = synth.SceneConfig("flow", P, W, H, 0, 0, 0.03, 1.0, rot_4d, gaussian_dim, False)
    return synth.make_scene(cfg, seed=seed, pose=pose, timestamp_frac=t, rot_sigma=ROT_SIGMA)


def pair(P, rot_4d, poses, seed=3, gaussian_dim=4, t1=T1):
    """(source scene at T0 seen from poses[0], target scene at t1 seen from poses[1]): the same Gaussians."""
    return make_scene(P, rot_4d, poses[0], T0, seed, gaussian_dim), make_scene(P, rot_4d, poses[1], t1, seed, gaussian_dim)


def params_of(scene, raw):
    """The six tensors by flow_oracle.NAMES; ``raw``: logarithms of the scales and quaternions of norm 0.5 .. 1.5."""
    par = {n: scene[n].clone() for n in fo.NAMES}
    if raw:
        P = par["means3D"].shape[0]
        par["scales"], par["scales_t"] = par["scales"].log(), par["scales_t"].log()
        g = torch.Generator().manual_seed(5)
        par["rotations"] = par["rotations"] * (0.5 + torch.rand(P, 1, generator=g))
        par["rotations_r"] = par["rotations_r"] * (0.5 + torch.rand(P, 1, generator=g))
    return par


def cam_args(s0, s1):
    """The leading arguments of flow_oracle.gaussian_flow for the two scenes' cameras."""
    return (s0["world_view_transform"], s0["full_proj_transform"], s0["timestamp"], s1["world_view_transform"], s1["full_proj_transform"],
            s1["timestamp"], W, H)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)
