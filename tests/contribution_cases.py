"""Scenes of the contribution-statistics tests (tests/test_contribution_oracle_host.py, tests/test_gpu_contribution.py) and their
oracle results, computed once per scene and shared.

Poses and seeds are fixed here; they were picked on the CPU so that the pixels the GPU test has to exclude (the oracle's ``border``
pixels and the restatement's ``near_tie`` pixels) stay far below its 1 % cap by the oracle alone."""
import functools

import numpy as np
import torch

from util import run_oracle, synth

import contribution_oracle as co

SC = synth.SceneConfig

# name -> (config, pose, seed): P, W x H, SH / time degree, s0, model
CONFIGS = {
    "a": (SC("ca", 700, 72, 56, 1, 0, 0.06, 1.0, True, 4, False), "axis", 0),     # rot_4d
    "b": (SC("cb", 1500, 97, 61, 3, 2, 0.05, 10.0, True, 4, False), "rig0", 1),   # rot_4d, 4D SH; one border pixel: the exclusion map is used
    "c": (SC("cc", 400, 40, 33, 2, 0, 0.08, 1.0, False, 3, False), "rig0", 1),    # 3D
    "d": (SC("cd", 3000, 130, 70, 0, 0, 0.04, 1.0, False, 4, True), "axis", 1),   # 4D without rot_4d
    # opaque: opacity 0.95 and scales large enough that pixels saturate -- the early-termination path (T < 1e-4)
    "opaque": (SC("co", 900, 72, 56, 1, 0, 0.16, 1.0, True, 4, False), "rig0", 0),
    # edge images with a handful of Gaussians
    "1x1": (SC("e1", 12, 1, 1, 0, 0, 0.5, 1.0, True, 4, True), "axis", 0),
    "8x8": (SC("e8", 24, 8, 8, 1, 0, 0.3, 1.0, True, 4, False), "axis", 0),
    "17x9": (SC("e17", 40, 17, 9, 0, 0, 0.25, 1.0, False, 3, False), "axis", 1),
}


def make(name, pose=None, timestamp_frac=0.5):
    cfg, p, seed = CONFIGS[name]
    scene = synth.make_scene(cfg, seed=seed, pose=p if pose is None else pose, timestamp_frac=timestamp_frac)
    if name == "opaque":
        scene["opacities"] = torch.full_like(scene["opacities"], 0.95)
    if name in ("1x1", "8x8", "17x9"):
        # a handful of Gaussians in front of a tiny image: pull them onto the optical axis and into the view's moment
        scene["means3D"][:, 0:2] *= 0.02
        scene["ts"] = torch.full_like(scene["ts"], scene["timestamp"])
    return scene


@functools.lru_cache(maxsize=None)
def oracle(name, pose=None, timestamp_frac=0.5):
    """(scene, the port oracle's forward, the restatement's walk, exclusion map) of a case; cached: treat as read-only.
    exclusion map: bool [H,W], the oracle's ``border`` pixels (the alpha = 1/255 and T = 1e-4 cliffs) and the ``near_tie`` pixels."""
    scene = make(name, pose, timestamp_frac)
    ref, _ = run_oracle(scene, None, kind="port")
    W, H = int(scene["W"]), int(scene["H"])
    wk = co.walk(ref, W, H)
    excl = ref["border"].astype(bool) | wk["near_tie"]
    return scene, ref, wk, excl


def random_weights(H, W, seed):
    """A weight map with about 30 % zeros, the rest in (0.25, 2)."""
    g = np.random.default_rng(seed)
    w = (0.25 + 1.75 * g.random((H, W))).astype(np.float32)
    w[g.random((H, W)) < 0.3] = 0.0
    return w
