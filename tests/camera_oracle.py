"""TEST INFRASTRUCTURE: the reference for the camera gradients (fdgs_camera_backward), from the float64 PyTorch statement of the
forward (oracle/torch_oracle.py) and autograd.

The discrete decisions (culls, radii, tile lists, n_contrib) come from the C oracle, as everywhere; ``world_view_transform``,
``full_proj_transform`` and ``camera_center`` enter ``torch_oracle.render`` as leaves (its ``.to(dtype)`` returns the same tensor when
the dtype already matches), the loss is sum(out * g) over colour, depth and alpha = 1 - out_T with the ``make_upstream_grads`` tensors.

``timestamp`` is a float in the oracle.  The forward depends on time ONLY through ``timestamp - ts_i`` (the temporal marginal and the
conditional mean shift take ``timestamp - ts``, the non-rotated marginal and the 4D-SH time factors ``ts - timestamp``), so
dL/dtimestamp = -sum_i dL/dts_i, which autograd gives; tests/test_camera_host.py checks that identity once against a central
difference of the oracle in ``timestamp``.
"""
import numpy as np
import torch

from oracle import pyoracle, torch_oracle
from util import synth

CAMERA_KEYS = ("world_view_transform", "full_proj_transform", "camera_center")
# the entries no path reaches: the view matrix' column that t does not read, the projection's depth column (row-major [4,4])
ZERO_VIEW = [3, 7, 11, 15]
ZERO_PROJ = [2, 6, 10, 14]


def build_scene(cfg, pose, seed=5, colors_precomp=False, scale_modifier=1.0, prefilter_var=-1.0, P=None, alloc=None, timestamp_frac=0.45):
    """A synth scene (camera from ``pose``) with the settings the tests vary; ``colors_precomp``: colours instead of SH."""
    scene = synth.make_scene(cfg, seed=seed, bg=(0.2, 0.1, 0.4), pose=pose, P=P, alloc=alloc, timestamp_frac=timestamp_frac)
    scene["scale_modifier"], scene["prefilter_var"] = float(scale_modifier), float(prefilter_var)
    if colors_precomp:
        g = torch.Generator().manual_seed(seed + 1)
        scene["colors_precomp"] = torch.rand(scene["P"], 3, generator=g)
        scene["shs"] = None
    return scene


def to_raw(scene):
    """The same scene as RAW parameters (fdgs_scene.raw_params = 1): log scales, logit opacity, quaternions of a norm other than 1."""
    out = dict(scene)
    out["scales"] = torch.log(scene["scales"])
    out["scales_t"] = torch.log(scene["scales_t"])
    out["opacities"] = torch.logit(scene["opacities"].clamp(1e-6, 1 - 1e-6))
    out["rotations"] = scene["rotations"] * 1.7
    out["rotations_r"] = scene["rotations_r"] * 0.6
    return out


def oracle_lists(scene):
    o = pyoracle.Oracle(scene, kind="port")
    lists = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in o.forward().items()}
    o.close()
    return lists


def loss_of(out, up, dtype):
    return ((out["out_color"] * up["grad_color"].to(dtype)).sum() + (out["out_depth"] * up["grad_depth"][0].to(dtype)).sum()
            + ((1 - out["out_T"]) * up["grad_alpha"][0].to(dtype)).sum())


def camera_reference(scene, up, lists=None, dtype=torch.float64):
    """{"viewmatrix" [4,4], "projmatrix" [4,4], "campos" [3], "timestamp" [1]} float64 numpy: dL/d(camera) of the oracle's forward in
    ``dtype`` arithmetic; also returns the loss value."""
    lists = oracle_lists(scene) if lists is None else lists
    sc = dict(scene)
    leaves = {}
    for k in CAMERA_KEYS:
        leaves[k] = scene[k].detach().to(dtype).clone().requires_grad_(True)
        sc[k] = leaves[k]
    need_ts = scene["gaussian_dim"] == 4
    out, p = torch_oracle.render(sc, lists, dtype=dtype, requires_grad=("ts",) if need_ts else ())
    loss = loss_of(out, up, dtype)
    zero = {"viewmatrix": np.zeros((4, 4)), "projmatrix": np.zeros((4, 4)), "campos": np.zeros(3), "timestamp": np.zeros(1)}
    if not loss.requires_grad:   # nothing visible
        return zero, float(loss.detach())
    loss.backward()
    g = lambda t, shape: np.zeros(shape) if t.grad is None else t.grad.double().numpy()   # noqa: E731
    ref = {"viewmatrix": g(leaves["world_view_transform"], (4, 4)), "projmatrix": g(leaves["full_proj_transform"], (4, 4)),
           "campos": g(leaves["camera_center"], (3,)),
           "timestamp": np.array([-float(p["ts"].grad.sum())]) if need_ts and p["ts"].grad is not None else np.zeros(1)}
    return ref, float(loss.detach())


def oracle_loss_at(scene, up, lists, timestamp):
    """The oracle's loss with the lists held and another timestamp (for the finite difference of the identity above)."""
    with torch.no_grad():
        out, _ = torch_oracle.render(dict(scene, timestamp=float(timestamp)), lists, dtype=torch.float64)
        return float(loss_of(out, up, torch.float64))


def bars(scene, up, lists, ref64):
    """Per tensor: the bar the kernel is held to.  The project's bar is 1e-4 * max(1, max|ref|).  These are long cancelling sums over
    P: where float32 arithmetic of the SAME formulas (torch_oracle.render(dtype=float32) on the same input) cannot meet that bar
    itself, the kernel is held to 4 x the float32 oracle's error instead (as tests/test_gpu_loss_edges.py does for the loss): the bar
    is max(plain bar, 4 x that error) and never looks at a kernel's output.
    Returns {name: (bar, plain bar, float32 oracle's error)}."""
    ref32, _ = camera_reference(scene, up, lists, dtype=torch.float32)
    out = {}
    for k, r in ref64.items():
        plain = 1e-4 * max(1.0, float(np.abs(r).max()))
        e32 = float(np.abs(ref32[k] - r).max())
        out[k] = (max(plain, 4.0 * e32), plain, e32)
    return out
