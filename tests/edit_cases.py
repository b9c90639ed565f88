"""Cases shared by tests/test_edit_host.py, tests/test_gpu_edit.py and tests/golden/make_golden_edit.py: the argument errors of
fdgs_model_transform, the models and transforms of the GPU tests, and the two sides of the render-invariance reference."""
import ctypes as C
import math

import numpy as np
import torch

import edit_oracle as eo
from fdgs import synth

W, H = 96, 64
SIZES = (1, 63, 64, 65, 257, 4099)
R_GEN = eo.axis_angle((0.3, -0.5, 0.8), 1.1)         # a non-axis rotation
T_GEN = (0.4, -0.25, 0.6)
# name -> (R, T, s, a, b)
TRANSFORMS = {
    "eq": (R_GEN, T_GEN, 0.7, 0.7, 0.2),               # rot_4d: the closed form
    "half": (R_GEN, T_GEN, 0.5, 1.0, 0.0),             # rot_4d: re-decomposition
    "fast": (eo.random_rotation(21), (-1.0, 0.5, 0.25), 2.0, 0.5, -0.3),
    "pi": (eo.axis_angle((1, 1, 0), math.pi), (0.0, 0.0, 0.0), 1.0, 1.0, 0.0),   # closed form, a half turn, nothing else
    "scale_only": (np.eye(3), (0.0, 0.0, 0.0), 1.5, 1.5, 0.0),
}
MODES = {"3d": dict(rot_4d=False, dim=3, alloc=(3, 0)), "4d": dict(rot_4d=False, dim=4, alloc=(3, 2)), "rot4d": dict(rot_4d=True, dim=4, alloc=(3, 2))}
RENDER_CASES = ("eq", "half")
RENDER_POSE = "rig1"
GOLDEN = "edit_render_psnr.json"


def similarity(name):
    from fdgs.edit import Similarity
    R, T, s, a, b = TRANSFORMS[name]
    return Similarity(R, T, s, a, b)


def make_scene(P, mode, D=3, D_t=2, seed=3, pose="rig1", duration=1.0):
    m = MODES[mode]
    D_t = D_t if m["dim"] == 4 and D == 3 else 0
    cfg = synth.SceneConfig("edit", P, W, H, D, D_t, 0.03, duration, m["rot_4d"], m["dim"], False)
    return synth.make_scene(cfg, seed=seed, bg=(0.1, 0.2, 0.3), pose=pose, alloc=m["alloc"], rot_sigma="uniform",
                            st_scale=0.6 if m["rot_4d"] else 0.2)


def make_model(scene, dev, unnormalised=True):
    """GaussianParams of ``scene``; ``unnormalised``: the raw quaternions get norms in about [0.3, 3] (what a trained model holds)."""
    from fdgs.train_host import GaussianParams
    model = GaussianParams(scene, dev)
    if unnormalised:
        g = torch.Generator().manual_seed(17)
        P = model.P
        with torch.no_grad():
            model._rotation.mul_(torch.exp(0.6 * torch.randn(P, 1, generator=g)).to(dev))
            model._rotation_r.mul_(torch.exp(0.6 * torch.randn(P, 1, generator=g)).to(dev))
    return model


def raw_numpy(model):
    return {k: v.detach().cpu().numpy().copy() for k, v in model.params.items()}


def psnr(a, b, peak):
    mse = float(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2))
    return 150.0 if mse <= 0.0 else min(150.0, 10.0 * math.log10(peak * peak / mse))


# ---- the render-invariance reference: both sides as scene dicts of the CPU oracle ----
def render_scene():
    return make_scene(4099, "rot4d", D=3, D_t=2, seed=3, pose=RENDER_POSE)


def camera_through(scene, R, T, s, a, b):
    """The camera entries of ``scene`` seen through the transform, in float64 from the definitions: view rotation R_view R^T, centre
    s R c + T, the same projection."""
    Wt = scene["world_view_transform"].numpy().astype(np.float64)
    proj_t = np.linalg.inv(Wt) @ scene["full_proj_transform"].numpy().astype(np.float64)
    Rv = Wt[:3, :3].T
    c = -Rv.T @ Wt[3, :3]
    c2 = s * np.asarray(R) @ c + np.asarray(T, np.float64)
    V = np.eye(4)
    V[:3, :3] = Rv @ np.asarray(R).T
    V[:3, 3] = -V[:3, :3] @ c2
    f32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32))  # noqa: E731
    return {"world_view_transform": f32(V.T), "full_proj_transform": f32(V.T @ proj_t), "camera_center": f32(c2),
            "timestamp": a * scene["timestamp"] + b}


def near_band_is_empty(scene, s):
    """The precondition of the render comparison: no Gaussian between the near cull z > 0.2 and its image under the scale."""
    x = scene["means3D"].numpy().astype(np.float64)
    z = (np.concatenate([x, np.ones((x.shape[0], 1))], 1) @ scene["world_view_transform"].numpy().astype(np.float64))[:, 2]
    lo, hi = 0.2 * min(1.0, 1.0 / s), 0.2 * max(1.0, 1.0 / s)
    return not bool(((z >= lo) & (z <= hi)).any())


def transformed_reference_scene(scene, raw, name):
    """``scene`` with float64-transformed parameters rounded to fp32 (activated: what the oracle takes) and the camera through the
    transform.  ``raw``: the model's raw fp32 parameters (numpy)."""
    R, T, s, a, b = TRANSFORMS[name]
    xyz, t, _, _ = eo.transformed_means(raw, R, T, s, a, b)
    r32 = eo.to_fp32(eo.decompose4(eo.transformed_cov4(raw, R, s, a)))
    D = eo.sh_rotation_fit(R)
    shs = raw["_features"].astype(np.float64)
    P, M = shs.shape[:2]
    shs = np.einsum("ij,pbjc->pbic", D, shs.reshape(P, M // 16, 16, 3)).reshape(P, M, 3)
    f32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32))  # noqa: E731
    q = lambda k: r32[k].astype(np.float64) / np.linalg.norm(r32[k].astype(np.float64), axis=1, keepdims=True)  # noqa: E731
    out = dict(scene)
    out.update(means3D=f32(xyz), ts=f32(t.reshape(-1, 1)), scales=f32(np.exp(r32["_scaling"].astype(np.float64))),
               scales_t=f32(np.exp(r32["_scaling_t"].astype(np.float64))), rotations=f32(q("_rotation")), rotations_r=f32(q("_rotation_r")),
               shs=f32(shs), time_duration=a * scene["time_duration"])
    out.update(camera_through(scene, R, T, s, a, b))
    return out


def original_reference_scene(scene, raw):
    """``scene`` with the activations of the model's raw fp32 parameters (float64, rounded): the other side of the comparison."""
    f32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32))  # noqa: E731
    n = lambda k: raw[k].astype(np.float64) / np.linalg.norm(raw[k].astype(np.float64), axis=1, keepdims=True)  # noqa: E731
    out = dict(scene)
    out.update(scales=f32(np.exp(raw["_scaling"].astype(np.float64))), scales_t=f32(np.exp(raw["_scaling_t"].astype(np.float64))),
               rotations=f32(n("_rotation")), rotations_r=f32(n("_rotation_r")),
               opacities=f32(1.0 / (1.0 + np.exp(-raw["_opacity"].astype(np.float64)))))
    return out


# ---- the ABI's argument errors ----
def args():
    """Valid arguments of fdgs_model_transform for an empty model (P = 0: nothing is launched)."""
    from fdgs import _capi
    a_in, a_out = _capi.FdgsTransformIn(), _capi.FdgsTransformOut()
    a_in.P, a_in.M, a_in.gaussian_dim, a_in.rot_4d = 0, 16, 4, 1
    a_in.scale, a_in.time_scale = 1.0, 1.0
    return a_in, a_out


def abi_rejections():
    """(what, mutate(a_in, a_out), text of fdgs_last_error): every argument error of fdgs_model_transform.  Only the cases that need
    P > 0 -- a missing tensor, SH rows on one side -- have it, with fake pointers that are never dereferenced: those checks come before
    any launch.  Every other case keeps P = 0 and no pointers, so that a check that went missing would return FDGS_OK without a launch
    instead of starting kernels on unmapped addresses."""
    fake = 0x1000

    def full(a_in, a_out):
        a_in.P = 8
        for n in ("means3D", "ts", "scales", "scales_t", "rotations", "rotations_r", "shs"):
            setattr(a_in, n, fake)
            setattr(a_out, n, fake)

    def then(f):
        def g(a_in, a_out):
            full(a_in, a_out)
            f(a_in, a_out)
        return g
    cases = [("negative P", lambda i, o: setattr(i, "P", -1), "bad sizes"),
             ("P = 2^26", lambda i, o: setattr(i, "P", 1 << 26), "bad sizes"),
             ("NULL means3D", then(lambda i, o: setattr(i, "means3D", None)), "must not be NULL"),
             ("NULL out rotations", then(lambda i, o: setattr(o, "rotations", None)), "must not be NULL"),
             ("NULL ts", then(lambda i, o: setattr(i, "ts", None)), "must not be NULL"),
             ("NULL out scales_t", then(lambda i, o: setattr(o, "scales_t", None)), "must not be NULL"),
             ("NULL rotations_r", then(lambda i, o: setattr(i, "rotations_r", None)), "must not be NULL"),
             ("one-sided shs", then(lambda i, o: setattr(o, "shs", None)), "both sides"),
             ("zero scale", lambda i, o: setattr(i, "scale", 0.0), "positive"),
             ("negative scale", lambda i, o: setattr(i, "scale", -1.0), "positive"),
             ("zero time_scale", lambda i, o: setattr(i, "time_scale", 0.0), "positive"),
             ("negative time_scale", lambda i, o: setattr(i, "time_scale", -0.5), "positive"),
             ("NaN scale", lambda i, o: setattr(i, "scale", float("nan")), "positive"),
             ("gaussian_dim 5", lambda i, o: setattr(i, "gaussian_dim", 5), "gaussian_dim"),
             ("rot_4d in 3D", lambda i, o: setattr(i, "gaussian_dim", 3), "rot_4d needs")]
    for M in (0, 2, 15, 17, 64):
        cases.append(("M = %d" % M, lambda i, o, M=M: setattr(i, "M", M), "M=%d" % M))
    return cases


def check_abi_rejections():
    from fdgs import _capi
    assert _capi.lib.fdgs_model_transform(None, None, None) == 1 and "NULL" in _capi.last_error()
    a_in, a_out = args()
    assert _capi.lib.fdgs_model_transform(None, C.byref(a_out), None) == 1 and "NULL" in _capi.last_error()
    assert _capi.lib.fdgs_model_transform(C.byref(a_in), None, None) == 1 and "NULL" in _capi.last_error()
    for what, mutate, text in abi_rejections():
        a_in, a_out = args()
        mutate(a_in, a_out)
        assert _capi.lib.fdgs_model_transform(C.byref(a_in), C.byref(a_out), None) == 1, what
        assert text in _capi.last_error(), (what, _capi.last_error())
