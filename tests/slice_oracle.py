"""float64 numpy statement of what ``fdgs.slice.time_slice`` computes, written from the formulas (forward.cu:242-352, 431-437, 133-192).

Every function takes ACTIVATED parameters (``activate`` turns a model's raw float32 parameters into them in float64) and returns
per-Gaussian arrays for ALL P Gaussians plus the live mask; the compaction is ``[live]``.
"""
import numpy as np

REF_PI = 3.14159265   # the reference's truncated pi (auxiliary.h:20): the forward's time factors are built on it
LIVE_BAR = 0.05


def activate(raw):
    """Raw float32 parameters (numpy, keys as GaussianParams.NAMES) -> the float64 activated inputs of ``slice_oracle``."""
    f = lambda k: np.asarray(raw[k], np.float64)  # noqa: E731
    out = {"xyz": f("_xyz"), "opacity": 1.0 / (1.0 + np.exp(-f("_opacity").reshape(-1))), "scales": np.exp(f("_scaling")),
           "scales_t": np.exp(f("_scaling_t").reshape(-1)), "rot": f("_rotation"), "ts": np.asarray(raw["_t"]).reshape(-1),
           "shs": np.asarray(raw["_features"])}
    if raw.get("_rotation_r") is not None:
        out["rot_r"] = f("_rotation_r")
    return out


def _unit(q):
    return q / np.maximum(np.sqrt((q * q).sum(1, keepdims=True)), 1e-12)


def sigma4(scales, scales_t, rot, rot_r, mod):
    """[P,4,4]: Sigma = R^T S^2 R, R = M_r M_l the product of the right- and left-isoclinic rotations (forward.cu:315-335)."""
    a, b, c, d = _unit(rot).T
    p, q, r, s = _unit(rot_r).T
    # the reference fills its matrices column by column: these literals are the COLUMNS
    Ml = np.array([[a, b, -c, d], [-b, a, d, c], [c, -d, a, b], [-d, -c, -b, a]]).transpose(2, 1, 0)
    Mr = np.array([[p, q, -r, -s], [-q, p, s, -r], [r, -s, p, -q], [s, r, q, p]]).transpose(2, 1, 0)
    R = Mr @ Ml
    S = mod * np.concatenate([scales, scales_t.reshape(-1, 1)], axis=1)
    M = S[:, :, None] * R
    return M.transpose(0, 2, 1) @ M


def sigma3(scales, rot, mod):
    """[P,3,3]: R S^2 R^T with R the rotation of the unit quaternion (w, x, y, z) (forward.cu:242-276)."""
    R = rotation_matrix(rot)
    S2 = (mod * scales) ** 2
    return (R * S2[:, None, :]) @ R.transpose(0, 2, 1)


def rotation_matrix(q):
    """build_rotation (utils/general_utils.py): [n,3,3] of quaternions (w, x, y, z), normalised first."""
    w, x, y, z = _unit(np.asarray(q, np.float64)).T
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]).transpose(2, 0, 1)


def upper6(S):
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], axis=1)


def full3(c6):
    c = np.asarray(c6, np.float64)
    return np.stack([np.stack([c[:, 0], c[:, 1], c[:, 2]], 1), np.stack([c[:, 1], c[:, 3], c[:, 4]], 1),
                     np.stack([c[:, 2], c[:, 4], c[:, 5]], 1)], 1)


def time_factors(ts, t, T):
    """(t1, t2) of the forward: dir_t = ts - t in the dtype of ``ts`` (the kernels subtract in fp32), the cosine in double."""
    ts = np.asarray(ts)
    dir_t = (ts - ts.dtype.type(t)).astype(np.float64)
    return np.cos(2 * REF_PI * dir_t / T), np.cos(2 * REF_PI * dir_t * 2 / T)


def fold_sh(shs, t1, t2, D, D_t, force_sh_3d=False):
    """[P,16,3] float64: block 0 up to (D + 1)^2 coefficients, the time blocks where the forward has them (4D SH, D == 3)."""
    shs = np.asarray(shs, np.float64)
    P = shs.shape[0]
    n0 = min(16, (D + 1) ** 2)
    out = np.zeros((P, 16, 3))
    out[:, :n0] = shs[:, :n0]
    nblocks = 1 + min(max(D_t, 0), 2) if (not force_sh_3d and D > 2) else 1
    if nblocks > 1:
        out += t1[:, None, None] * shs[:, 16:32]
    if nblocks > 2:
        out += t2[:, None, None] * shs[:, 32:48]
    return out


def slice_oracle(p, t, mod=1.0, prefilter_var=-1.0, rot_4d=True, D=0, D_t=0, T=1.0, force_sh_3d=False):
    """``p``: activated parameters (see ``activate``).  Returns marginal, live, index, xyz, cov6, opacity (all P rows) and, when
    ``p`` has ``shs``, the folded rows."""
    ts64 = np.asarray(p["ts"], np.float64).reshape(-1)
    xyz = np.asarray(p["xyz"], np.float64)
    if rot_4d:
        Sig = sigma4(p["scales"], p["scales_t"], p["rot"], p["rot_r"], mod)
        cov_t = Sig[:, 3, 3]
        c12 = Sig[:, :3, 3]
        cond = Sig[:, :3, :3] - c12[:, :, None] * c12[:, None, :] / cov_t[:, None, None]
        dt = t - ts64
        xyz = xyz + c12 / cov_t[:, None] * dt[:, None]
    else:
        cond = sigma3(p["scales"], p["rot"], mod)
        cov_t = np.asarray(p["scales_t"], np.float64).reshape(-1) * mod   # a variance, not squared: the reference's quirk
        dt = ts64 - t
    var = cov_t + prefilter_var if prefilter_var > 0.0 else cov_t
    marginal = np.exp(-0.5 * dt * dt / var)
    live = marginal > LIVE_BAR
    out = {"marginal": marginal, "live": live, "index": np.nonzero(live)[0].astype(np.int32), "xyz": xyz, "cov6": upper6(cond),
           "opacity": np.asarray(p["opacity"], np.float64).reshape(-1) * marginal,
           "cliff": np.abs(marginal - LIVE_BAR) <= 1e-5 * LIVE_BAR}
    if p.get("shs") is not None:
        t1, t2 = time_factors(np.asarray(p["ts"]).reshape(-1), t, T)
        out["t1"], out["t2"] = t1, t2
        out["shs"] = fold_sh(p["shs"], t1, t2, D, D_t, force_sh_3d)
    return out


def sliced_scene(scene, sl):
    """The 3D scene dict (fdgs.synth keys) of an oracle slice ``sl`` of the 4D ``scene``: precomputed covariances, folded SH rows."""
    import torch
    live = sl["live"]
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32)))  # noqa: E731
    out = {k: v for k, v in scene.items() if k not in ("ts", "scales", "scales_t", "rotations", "rotations_r", "flow_2d")}
    out.update(means3D=f32(sl["xyz"][live]), cov3D_precomp=f32(sl["cov6"][live]), opacities=f32(sl["opacity"][live]).reshape(-1, 1),
               shs=f32(sl["shs"][live]), M=16, P=int(live.sum()), sh_degree_t=0, rot_4d=False, gaussian_dim=3, force_sh_3d=False,
               scale_modifier=1.0, prefilter_var=-1.0)
    return out
