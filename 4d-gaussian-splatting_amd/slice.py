"""A 4D model at one timestamp as an ordinary 3D Gaussian scene: ``time_slice``, ``render_slice``, ``save_ply`` / ``load_ply``.

At time ``t`` a 4D Gaussian is exactly a 3D Gaussian:

* mean and covariance conditioned on ``t`` (``rot_4d``; otherwise the plain mean and ``R S^2 R^T``),
* opacity times the temporal marginal ``exp(-0.5 dt^2 / cov_t)`` (``cov_t + prefilter_var`` when the model has one),
* a plain degree-``D`` SH row with the time blocks folded in: ``sh[k] + cos(2 pi dt / T) sh[16 + k] + cos(4 pi dt / T) sh[32 + k]``.

``time_slice`` computes that in HIP (csrc/time_slice.hip, ``fdgs_time_slice``) for the Gaussians that pass the forward's own temporal
cull (marginal > 0.05) and returns them compacted, in ascending original index; where the forward keeps a Gaussian, mean, covariance
and opacity are the forward's bit for bit.  The reference's quirks are kept: without ``rot_4d`` the temporal variance is
``scaling_t * scaling_modifier``, not its square (forward.cu:431-436).

One quirk a slice cannot carry: the reference's 4D *kernel* path takes the SH view direction from the UNSHIFTED mean
(forward.cu:79-81), while its Python branch (gaussian_renderer/__init__.py:100-101) and any 3D viewer take it from the shifted one.
A slice is a 3D scene, so it is defined as the latter: ``render_slice`` equals ``render()`` of the 4D model exactly only where the two
directions coincide -- no ``rot_4d``, or SH degree 0 -- and differs by the view dependence of the colour over the mean shift elsewhere.

No gradients flow through a slice.
"""
import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _capi, layout

SH_ROW = 16   # coefficients per row of a slice: a full degree-3 row, zero beyond the active degree


@dataclass
class TimeSlice:
    """``n`` live Gaussians of a ``P``-Gaussian model at ``timestamp``; every tensor is the first ``n`` rows of a buffer of ``capacity`` rows."""
    n: int
    index: torch.Tensor                 # [n] int32, ascending: row -> Gaussian of the model
    xyz: torch.Tensor                   # [n, 3]
    cov3D: torch.Tensor                 # [n, 6] xx, xy, xz, yy, yz, zz
    opacity: torch.Tensor               # [n] sigmoid(raw) * marginal
    shs: torch.Tensor                   # [n, 16, 3]
    sh_degree: int
    scales: Optional[torch.Tensor]      # [n, 3] (decompose=True): cov3D = R(rotations) diag(scales^2) R^T
    rotations: Optional[torch.Tensor]   # [n, 4] unit (w, x, y, z)
    P: int = 0
    timestamp: float = 0.0


def time_slice(model, timestamp, scaling_modifier=1.0, *, decompose=False, capacity=None) -> TimeSlice:
    """The 3D Gaussians ``model`` (gaussian_dim == 4, raw parameters ``_xyz, _opacity, _scaling, _rotation, _t, _scaling_t,
    _rotation_r`` and ``get_features`` [P, M, 3] on the GPU) consists of at ``timestamp``.  ``decompose``: also ``scales`` /
    ``rotations`` of every covariance (an in-kernel Jacobi; what ``save_ply`` needs).  ``capacity``: rows of the output buffers
    (default P); more live Gaussians than that raise.  One host read (the live count) per call."""
    if int(model.gaussian_dim) != 4:
        raise ValueError("time_slice: the model is 3D (gaussian_dim == %d): it has no time to slice" % int(model.gaussian_dim))
    xyz = model._xyz
    _capi.need_gpu(xyz, "_xyz", what="the model")
    dev = xyz.device
    P = int(xyz.shape[0])
    cap = P if capacity is None else int(capacity)
    if cap < 0:
        raise ValueError("time_slice: capacity must not be negative")
    rot_4d = bool(model.rot_4d)
    f = _capi._dev_f32
    feats = f(model.get_features.detach(), "features")
    live = layout.used(4, rot_4d)
    g = {s.kernel: f(getattr(model, s.name).detach(), s.name) if s.name in live else None for s in layout.GEOMETRY}   # raw, by kernel name
    prefilter_var = float(model.prefilter_var) if float(model.prefilter_var) > 0.0 else -1.0
    D, D_t = int(model.active_sh_degree), int(model.active_sh_degree_t)
    fo = dict(dtype=torch.float32, device=dev)
    index = torch.empty((cap,), dtype=torch.int32, device=dev)
    o_xyz, o_cov, o_op, o_sh = torch.empty((cap, 3), **fo), torch.empty((cap, 6), **fo), torch.empty((cap,), **fo), torch.empty((cap, SH_ROW, 3), **fo)
    o_s = torch.empty((cap, 3), **fo) if decompose else None
    o_q = torch.empty((cap, 4), **fo) if decompose else None
    n_live = torch.empty((1,), dtype=torch.int32, device=dev)
    inputs = (g["means3D"], feats, g["opacities"], g["ts"], g["scales"], g["scales_t"], g["rotations"], g["rotations_r"])
    _enqueue(inputs, (D, D_t, float(scaling_modifier), prefilter_var, float(timestamp), float(model.time_duration[1] - model.time_duration[0]),
                      rot_4d, bool(model.force_sh_3d)), cap, (index, o_xyz, o_cov, o_op, o_sh, o_s, o_q), n_live)
    n = int(n_live.item())
    if n > cap:
        raise RuntimeError("time_slice: %d Gaussians are live at t = %g, the buffers hold %d (capacity)" % (n, float(timestamp), cap))
    return TimeSlice(n, index[:n], o_xyz[:n], o_cov[:n], o_op[:n], o_sh[:n], D, o_s[:n] if decompose else None, o_q[:n] if decompose else None,
                     P, float(timestamp))


def _enqueue(inputs, settings, cap, outputs, n_live):
    """fdgs_time_slice on the current stream.  ``inputs``: means3D, features, raw opacity, t, raw scaling, raw scaling_t, raw rotation,
    raw rotation_r (or None); ``settings``: D, D_t, scaling modifier, prefilter_var, timestamp, time duration, rot_4d, force_sh_3d;
    ``outputs``: index, xyz, cov3D, opacity, shs, scales, rotations (the last two None: no decomposition) of ``cap`` rows."""
    means3D, feats = inputs[0], inputs[1]
    dev, P = means3D.device, int(means3D.shape[0])
    D, D_t, mod, prefilter_var, timestamp, duration, rot_4d, force_sh_3d = settings
    scratch = _capi.scratch(_capi.lib.fdgs_time_slice_scratch_bytes(P), dev, floor=1)
    p = _capi._ptr
    a_in = _capi.FdgsSliceIn(P, int(D), int(D_t), int(feats.shape[1]) if P else 0, *[p(t) for t in inputs], float(mod), float(prefilter_var),
                             float(timestamp), float(duration), int(bool(rot_4d)), int(bool(force_sh_3d)))
    a_out = _capi.FdgsSliceOut(int(cap), *[p(t) for t in outputs], n_live.data_ptr())
    _capi.call("fdgs_time_slice", dev, C.byref(a_in), C.byref(a_out), scratch.data_ptr())


def _rasterize(slice: TimeSlice, camera, bg):
    """The rasterizer's 3D path on the compact slice: image, radii [n], depth, alpha, flow."""
    from .gaussian_renderer.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    rs = GaussianRasterizationSettings(
        image_height=int(camera.image_height), image_width=int(camera.image_width), tanfovx=math.tan(camera.FoVx * 0.5),
        tanfovy=math.tan(camera.FoVy * 0.5), bg=bg, scale_modifier=1.0, viewmatrix=camera.world_view_transform,
        projmatrix=camera.full_proj_transform, sh_degree=int(slice.sh_degree), sh_degree_t=0, campos=camera.camera_center,
        timestamp=float(slice.timestamp), time_duration=1.0, rot_4d=False, gaussian_dim=3, force_sh_3d=False, prefiltered=False, debug=False)
    with torch.no_grad():
        image, radii, depth, alpha, flow, _covs = GaussianRasterizer(rs)(
            means3D=slice.xyz, means2D=torch.zeros_like(slice.xyz), opacities=slice.opacity.reshape(-1, 1), shs=slice.shs,
            flow_2d=torch.zeros_like(slice.xyz[:, :2]), cov3D_precomp=slice.cov3D)
    return image, radii, depth, alpha, flow


def render_slice(slice: TimeSlice, camera, bg) -> dict:
    """The slice seen by ``camera`` over background ``bg`` through the rasterizer's 3D path (precomputed covariances, SH rows);
    ``render()``'s keys.  ``radii`` / ``visibility_filter`` have the MODEL's P entries, scattered back through ``slice.index`` as the
    reference does with its ``radii_all``: zero / False for every Gaussian that is not in the slice."""
    image, radii, depth, alpha, flow = _rasterize(slice, camera, bg)
    radii_all = radii.new_zeros((int(slice.P),))
    radii_all[slice.index.long()] = radii
    return {"render": image, "viewspace_points": torch.zeros((int(slice.P), 3), dtype=torch.float32, device=slice.xyz.device),
            "visibility_filter": radii_all > 0, "radii": radii_all, "depth": depth, "alpha": alpha, "flow": flow}


# ---- PLY in the common 3DGS layout ----
PLY_PROPERTIES = (["x", "y", "z", "nx", "ny", "nz"] + ["f_dc_%d" % i for i in range(3)] + ["f_rest_%d" % i for i in range(3 * (SH_ROW - 1))]
                  + ["opacity"] + ["scale_%d" % i for i in range(3)] + ["rot_%d" % i for i in range(4)])


def ply_fields(slice: TimeSlice) -> np.ndarray:
    """[n, 62] float32: the rows ``save_ply`` writes.  opacity as a logit, scales as logarithms -- of values clamped into the range
    where both are finite in fp32 (opacity to [1e-30, 1 - 2^-24], scales are floored by the kernel)."""
    if slice.scales is None or slice.rotations is None:
        raise ValueError("save_ply needs scales and rotations: take the slice with time_slice(..., decompose=True)")
    n = int(slice.n)
    cpu = lambda t: t.detach().cpu().numpy()  # noqa: E731
    rows = np.zeros((n, len(PLY_PROPERTIES)), np.float32)
    rows[:, 0:3] = cpu(slice.xyz)
    shs = cpu(slice.shs).reshape(n, SH_ROW, 3)
    rows[:, 6:9] = shs[:, 0, :]
    rows[:, 9:9 + 3 * (SH_ROW - 1)] = shs[:, 1:, :].transpose(0, 2, 1).reshape(n, 3 * (SH_ROW - 1))   # channel-major: all of R, then G, then B
    o = np.clip(cpu(slice.opacity).astype(np.float64).reshape(n), 1e-30, 1.0 - 2.0 ** -24)
    rows[:, 54] = np.log(o / (1.0 - o))
    rows[:, 55:58] = np.log(np.maximum(cpu(slice.scales).astype(np.float64), 1e-30))
    rows[:, 58:62] = cpu(slice.rotations)
    return rows


def save_ply(path, slice: TimeSlice) -> None:
    """Binary little-endian PLY: x y z nx ny nz f_dc_0..2 f_rest_0..44 opacity scale_0..2 rot_0..3, what 3DGS viewers read."""
    rows = ply_fields(slice)
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % rows.shape[0]
    header += "".join("property float %s\n" % name for name in PLY_PROPERTIES) + "end_header\n"
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(np.ascontiguousarray(rows.astype("<f4")).tobytes())


def load_ply(path, device):
    """A 3D model (``GaussianParams.from_raw``: raw parameters, 16 SH coefficients) from a PLY in the layout ``save_ply`` writes."""
    from .train_host import GaussianParams
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or "format binary_little_endian 1.0" not in lines:
        raise ValueError("load_ply: %s is not a binary little-endian PLY" % path)
    n = next(int(ln.split()[2]) for ln in lines if ln.startswith("element vertex"))
    props = [ln.split() for ln in lines if ln.startswith("property")]
    if any(pr[1] != "float" for pr in props):
        raise ValueError("load_ply: only float properties are supported")
    col = {pr[2]: i for i, pr in enumerate(props)}
    rows = np.frombuffer(data, dtype="<f4", count=n * len(props), offset=end).reshape(n, len(props)).astype(np.float32)
    n_rest = sum(1 for k in col if k.startswith("f_rest_"))
    if n_rest % 3 or any(k not in col for k in ("x", "y", "z", "f_dc_0", "f_dc_1", "f_dc_2", "opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3")):
        raise ValueError("load_ply: %s misses properties of the 3DGS layout" % path)
    M = 1 + n_rest // 3
    feats = np.zeros((n, M, 3), np.float32)
    feats[:, 0, :] = rows[:, [col["f_dc_%d" % i] for i in range(3)]]
    if n_rest:
        rest = rows[:, [col["f_rest_%d" % i] for i in range(n_rest)]]
        feats[:, 1:, :] = rest.reshape(n, 3, M - 1).transpose(0, 2, 1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    tensors = {"_xyz": t(rows[:, [col["x"], col["y"], col["z"]]]), "_features": t(feats), "_opacity": t(rows[:, [col["opacity"]]]),
               "_scaling": t(rows[:, [col["scale_%d" % i] for i in range(3)]]), "_rotation": t(rows[:, [col["rot_%d" % i] for i in range(4)]])}
    degree = int(round(math.sqrt(M))) - 1
    return GaussianParams.from_raw(tensors, device, max_sh_degree=degree, gaussian_dim=3, rot_4d=False)
