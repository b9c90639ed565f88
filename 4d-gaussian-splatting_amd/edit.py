"""Place, retime and merge 4D models: ``Similarity``, ``transform``, ``transform_camera``, ``merge``, ``extract``.

The map is ``x' = s R x + T`` in space and ``t' = a t + b`` in time.  ``transform`` applies it to a model's RAW parameters in HIP
(csrc/model_transform.hip, ``fdgs_model_transform``): one pass over the 17 geometry floats of every Gaussian and one over the SH rows.

Conventions (all restated from the kernels' headers and checked against them in tests/):

* quaternions are ``(w, x, y, z)``; the world-space 3D covariance of a Gaussian is ``R(q) S^2 R(q)^T`` with the usual rotation matrix of
  ``q`` (``quat_to_R`` stores its transpose column-major), so a rotated Gaussian has ``q' = q_R * q`` (Hamilton product);
* with ``rot_4d`` the covariance is ``R4^T S^2 R4``, ``R4 = M_r(q_r) M_l(q_l)`` (``build_Ml_Mr`` in csrc/fdgs_math.h).  The two
  isoclinic families commute and each is closed under the product, so for ``s == a`` the rotation folds into the stored quaternions:
  ``R4' = R4 diag(R, 1)^T`` and ``diag(R, 1)^T = M_r(u) M_l(v)`` (``isoclinic_pair``) give ``q_l' = q_l * v``, ``q_r' = q_r * u``.  For
  ``s != a`` the eigenvectors change: the kernel re-decomposes ``A Sigma A^T``, ``A = diag(s R, a)``, with a cyclic Jacobi in double;
* the colour is 16 real-SH coefficients per block of a row, up to three blocks (time basis 1, cos, cos 2): every block's bands 1-3 are
  multiplied by ``sh_rotation(R)``, the DC coefficient is left alone;
* without ``rot_4d`` ``exp(_scaling_t)`` is a VARIANCE (``+= 2 log a``), with it a standard deviation (``+= log a``); ``prefilter_var``
  is a variance in time (``* a^2``); the SH time basis is ``cos(2 pi k dt / T)`` with ``T`` the model's duration, which scales by ``a``
  exactly as ``dt`` does.

Not carried: an environment map (``transform`` raises) and the optimizer's Adam moments -- ``inplace=True`` rewrites the parameters
under a running optimizer without touching ``exp_avg`` / ``exp_avg_sq``, which then describe the old frame; re-create the optimizer
state (or keep training only what the transform leaves alone) after an in-place edit.  Opacity is never changed.

No gradients flow through an edit.
"""
import copy
import ctypes as C
import math

import numpy as np
import torch

from . import _capi, layout

SH_M = (1, 4, 9, 16, 32, 48)   # coefficients per Gaussian the SH pass knows how to walk
_BANDS = ((1, 4), (4, 9), (9, 16))

# csrc/fdgs_math.h SH_C0 .. SH_C3 as doubles
_C0 = 0.28209479177387814
_C1 = 0.4886025119029199
_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
       -0.5900435899266435)


def _sh_basis(d):
    """[n,16] float64: the basis of ``sh_tables`` (csrc/sh_eval.h) at unit directions ``d`` [n,3]."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    return np.stack([
        np.full_like(x, _C0), -_C1 * y, _C1 * z, -_C1 * x,
        _C2[0] * xy, _C2[1] * yz, _C2[2] * (2.0 * zz - xx - yy), _C2[3] * xz, _C2[4] * (xx - yy),
        _C3[0] * y * (3 * xx - yy), _C3[1] * xy * z, _C3[2] * y * (4 * zz - xx - yy), _C3[3] * z * (2 * zz - 3 * xx - 3 * yy),
        _C3[4] * x * (4 * zz - xx - yy), _C3[5] * z * (xx - yy), _C3[6] * x * (xx - 3 * yy)], axis=1)


def _as_rotation(rotation):
    """3x3 float64 from a 3x3 matrix or a unit (w, x, y, z) quaternion; ValueError unless it is a proper rotation."""
    r = np.asarray(rotation.detach().cpu().numpy() if isinstance(rotation, torch.Tensor) else rotation, np.float64)
    if not np.isfinite(r).all():
        raise ValueError("Similarity: the rotation has a non-finite entry")
    if r.shape == (4,):
        if abs(float(r @ r) - 1.0) > 2e-6:
            raise ValueError("Similarity: the quaternion must have unit norm (|q|^2 = %.9g)" % float(r @ r))
        w, x, y, z = r / math.sqrt(float(r @ r))
        r = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    if r.shape != (3, 3):
        raise ValueError("Similarity: rotation must be a 3x3 matrix or a (w, x, y, z) quaternion, got shape %s" % (r.shape,))
    if np.abs(r @ r.T - np.eye(3)).max() > 1e-6:
        raise ValueError("Similarity: the rotation is not orthonormal to 1e-6")
    if np.linalg.det(r) < 0.0:
        raise ValueError("Similarity: det R = -1 (a reflection); only proper rotations are supported")
    return r


def _quat_of(R):
    """Unit quaternion (w, x, y, z), w >= 0, of a rotation matrix (float64; the largest of the four candidates as the pivot)."""
    t = np.array([1 + R[0, 0] + R[1, 1] + R[2, 2], 1 + R[0, 0] - R[1, 1] - R[2, 2], 1 - R[0, 0] + R[1, 1] - R[2, 2],
                  1 - R[0, 0] - R[1, 1] + R[2, 2]])
    k = int(np.argmax(t))
    if k == 0:
        q = np.array([t[0], R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    elif k == 1:
        q = np.array([R[2, 1] - R[1, 2], t[1], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]])
    elif k == 2:
        q = np.array([R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], t[2], R[1, 2] + R[2, 1]])
    else:
        q = np.array([R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], t[3]])
    q = q / np.linalg.norm(q)
    return -q if q[0] < 0 else q


class Similarity:
    """``x' = scale * R x + translation``, ``t' = time_scale * t + time_shift``.  ``rotation``: a 3x3 matrix or a unit (w, x, y, z)
    quaternion (None: the identity).  Everything is held in float64."""

    def __init__(self, rotation=None, translation=(0.0, 0.0, 0.0), scale=1.0, time_scale=1.0, time_shift=0.0):
        self.R = np.eye(3) if rotation is None else _as_rotation(rotation)
        t = np.asarray(translation.detach().cpu().numpy() if isinstance(translation, torch.Tensor) else translation, np.float64)
        if t.shape != (3,):
            raise ValueError("Similarity: translation must have 3 entries")
        self.T = t.copy()
        self.s, self.a, self.b = float(scale), float(time_scale), float(time_shift)
        if not (np.isfinite(self.T).all() and all(math.isfinite(v) for v in (self.s, self.a, self.b))):
            raise ValueError("Similarity: every value must be finite")
        if not self.s > 0.0:
            raise ValueError("Similarity: scale must be positive (got %g)" % self.s)
        if not self.a > 0.0:
            raise ValueError("Similarity: time_scale must be positive (got %g)" % self.a)

    rotation = property(lambda self: self.R)
    translation = property(lambda self: self.T)
    scale = property(lambda self: self.s)
    time_scale = property(lambda self: self.a)
    time_shift = property(lambda self: self.b)

    def matrix(self):
        """4x4 float64: ``[[s R, T], [0, 1]]``."""
        m = np.eye(4)
        m[:3, :3] = self.s * self.R
        m[:3, 3] = self.T
        return m

    def inverse(self):
        Rt = self.R.T
        return Similarity(Rt, -(Rt @ self.T) / self.s, 1.0 / self.s, 1.0 / self.a, -self.b / self.a)

    def compose(self, other):
        """``self`` after ``other``: ``self.compose(other)(x) == self(other(x))``."""
        return Similarity(_reorthonormalize(self.R @ other.R), self.s * (self.R @ other.T) + self.T, self.s * other.s,
                          self.a * other.a, self.a * other.b + self.b)

    def apply(self, xyz, t=None):
        """float64 numpy: the mapped points [n,3] (and times)."""
        x = np.asarray(xyz, np.float64) @ (self.s * self.R).T + self.T
        return x if t is None else (x, self.a * np.asarray(t, np.float64) + self.b)

    def __repr__(self):
        return "Similarity(q=%s, T=%s, s=%g, a=%g, b=%g)" % (np.round(_quat_of(self.R), 6).tolist(), self.T.tolist(), self.s, self.a, self.b)


def _reorthonormalize(R):
    u, _, vt = np.linalg.svd(R)
    return u @ vt


def sh_rotation(R) -> np.ndarray:
    """[16,16] float64, block diagonal (1, 3, 5, 7): the matrix ``D`` with ``sum_k (D c)_k Y_k(R d) = sum_k c_k Y_k(d)`` for the basis
    of ``sh_tables`` (csrc/sh_eval.h).  Each band is invariant under rotation, ``Y(R d) = Q Y(d)``; ``Q`` is projected out by a
    quadrature that is exact for the band's polynomials (Gauss-Legendre in z, equispaced in the azimuth) and ``D = Q^-T``."""
    R = _as_rotation(R)
    zs, wz = np.polynomial.legendre.leggauss(8)
    nphi = 16
    phi = (np.arange(nphi) + 0.5) * (2.0 * math.pi / nphi)
    z = np.repeat(zs, nphi)
    rho = np.sqrt(1.0 - z * z)
    d = np.stack([rho * np.tile(np.cos(phi), zs.size), rho * np.tile(np.sin(phi), zs.size), z], axis=1)
    w = np.repeat(wz, nphi) * (2.0 * math.pi / nphi)
    Y, Yr = _sh_basis(d), _sh_basis(d @ R.T)
    D = np.zeros((16, 16))
    D[0, 0] = 1.0
    for lo, hi in _BANDS:
        B = (Yr[:, lo:hi] * w[:, None]).T @ Y[:, lo:hi]
        G = (Y[:, lo:hi] * w[:, None]).T @ Y[:, lo:hi]
        Q = B @ np.linalg.inv(G)
        D[lo:hi, lo:hi] = np.linalg.inv(Q).T
    return D


def _Ml(q):
    """M_l of ``build_Ml_Mr`` as a mathematical matrix [row, column] (the header's literals are its columns)."""
    a, b, c, d = q
    return np.array([[a, b, -c, d], [-b, a, d, c], [c, -d, a, b], [-d, -c, -b, a]], np.float64).T


def _Mr(q):
    p, q_, r, s = q
    return np.array([[p, q_, -r, -s], [-q_, p, s, -r], [r, -s, p, -q_], [s, r, q_, p]], np.float64).T


def _iso_coefficients(R4):
    """K[a, b] = <M_r(e_a) M_l(e_b), R4> / 4: for ``R4 = M_r(u) M_l(v)`` the rank-1 matrix ``u v^T`` (the 16 products are orthogonal
    signed permutations)."""
    e = np.eye(4)
    return np.array([[float((_Mr(e[a]) @ _Ml(e[b]) * R4).sum()) / 4.0 for b in range(4)] for a in range(4)])


def isoclinic_pair(R):
    """Unit quaternions ``(u, v)``, float64, with ``M_r(u) M_l(v) = diag(R, 1)^T`` in the conventions of ``build_Ml_Mr``: every SO(4)
    matrix is bilinear in ``(q_r, q_l)`` with a rank-1 coefficient matrix, whose dominant singular pair is the two quaternions.  The
    pair is unique up to a common sign; the component of ``u`` that is largest in magnitude is made positive."""
    R = _as_rotation(R)
    G = np.eye(4)
    G[:3, :3] = R.T
    K = _iso_coefficients(G)
    U, S, Vt = np.linalg.svd(K)
    u, v = U[:, 0] * math.sqrt(S[0]), Vt[0] * math.sqrt(S[0])
    u, v = u / np.linalg.norm(u), v / np.linalg.norm(v)
    if u[int(np.argmax(np.abs(u)))] < 0.0:
        u, v = -u, -v
    return u, v


# ---- the model pass ----
# the tensors fdgs_model_transform maps, in the order of its ABI structs: means3D, ts, scales, scales_t, rotations, rotations_r, shs
_ORDER = tuple(layout.BY_KERNEL[k].name for k in ("means3D", "ts", "scales", "scales_t", "rotations", "rotations_r", "shs"))


def _sh_rows(D):
    """The 83 entries of bands 1-3 (3x3, 5x5, 7x7 row-major) as float32."""
    return np.concatenate([D[lo:hi, lo:hi].reshape(-1) for lo, hi in _BANDS]).astype(np.float32)


def _arguments(sim, gaussian_dim, rot_4d, M, inputs, outputs):
    """The two ABI structs of fdgs_model_transform.  ``inputs`` / ``outputs``: means3D, ts, scales, scales_t, rotations, rotations_r,
    shs (None: the segment is absent / not to be touched).  Everything derived from the rotation -- its quaternion, the isoclinic
    pair, the SH matrices -- is computed here, in float64; the tensors must stay alive until the call is made."""
    P = int(inputs[0].shape[0])
    u, v = isoclinic_pair(sim.R)
    p = _capi._ptr
    arr = lambda ty, vals: (ty * len(vals))(*[float(x) for x in vals])  # noqa: E731
    a_in = _capi.FdgsTransformIn(P, int(M), int(gaussian_dim), int(bool(rot_4d)), *[p(t) for t in inputs],
                                 arr(C.c_double, sim.R.reshape(-1)), arr(C.c_double, sim.T), sim.s, sim.a, sim.b,
                                 arr(C.c_double, _quat_of(sim.R)), arr(C.c_double, u), arr(C.c_double, v), math.log(sim.s), math.log(sim.a),
                                 arr(C.c_float, _sh_rows(sh_rotation(sim.R))))
    return a_in, _capi.FdgsTransformOut(*[p(t) for t in outputs])


def _enqueue(sim, gaussian_dim, rot_4d, M, inputs, outputs):
    """fdgs_model_transform on the current stream of the inputs' device."""
    a_in, a_out = _arguments(sim, gaussian_dim, rot_4d, M, inputs, outputs)
    _capi.call("fdgs_model_transform", inputs[0].device, C.byref(a_in), C.byref(a_out))


def transform(model, sim, *, inplace=False):
    """``model`` seen through ``sim``: a ``GaussianParams`` with the same degrees and flags whose Gaussians are the model's, moved.

    ``model``: raw ``_xyz, _opacity, _scaling, _rotation, _t, _scaling_t, _rotation_r`` and ``get_features`` (or ``_features``)
    [P, M, 3] on the GPU; ``gaussian_dim`` 3 or 4, with or without ``rot_4d``.  The WHOLE allocated SH row is rotated, not only the
    active degrees, so a later ``oneupSHdegree`` stays consistent.  ``time_duration`` becomes ``[a t0 + b, a t1 + b]``, a positive
    ``prefilter_var`` is multiplied by ``a^2``; opacity is untouched.  A model with an ``env_map`` raises: a background at infinity
    only rotates, and is not carried.

    ``inplace=True`` writes into the model's own tensors and returns the model; the SH rows must then be the model's single
    ``_features`` tensor (``get_features`` is not consulted: it may return a temporary), else ValueError.  The optimizer's Adam moments are NOT transformed:
    they then belong to the old frame (see the module docstring).

    The identity returns the input bit for bit.  With ``rot_4d`` and ``scale != time_scale`` the covariance is re-decomposed: the
    result has the same covariances to fp32 accuracy, other quaternions and an arbitrary order of the three spatial scales."""
    from .train_host import GaussianParams
    if getattr(model, "env_map", None) is not None:
        raise ValueError("transform: the model has an environment map, which a similarity transform does not carry")
    gd, rot_4d = int(model.gaussian_dim), bool(model.rot_4d)
    if gd not in (3, 4) or (rot_4d and gd != 4):
        raise ValueError("transform: gaussian_dim must be 3 or 4, rot_4d needs 4 (got %d, rot_4d = %s)" % (gd, rot_4d))
    if inplace:
        # a getter may build the rows on the fly (a reference-style model concatenates _features_dc and _features_rest): rotating that
        # temporary would move the geometry and leave the colour behind
        feats = getattr(model, "_features", None)
        if feats is None:
            raise ValueError("transform(inplace=True): the model must hold its SH rows as one _features tensor [P, M, 3]")
    else:
        feats = model.get_features if hasattr(model, "get_features") else model._features
    xyz = model._xyz
    _capi.need_gpu(xyz, "_xyz", what="the model")
    P, M = int(xyz.shape[0]), int(feats.shape[1])
    if M not in SH_M:
        raise ValueError("transform: %d SH coefficients per Gaussian; supported: %s" % (M, (SH_M,)))
    t0, t1 = float(model.time_duration[0]), float(model.time_duration[1])
    duration = [sim.a * t0 + sim.b, sim.a * t1 + sim.b]
    pv = float(model.prefilter_var)
    pv = pv * sim.a * sim.a if pv > 0.0 else pv
    have = lambda n: getattr(model, n, None) is not None and getattr(model, n).numel() > 0  # noqa: E731
    # the segments this model's mode reads: a 3D model's time columns and _rotation_r without rot_4d are placeholders (and a 4D
    # model may come without its time columns)
    reads = [n for n in layout.used(gd, rot_4d) if layout.BY_NAME[n].when != layout.DIM4 or have(n)]
    src = {n: (feats if n == "_features" else getattr(model, n)).detach() if n in reads else None for n in _ORDER}
    for n, t in src.items():
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda):
            if inplace:
                raise ValueError("transform(inplace=True): %s must be a contiguous float32 GPU tensor" % n)
            src[n] = _capi._dev_f32(t, n)
    if inplace:
        out, dst = model, dict(src)
    else:
        # from_raw copies every segment bit for bit; the pass below then overwrites the ones it maps
        raw = dict(layout.raw_of(model), **{n: src[n] for n in ("_xyz", "_features", "_scaling", "_rotation")})
        out = GaussianParams.from_raw(raw, xyz.device, **layout.settings_of(model))
        dst = {n: (getattr(out, n).detach() if src[n] is not None else None) for n in src}
    if P > 0:
        with torch.no_grad():
            _enqueue(sim, gd, rot_4d, M, [src[n] for n in _ORDER], [dst[n] for n in _ORDER])
    out.time_duration = duration
    out.prefilter_var = pv
    return out


def transform_camera(camera, sim):
    """The rigid camera that sees ``transform(model, sim)`` as ``camera`` saw ``model``: view rotation ``R_view R^T``, centre
    ``s R c + T``, timestamp ``a t + b``, the same intrinsics (a shallow copy of ``camera`` with ``world_view_transform``,
    ``full_proj_transform``, ``camera_center`` and ``timestamp`` replaced).  The image is the same; view-space depth is ``s`` times the
    original's -- and so is the distance of the fixed z > 0.2 near cull from the scene: Gaussians between 0.2 and 0.2 / s of the
    original camera (s < 1: those nearer than 0.2 / s are dropped; s > 1: those between 0.2 / s and 0.2 appear) render differently."""
    wv = camera.world_view_transform
    dev = wv.device
    Wt = wv.detach().cpu().numpy().astype(np.float64)          # V^T, V = [[R_view, t], [0, 1]]
    full = camera.full_proj_transform.detach().cpu().numpy().astype(np.float64)
    proj_t = np.linalg.solve(Wt, full)                          # P^T: full = V^T P^T
    Rv = Wt[:3, :3].T
    c = -Rv.T @ Wt[3, :3]
    c2 = sim.s * (sim.R @ c) + sim.T
    V2 = np.eye(4)
    V2[:3, :3] = Rv @ sim.R.T
    V2[:3, 3] = -V2[:3, :3] @ c2
    out = copy.copy(camera)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)  # noqa: E731
    out.world_view_transform = f32(V2.T)
    out.full_proj_transform = f32(V2.T @ proj_t)
    out.camera_center = f32(c2)
    out.timestamp = sim.a * float(camera.timestamp) + sim.b
    return out


# ---- torch glue: subsets and unions of models ----
def extract(model, mask):
    """The Gaussians of ``model`` that ``mask`` selects (a bool mask [P] or an index tensor), as a new model with the same settings."""
    from .train_host import GaussianParams
    if getattr(model, "env_map", None) is not None:
        raise ValueError("extract: the model has an environment map, which is not carried")
    dev = model._xyz.device
    mask = torch.as_tensor(mask, device=dev)
    if mask.dtype == torch.bool and mask.shape != (int(model._xyz.shape[0]),):
        raise ValueError("extract: the mask must have one entry per Gaussian")
    raw = {n: t[mask] for n, t in layout.raw_of(model).items()}
    return GaussianParams.from_raw(raw, dev, **layout.settings_of(model))


def merge(models):
    """One model of all the Gaussians of ``models``, in order.  The models must agree in ``gaussian_dim``, ``rot_4d``, ``force_sh_3d``,
    the SH row length ``M``, the maximum degrees and ``prefilter_var``; with an active time degree also in their duration
    ``t1 - t0`` (the time basis ``cos(2 pi k dt / T)`` is per model).  Active degrees become the maxima over the models,
    ``time_duration`` the union of the intervals -- with an active time degree ``[min t0, min t0 + T]``, since ``T = t1 - t0`` is all
    the renderer reads of it and must stay the models' common duration."""
    from .train_host import GaussianParams
    models = list(models)
    if not models:
        raise ValueError("merge: no models")
    sets = [layout.settings_of(m) for m in models]
    raws = [layout.raw_of(m) for m in models]
    first = sets[0]
    for i, (m, s, r) in enumerate(zip(models, sets, raws)):
        if getattr(m, "env_map", None) is not None:
            raise ValueError("merge: model %d has an environment map, which is not carried" % i)
        for key in ("gaussian_dim", "rot_4d", "force_sh_3d", "max_sh_degree", "max_sh_degree_t", "prefilter_var"):
            if s[key] != first[key]:
                raise ValueError("merge: model %d differs in %s (%s, model 0 has %s)" % (i, key, s[key], first[key]))
        if int(r["_features"].shape[1]) != int(raws[0]["_features"].shape[1]):
            raise ValueError("merge: model %d differs in M (%d SH coefficients, model 0 has %d)"
                             % (i, int(r["_features"].shape[1]), int(raws[0]["_features"].shape[1])))
        if set(r) != set(raws[0]):
            raise ValueError("merge: model %d holds other parameter tensors than model 0" % i)
    dur = [s["time_duration"][1] - s["time_duration"][0] for s in sets]
    if any(s["active_sh_degree_t"] > 0 for s in sets):
        for i, d in enumerate(dur):
            if abs(d - dur[0]) > 1e-6 * max(abs(dur[0]), abs(d)):
                raise ValueError("merge: model %d lasts %g, model 0 lasts %g, and a time degree is active: the SH time basis cos(2 pi k dt / T) "
                                 "cannot be shared; retime it first with time_scale = T_a / T_b = %g" % (i, d, dur[0], dur[0] / d))
    dev = models[0]._xyz.device
    raw = {n: torch.cat([r[n].to(dev) for r in raws], dim=0) for n in raws[0]}
    settings = dict(first)
    settings["active_sh_degree"] = max(s["active_sh_degree"] for s in sets)
    settings["active_sh_degree_t"] = max(s["active_sh_degree_t"] for s in sets)
    t0 = min(s["time_duration"][0] for s in sets)
    # the renderer reads only T = t1 - t0 (the SH time basis): with a time degree active it must stay the models' common duration
    t1 = t0 + dur[0] if settings["active_sh_degree_t"] > 0 else max(s["time_duration"][1] for s in sets)
    settings["time_duration"] = (t0, t1)
    return GaussianParams.from_raw(raw, dev, **settings)
