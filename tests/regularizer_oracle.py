"""CPU oracle of the reference trainer's extra loss terms (train.py:119-159) and of its k-NN query (pointops2 knnquery).

numpy / torch on the CPU, float64 or float32.  Each expression is restated from the reference:
* knn:       utils/general_utils.py:170-184 -> pointops2 knnquery: the k nearest sources of every query, SQUARED distances.
             Rows here are ordered by (d2, source index); d2 = (dx*dx + dy*dy) + dz*dz in float32 (the kernel's rounding).
             Empty slots: d2 = 1e10, index 0 (the reference kernel's initial heap).
* velocity:  scene/gaussian_model.py:34-47 (build_covariance_from_scaling_rotation_4d, mean_offset = cov_12 / cov_t * dt) with
             the timestamp gaussians.get_t + 0.1 of train.py:143, so dt = (t + 0.1) - t, computed in float32 as the reference's
             float32 tensors do; scale = exp(cat(_scaling, _scaling_t)) (get_scaling_xyzt), L = R4(_rotation, _rotation_r) diag(s)
             (utils/general_utils.py:113-145: the quaternions are normalised there).
* rigid:     train.py:141-149:  sum(exp(-100 dist) * |v[idx] - v[i]|) / k / N.
* motion:    train.py:153-156:  mean_i |v_i|.
* opa mask:  train.py:120-128:  o = alpha.clamp(1e-6, 1 - 1e-6); mean(-(1 - gt_alpha_mask) * log(1 - o)).
"""
import numpy as np
import torch

EMPTY_D2 = 1e10


def knn(x: np.ndarray, src: np.ndarray, k: int, rows=None, chunk: int = 256):
    """Brute force over [n, 3] / [m, 3] float32 arrays (one batch).  Returns (idx int64 [r, k], d2 float32 [r, k]) for the query
    rows ``rows`` (default: all)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    src = np.ascontiguousarray(src, dtype=np.float32)
    rows = np.arange(x.shape[0]) if rows is None else np.asarray(rows)
    m = src.shape[0]
    out_i = np.zeros((len(rows), k), dtype=np.int64)
    out_d = np.full((len(rows), k), EMPTY_D2, dtype=np.float32)
    if m == 0:
        return out_i, out_d
    for b in range(0, len(rows), chunk):
        q = x[rows[b:b + chunk]]
        dx = src[None, :, 0] - q[:, None, 0]
        dy = src[None, :, 1] - q[:, None, 1]
        dz = src[None, :, 2] - q[:, None, 2]
        d2 = (dx * dx + dy * dy) + dz * dz                      # float32 throughout, no fused multiply-add
        for r in range(q.shape[0]):
            row = d2[r]
            kk = min(k, m)
            kth = np.partition(row, kk - 1)[kk - 1]
            cand = np.nonzero(row <= kth)[0]
            cand = cand[np.lexsort((cand, row[cand]))][:kk]    # (d2, index) ascending
            cand = cand[row[cand] < EMPTY_D2]                   # the reference's heap never takes d2 >= 1e10
            out_i[b + r, :len(cand)] = cand
            out_d[b + r, :len(cand)] = row[cand]
    return out_i, out_d


def dt_of(t: torch.Tensor) -> torch.Tensor:
    """(t + 0.1) - t in float32 (train.py:143 -> gaussian_model.py:251), as a constant."""
    t32 = t.detach().float()
    return (t32 + 0.1) - t32


def velocity(scaling, scaling_t, rotation, rotation_r, t, dtype=torch.float64, dt=None) -> torch.Tensor:
    """v [P, 3] from the raw parameters; differentiable in the four tensors (t only enters through dt, which has no gradient).
    ``dt``: a constant in place of dt_of(t), for the host test's deliberately wrong statement."""
    s = torch.exp(torch.cat([scaling, scaling_t], dim=1).to(dtype))
    ql = rotation.to(dtype)
    qr = rotation_r.to(dtype)
    ql = ql / torch.norm(ql, dim=-1, keepdim=True)
    qr = qr / torch.norm(qr, dim=-1, keepdim=True)
    a, b, c, d = ql.unbind(-1)
    p, q, r, w = qr.unbind(-1)
    Ml = torch.stack([a, -b, -c, -d, b, a, -d, c, c, d, a, -b, d, -c, b, a], dim=1).view(-1, 4, 4)
    Mr = torch.stack([p, q, r, w, -q, p, -w, r, -r, w, p, -q, -w, -r, q, p], dim=1).view(-1, 4, 4)
    R = (Ml @ Mr).flip(1, 2)
    L = R * s.unsqueeze(1)                                      # R @ diag(s)
    sigma = L @ L.transpose(1, 2)
    c12, ct = sigma[:, 0:3, 3], sigma[:, 3, 3:4]
    return c12 / ct * (dt_of(t).to(dtype) if dt is None else dt)


def valid_entries(idx: torch.Tensor, P: int) -> torch.Tensor:
    """The entries of a neighbour table that name a Gaussian: the kernels skip every other one (n < 0 or n >= P)."""
    return (idx >= 0) & (idx < P)


def rigid(v: torch.Tensor, idx: torch.Tensor, d2: torch.Tensor, mask=None) -> torch.Tensor:
    """idx [P, k] int64, d2 [P, k] (the squared distances the query returned).  ``mask`` [P, k] bool: entries that are False
    contribute nothing and their index is not read (valid_entries: how the kernels treat an index outside [0, P))."""
    P, k = idx.shape
    w = torch.exp(-100 * d2.to(v.dtype))
    if mask is not None:
        idx = torch.where(mask, idx, torch.zeros_like(idx))
        w = w * mask.to(v.dtype)
    vd = torch.norm(v[idx] - v[:, None, :], p=2, dim=-1)
    return (w * vd).sum() / k / P


def motion(v: torch.Tensor) -> torch.Tensor:
    return v.norm(p=2, dim=1).mean()


# torch.clamp(1e-6, 1 - 1e-6) on a float32 tensor compares against the bounds rounded to float32: the float64 oracle of a float32
# alpha takes these bounds (float32(1e-6) < 1e-6, so the double bound would block the gradient at the float32 lower bound)
OPA_BOUNDS_F32 = (float(np.float32(1e-6)), float(np.float32(1 - 1e-6)))


def opa_mask(alpha: torch.Tensor, gt_alpha_mask: torch.Tensor, bounds=(1e-6, 1 - 1e-6)) -> torch.Tensor:
    o = alpha.clamp(*bounds)
    sky = 1 - gt_alpha_mask
    return (-sky * torch.log(1 - o)).mean()


NAMES4 = ("_scaling", "_scaling_t", "_rotation", "_rotation_r")


def rigid_motion_with_grads(params, idx, d2, dtype=torch.float64, g_rigid=1.0, g_motion=1.0, mask=None):
    """params: dict of CPU tensors _scaling, _scaling_t, _rotation, _rotation_r, _t.  Returns (L_rigid, L_motion, grads dict) of
    g_rigid * L_rigid + g_motion * L_motion with respect to the four raw tensors, computed in ``dtype``.  ``mask``: see rigid()."""
    leaves = {n: params[n].detach().to(dtype).clone().requires_grad_(True) for n in NAMES4}
    v = velocity(leaves["_scaling"], leaves["_scaling_t"], leaves["_rotation"], leaves["_rotation_r"], params["_t"], dtype)
    lr = rigid(v, torch.as_tensor(idx), torch.as_tensor(d2), mask)
    lm = motion(v)
    (g_rigid * lr + g_motion * lm).backward()
    return float(lr.detach()), float(lm.detach()), {n: t.grad.detach() for n, t in leaves.items()}


# ---- the bar a float32 kernel's gradients are held to ----
#
# bar = K * max(e32, 4 eps32 max|ref64|) per tensor, absolute, with NO floor: e32 = max|float32 statement - float64 statement| of
# that tensor on that input (both from rigid_motion_with_grads) is the measurement of what float32 can do there -- 2e-7 .. 4e-7 of
# max|ref64| for _scaling, _rotation and _rotation_r, 1e-4 .. 2e-3 for _scaling_t, whose derivative is a cancelling sum in any
# float32 implementation -- and K covers a kernel that evaluates in another order than torch.  K is measured, not chosen: 4 times the
# largest |hip - ref64| / max(e32, 4 eps32 max|ref64|) seen on the GPU over all cases of tests/regularizer_cases.py, rounded up to
# a power of two, at least 8 ("Regulariser gradients", has the ratios).
EPS32 = float(np.finfo(np.float32).eps)
GRAD_BAR_K = {"_scaling": 8.0, "_scaling_t": 64.0, "_rotation": 8.0, "_rotation_r": 8.0, "velocity": 8.0}


class Bar:
    """ref: the float64 statement; unit = max(e32, 4 eps32 max|ref|); bar = K * unit."""

    def __init__(self, name, ref, f32):
        self.name, self.ref = name, ref
        self.ref_max = float(ref.abs().max()) if ref.numel() else 0.0
        self.e32 = float((f32.double() - ref).abs().max()) if ref.numel() else 0.0
        self.unit = max(self.e32, 4 * EPS32 * self.ref_max)
        self.bar = GRAD_BAR_K[name] * self.unit

    def err(self, got) -> float:
        got = got.detach().cpu().double().reshape(self.ref.shape)
        return float((got - self.ref).abs().max()) if torch.isfinite(got).all() else float("inf")

    def ratio(self, got) -> float:
        """err / unit (0 / 0 = 0: an exact zero reference met exactly): a kernel passes where this is <= K."""
        e = self.err(got)
        return e / self.unit if self.unit > 0 else (0.0 if e == 0 else float("inf"))

    def accepts(self, got) -> bool:
        return self.err(got) <= self.bar


def grad_bar(params, idx, d2, g_rigid, g_motion, mask=None):
    """Per tensor of NAMES4: a Bar with the float64 reference gradient of g_rigid * L_rigid + g_motion * L_motion and its bar."""
    g64 = rigid_motion_with_grads(params, idx, d2, torch.float64, g_rigid, g_motion, mask)[2]
    g32 = rigid_motion_with_grads(params, idx, d2, torch.float32, g_rigid, g_motion, mask)[2]
    return {n: Bar(n, g64[n], g32[n]) for n in NAMES4}


def velocity_bar(params):
    """The same bar for the velocity output."""
    args = [params[n] for n in NAMES4 + ("_t",)]
    with torch.no_grad():
        return Bar("velocity", velocity(*args, torch.float64), velocity(*args, torch.float32))
