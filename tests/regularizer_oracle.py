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


def velocity(scaling, scaling_t, rotation, rotation_r, t, dtype=torch.float64) -> torch.Tensor:
    """v [P, 3] from the raw parameters; differentiable in the four tensors (t only enters through dt, which has no gradient)."""
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
    return c12 / ct * dt_of(t).to(dtype)


def rigid(v: torch.Tensor, idx: torch.Tensor, d2: torch.Tensor) -> torch.Tensor:
    """idx [P, k] int64, d2 [P, k] (the squared distances the query returned)."""
    P, k = idx.shape
    w = torch.exp(-100 * d2.to(v.dtype))
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


def rigid_motion_with_grads(params, idx, d2, dtype=torch.float64, g_rigid=1.0, g_motion=1.0):
    """params: dict of CPU tensors _scaling, _scaling_t, _rotation, _rotation_r, _t.  Returns (L_rigid, L_motion, grads dict) of
    g_rigid * L_rigid + g_motion * L_motion with respect to the four raw tensors, computed in ``dtype``."""
    leaves = {n: params[n].detach().to(dtype).clone().requires_grad_(True) for n in ("_scaling", "_scaling_t", "_rotation", "_rotation_r")}
    v = velocity(leaves["_scaling"], leaves["_scaling_t"], leaves["_rotation"], leaves["_rotation_r"], params["_t"], dtype)
    lr = rigid(v, torch.as_tensor(idx), torch.as_tensor(d2))
    lm = motion(v)
    (g_rigid * lr + g_motion * lm).backward()
    return float(lr), float(lm), {n: t.grad.detach() for n, t in leaves.items()}
