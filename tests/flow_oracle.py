"""PyTorch statement, on the CPU, of ``fdgs.flow.gaussian_flow`` (csrc/flow.hip), written from its definition:

    flow_i = pix(mu_i(t_1); target camera) - pix(mu_i(t_0); source camera)

* mu_i(t): with ``rot_4d`` the conditional mean ``p + Sigma[0:3,3] / Sigma[3,3] * (t - t_i)`` of the 4D Gaussian, the covariance put
  together as scene/gaussian_model.py:34-47 does (``L = R4 diag(modifier * s)``, ``Sigma = L L^T``, ``R4`` the product of the two
  isoclinic matrices of utils/general_utils.py:113-133); otherwise the plain mean.
* pix: ``h = (mu, 1) @ full_proj_transform``, ``ndc = h.xy / (h.w + 1e-7)``, ``pix = ((ndc + 1) * (W, H) - 1) / 2`` (auxiliary.h:42-45).
* a Gaussian whose view-space z ``((mu, 1) @ world_view_transform).z <= 0.2`` at either end: flow 0, and no gradient.

``raw=True``: ``scales`` / ``scales_t`` go through exp and the quaternions through F.normalize first (the model's activations);
``raw=False``: the tensors are the activated values and enter AS PASSED -- the matrices are built from the quaternions without
normalising them again, which is what "the gradient with respect to the activated values" means (for unit quaternions the value is the
same).  dtype-generic (float64: the reference of the GPU tests; float32: how far fp32 itself is from it) and differentiable.  The
timestamps are rounded to float32 first: the kernels receive them as floats.
"""
import numpy as np
import torch


def sigma4(scales4, rot, rot_r):
    """[P,4,4] Sigma = L L^T, L = R4 diag(scales4); the quaternions enter as they are."""
    a, b, c, d = rot.unbind(-1)
    p, q, r, s = rot_r.unbind(-1)
    Ml = torch.stack([a, -b, -c, -d, b, a, -d, c, c, d, a, -b, d, -c, b, a], dim=1).view(-1, 4, 4)
    Mr = torch.stack([p, q, r, s, -q, p, -s, r, -r, s, p, -q, -s, -r, q, p], dim=1).view(-1, 4, 4)
    R = (Ml @ Mr).flip(1, 2)
    L = R * scales4.unsqueeze(1)
    return L @ L.transpose(1, 2)


def velocity(scales, scales_t, rotations, rotations_r, raw, scaling_modifier=1.0):
    """[P,3]: Sigma[0:3,3] / Sigma[3,3] (the mean moves by this per unit of time)."""
    s4 = torch.cat([scales, scales_t.reshape(-1, 1)], dim=1)
    ql, qr = rotations, rotations_r
    if raw:
        s4 = torch.exp(s4)
        ql = torch.nn.functional.normalize(ql, dim=-1)
        qr = torch.nn.functional.normalize(qr, dim=-1)
    sig = sigma4(scaling_modifier * s4, ql, qr)
    return sig[:, 0:3, 3] / sig[:, 3, 3:4]


def project(mean, view, proj, W, H):
    """(pix [P,2], view-space z [P]) of world points; ``view`` / ``proj``: world_view_transform / full_proj_transform (row-vector convention)."""
    hom = torch.cat([mean, torch.ones_like(mean[:, :1])], dim=1)
    h = hom @ proj.to(mean.dtype)
    z = (hom @ view.to(mean.dtype))[:, 2]
    ndc = h[:, 0:2] / (h[:, 3:4] + 1e-7)
    wh = torch.tensor([float(W), float(H)], dtype=mean.dtype)
    return ((ndc + 1.0) * wh - 1.0) * 0.5, z


def gaussian_flow(view0, proj0, t0, view1, proj1, t1, W, H, means3D, ts, scales, scales_t, rotations, rotations_r, *, rot_4d, raw,
                  scaling_modifier=1.0, dtype=torch.float64, details=False):
    """[P,2] flow in ``dtype``; every tensor argument may require grad (convert to ``dtype`` BEFORE the call to differentiate).
    ``details``: also the two pixel positions and the validity mask."""
    cv = lambda t: None if t is None else t.to(dtype)  # noqa: E731
    means3D = cv(means3D)
    t0, t1 = float(np.float32(t0)), float(np.float32(t1))
    m0 = m1 = means3D
    if rot_4d:
        w = velocity(cv(scales), cv(scales_t), cv(rotations), cv(rotations_r), raw, scaling_modifier)
        ti = cv(ts).reshape(-1, 1)
        m0 = means3D + w * (t0 - ti)
        m1 = means3D + w * (t1 - ti)
    pix0, z0 = project(m0, view0, proj0, W, H)
    pix1, z1 = project(m1, view1, proj1, W, H)
    ok = ~(z0 <= 0.2) & ~(z1 <= 0.2)
    flow = torch.where(ok.unsqueeze(1), pix1 - pix0, torch.zeros_like(pix0))
    return (flow, pix0, pix1, ok) if details else flow


NAMES = ("means3D", "ts", "scales", "scales_t", "rotations", "rotations_r")


def flow_with_grads(view0, proj0, t0, view1, proj1, t1, W, H, params, dL_dflows, *, rot_4d, raw, scaling_modifier=1.0, dtype=torch.float64):
    """(flow, {name: gradient}) of sum(flow * dL_dflows) with respect to the six tensors of ``params`` (a dict by NAMES), in ``dtype``."""
    leaves = {n: params[n].detach().to(dtype).clone().requires_grad_(True) for n in NAMES}
    flow = gaussian_flow(view0, proj0, t0, view1, proj1, t1, W, H, *[leaves[n] for n in NAMES], rot_4d=rot_4d, raw=raw,
                         scaling_modifier=scaling_modifier, dtype=dtype)
    (flow * dL_dflows.to(dtype)).sum().backward()
    return flow.detach(), {n: (torch.zeros_like(t) if t.grad is None else t.grad.detach()) for n, t in leaves.items()}
