"""PyTorch statement of fdgs.depth (csrc/depth_loss.hip), written from its definition, with gradients by autograd.

Evaluated in float64 on the CPU it is what the kernels are compared with; the same code in float32 is the error yardstick (what the
plain tensor formulation of the same term costs in accuracy), and on GPU tensors it is the float32 torch formulation the end-to-end
test and the example's --bench put next to the kernels.

    z = depth / alpha where alpha >= alpha_min (alpha None: z = depth); valid: that test, mask None or > 0, and for the losses a
    finite prior > 0.  pearson: 1 - rho over the valid pixels; ssi: sum |s z + b - p| / n with the least-squares (s, b) DETACHED;
    degenerate (n < 2, or a variance of z or p at or below 1e-12 max(1, mean^2)): 1 / 0 with a zero gradient.
    normals: P = ((u+.5-cx)/fl_x z, (v+.5-cy)/fl_y z, z), a = P(u+1,v) - P(u-1,v), b = P(u,v+1) - P(u,v-1), n = (b x a)/|b x a|,
    valid where the five pixels are inside and valid and |b x a|^2 > 1e-20, else n = 0.
"""
import torch

LEN2_MIN = 1e-20


def depth_z(depth, alpha, mask, alpha_min, dtype):
    """(z [H, W] in ``dtype``, ok [H, W] bool); z is finite everywhere (the division is by 1 where the alpha test fails)."""
    D = depth.reshape(depth.shape[-2:]).to(dtype)
    if alpha is None:
        ok = torch.ones(D.shape, dtype=torch.bool, device=D.device)
        z = D
    else:
        A = alpha.reshape(D.shape).to(dtype)
        ok = A.detach() >= alpha_min
        z = D / torch.where(ok, A, torch.ones_like(A))
    if mask is not None:
        ok = ok & (mask.reshape(D.shape) > 0)
    return z, ok


def prior_ok(prior):
    p = prior.reshape(prior.shape[-2:])
    return torch.isfinite(p) & (p > 0)


def moments(z, p, v):
    """n, means, population variances and covariance over the pixels where ``v``."""
    n = v.sum()
    zm, pm = (z * v).sum() / n, (p * v).sum() / n
    dz, dp = (z - zm) * v, (p - pm) * v
    return n, zm, pm, (dz * dz).sum() / n, (dp * dp).sum() / n, (dz * dp).sum() / n


def is_degenerate(n, zm, pm, vz, vp):
    n, zm, pm, vz, vp = (float(t.detach()) for t in (n, zm, pm, vz, vp))
    if n < 2:
        return True
    return not (vz > 1e-12 * max(1.0, zm ** 2)) or not (vp > 1e-12 * max(1.0, pm ** 2))


def depth_loss(depth, alpha, prior, mask=None, mode="pearson", alpha_min=0.5, dtype=torch.float64, align=None):
    """(loss, stats): stats = (n, rho, 0) for pearson, (n, s, b) for ssi, Python floats.  ``align`` = (s, b): use this alignment
    instead of the fit (ssi; for finite differences of the detached-alignment loss)."""
    z, ok = depth_z(depth, alpha, mask, alpha_min, dtype)
    pv = prior_ok(prior)
    ok = ok & pv
    p = torch.where(pv, prior.reshape(z.shape), torch.zeros_like(prior.reshape(z.shape))).to(dtype)
    v = ok.to(dtype)
    zero = (z * 0.0).sum()                    # keeps the graph: a degenerate case still has a (zero) gradient
    if float(v.sum()) < 1:
        return zero + (1.0 if mode == "pearson" else 0.0), (0.0, 0.0, 0.0)
    z = torch.where(ok, z, torch.zeros_like(z))
    n, zm, pm, vz, vp, cov = moments(z, p, v)
    if is_degenerate(n, zm, pm, vz, vp):
        return zero + (1.0 if mode == "pearson" else 0.0), (float(n), 0.0, 0.0)
    if mode == "pearson":
        rho = cov / torch.sqrt(vz * vp)
        return 1.0 - rho, (float(n), float(rho.detach()), 0.0)
    if align is None:
        s = (cov / vz).detach()
        b = (pm - s * zm).detach()
    else:
        s, b = align
    r = (s * z + b - p) * v
    return r.abs().sum() / n, (float(n), float(s), float(b))


def normals(depth, alpha, intrinsics, mask=None, alpha_min=0.5, viewmatrix=None, dtype=torch.float64):
    """(normals [3, H, W] in ``dtype``, valid [1, H, W] bool, len2 [H, W]: |b x a|^2 where the five pixels are valid, else 0)."""
    z, ok = depth_z(depth, alpha, mask, alpha_min, dtype)
    H, W = z.shape
    dev = z.device
    out = torch.zeros((3, H, W), dtype=dtype, device=dev)
    valid = torch.zeros((1, H, W), dtype=torch.bool, device=dev)
    len2_full = torch.zeros((H, W), dtype=dtype, device=dev)
    if H < 3 or W < 3:
        return out + (z * 0.0).sum(), valid, len2_full
    fl_x, fl_y, cx, cy = intrinsics
    xs = (torch.arange(W, dtype=dtype, device=dev) + 0.5 - cx) / fl_x
    ys = (torch.arange(H, dtype=dtype, device=dev) + 0.5 - cy) / fl_y
    P = torch.stack([xs[None, :] * z, ys[:, None] * z, z])
    a = P[:, 1:-1, 2:] - P[:, 1:-1, :-2]
    b = P[:, 2:, 1:-1] - P[:, :-2, 1:-1]
    N = torch.stack([b[1] * a[2] - b[2] * a[1], b[2] * a[0] - b[0] * a[2], b[0] * a[1] - b[1] * a[0]])
    len2 = (N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]
    five = ok[1:-1, 1:-1] & ok[1:-1, 2:] & ok[1:-1, :-2] & ok[2:, 1:-1] & ok[:-2, 1:-1]
    v = five & (len2.detach() > LEN2_MIN)
    n = torch.where(v[None], N / torch.sqrt(torch.where(v, len2, torch.ones_like(len2)))[None], torch.zeros_like(N))
    if viewmatrix is not None:
        R = viewmatrix.to(dev, dtype)[:3, :3]       # view -> world of the transposed world-to-view matrix
        n = torch.stack([(R[i, 0] * n[0] + R[i, 1] * n[1]) + R[i, 2] * n[2] for i in range(3)])
    out = torch.nn.functional.pad(n, (1, 1, 1, 1))
    valid[0, 1:-1, 1:-1] = v
    len2_full[1:-1, 1:-1] = torch.where(five, len2.detach(), torch.zeros_like(len2))
    return out, valid, len2_full


def normal_loss(n, valid, prior_normals):
    v = valid.to(n.dtype)
    return ((1.0 - (n * prior_normals.to(n.dtype)).sum(-3, keepdim=True)) * v).sum() / v.sum().clamp(min=1.0)


# ---- inputs shared by the host and the GPU tests: float32 CPU tensors, seeded ----
def smooth_depth(H, W, seed, noise=0.02):
    """A smooth surface between 2 and 6 plus noise, like a rendered depth."""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(1, 1, H // 8 + 2, W // 8 + 2, generator=g)
    up = torch.nn.functional.interpolate(base, size=(H, W), mode="bilinear", align_corners=True)[0]
    return 2.0 + 4.0 * up + noise * torch.randn(1, H, W, generator=g)


def make_inputs(kind, H, W, seed=3):
    """dict(depth, alpha, prior, mask) of one input class (tests/test_gpu_depth.py lists them)."""
    g = torch.Generator().manual_seed(1000 + seed)
    z = smooth_depth(H, W, seed)
    alpha = 0.6 + 0.4 * torch.rand(1, H, W, generator=g)
    prior = (0.7 * smooth_depth(H, W, seed + 1, noise=0.05) + 0.3 * z + 0.5).clamp(min=0.1)
    mask = None
    if kind == "smooth":
        pass
    elif kind == "affine":                     # rho = 1, zero ssi residual
        prior = (1.7 * (z.double()) + 0.4).float()
    elif kind == "constant":                   # degenerate variance of z: depth = 3 alpha exactly
        z = torch.full((1, H, W), 3.0)
        alpha = torch.full((1, H, W), 0.75)
    elif kind == "all_invalid":
        mask = torch.zeros(1, H, W)
    elif kind == "alpha_straddle":             # alpha on both sides of alpha_min = 0.5, some exactly at it, some 0
        alpha = 0.35 + 0.6 * torch.rand(1, H, W, generator=g)
        alpha.view(-1)[::7] = 0.5
        alpha.view(-1)[3::11] = 0.0
        if H * W >= 64:
            mask = (torch.rand(1, H, W, generator=g) > 0.1).float()
    elif kind == "alpha_none":
        alpha = None
    elif kind == "bad_prior":                  # 0, inf, nan and negative priors: excluded
        flat = prior.view(-1)
        flat[0::5] = 0.0
        flat[1::9] = float("inf")
        flat[2::13] = float("nan")
        flat[4::17] = -1.0
    else:
        raise KeyError(kind)
    depth = z if alpha is None else (z.double() * alpha.double()).float()
    if kind == "constant":
        depth = torch.full((1, H, W), 2.25)    # 3 * 0.75 exactly
    if kind == "affine":                       # of the z the kernels see, rounded to float32 once
        prior = (1.7 * (depth.double() / alpha.double()) + 0.4).float()
    return {"depth": depth, "alpha": alpha, "prior": prior, "mask": mask}


KINDS = ("smooth", "affine", "constant", "all_invalid", "alpha_straddle", "alpha_none", "bad_prior")


def intrinsics_for(H, W):
    """An off-centre pinhole for an H x W image."""
    return (0.9 * W + 3.0, 0.85 * W + 3.0, 0.5 * W + 1.25, 0.5 * H - 0.75)
