"""float64 torch statement of the environment-map composite (gaussian_renderer/__init__.py:165-177, scene/cameras.py:75-82):
rays, sphere intersection, texture coordinates, the bilinear zero-padded lookup written out by hand (not F.grid_sample: the host
tests compare the two), the composite and -- through autograd -- its gradients.  One deliberate difference from the reference:
z / R is clamped to [-1, 1] before the acos (csrc/envmap.hip takes the equal atan2(sqrt(x^2 + y^2), z), which cannot leave [0, pi])."""
import math

import numpy as np
import torch

F64 = torch.float64


def rays(world_view_transform, camera_center, fl_x, fl_y, cx, cy, H, W):
    """(origin [3], unit directions [H, W, 3]) of the pixel centres, as Camera.get_rays."""
    vm = torch.as_tensor(world_view_transform).to(F64).cpu()
    o = torch.as_tensor(camera_center).to(F64).cpu().reshape(3)
    j, i = torch.meshgrid(torch.arange(H, dtype=F64) + 0.5, torch.arange(W, dtype=F64) + 0.5, indexing="ij")
    one = torch.ones_like(i)
    pts = torch.stack([(i - cx) / fl_x, (j - cy) / fl_y, one, one], -1)
    c2w = torch.linalg.inv(vm.transpose(0, 1))
    d = (pts @ c2w.T)[..., :3] - o
    return o, d / torch.norm(d, dim=-1, keepdim=True)


def intersect(o, d, R=60.0):
    """The point where the ray leaves the sphere, with the reference's operator precedence."""
    od, dd, oo = (o * d).sum(-1), (d * d).sum(-1), (o * o).sum(-1)
    delta = od ** 2 - dd * (oo - R ** 2)
    t = -od + torch.sqrt(delta) / dd
    return o + d * t.unsqueeze(-1)


def texcoord(x, R=60.0):
    """(u, v) in [0, 1]: u = atan2(y, x) / 2pi + 0.5, v = acos(clamp(z / R)) / pi."""
    u = torch.atan2(x[..., 1], x[..., 0]) / (2 * math.pi) + 0.5
    v = torch.acos((x[..., 2] / R).clamp(-1.0, 1.0)) / math.pi
    return u, v


def bilinear(env, u, v):
    """grid_sample(env[None], grid = (u, v) * 2 - 1, bilinear, zeros, align_corners=False)[0], written out: [3, H, W]."""
    C, eh, ew = env.shape
    ix = ((u * 2 - 1 + 1) * ew - 1) / 2
    iy = ((v * 2 - 1 + 1) * eh - 1) / 2
    x0, y0 = torch.floor(ix), torch.floor(iy)
    out = torch.zeros((C,) + tuple(u.shape), dtype=env.dtype)
    flat = env.reshape(C, -1)
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        xk, yk = x0 + dx, y0 + dy
        w = (1 - (ix - xk).abs()) * (1 - (iy - yk).abs())
        ok = (xk >= 0) & (xk < ew) & (yk >= 0) & (yk < eh)
        idx = (yk.clamp(0, eh - 1) * ew + xk.clamp(0, ew - 1)).long()
        out = out + torch.where(ok, w, torch.zeros_like(w)) * flat[:, idx.reshape(-1)].reshape((C,) + tuple(u.shape))
    return out


def cam_rays(cam, H, W):
    return rays(cam.world_view_transform, cam.camera_center, float(cam.fl_x), float(cam.fl_y), float(cam.cx), float(cam.cy), H, W)


def lookup(cam, env, H, W, R=60.0):
    """env(ray) [3, H, W] and the flags of the pixels within 1e-4 R of the seam or 1e-3 R of the pole axis [H, W]."""
    o, d = cam_rays(cam, H, W)
    x = intersect(o, d, R)
    u, v = texcoord(x, R)
    seam = (x[..., 1].abs() < 1e-4 * R) & (x[..., 0] < 0)
    pole = torch.sqrt(x[..., 0] ** 2 + x[..., 1] ** 2) < 1e-3 * R
    return bilinear(env, u, v), seam | pole


def composite(colour, alpha, env, cam, R=60.0):
    """colour + (1 - alpha) * env(ray), float64, differentiable in colour, alpha and env.  Returns (image, flags)."""
    H, W = colour.shape[-2:]
    e, flags = lookup(cam, env, H, W, R)
    return colour + (1 - alpha) * e, flags


def composite_grads(colour, alpha, env, cam, g, R=60.0):
    """(d <g, composite> / d alpha, d / d env) in float64 through autograd."""
    a = alpha.detach().to(F64).cpu().requires_grad_(True)
    e = env.detach().to(F64).cpu().requires_grad_(True)
    out, _ = composite(colour.detach().to(F64).cpu(), a, e, cam, R)
    (out * g.detach().to(F64).cpu()).sum().backward()
    return a.grad, e.grad


class PlainCamera:
    """What the composite reads of a camera: world_view_transform, camera_center, fl_x, fl_y, cx, cy."""

    def __init__(self, world_view_transform, camera_center, fl_x, fl_y, cx, cy):
        self.world_view_transform, self.camera_center = world_view_transform, camera_center
        self.fl_x, self.fl_y, self.cx, self.cy = fl_x, fl_y, cx, cy

    def to(self, dev):
        return PlainCamera(self.world_view_transform.to(dev), self.camera_center.to(dev), self.fl_x, self.fl_y, self.cx, self.cy)


def camera(pose, W, H):
    """A PlainCamera of fdgs.synth.camera_for(pose) with its pinhole intrinsics (centre-shift principal point where the pose has one)."""
    from fdgs import synth
    kw = dict(synth.POSES[pose] if isinstance(pose, str) else pose)
    off = kw.pop("principal_off", None)
    c = synth.camera_for(pose, W, H)
    focal = W / (2.0 * c["tanfovx"])
    cx, cy = (0.5 * W, 0.5 * H) if off is None else (0.5 * W + off[0], 0.5 * H + off[1])
    return PlainCamera(c["world_view_transform"], c["camera_center"], focal, focal, cx, cy)


# the poses of the tests: "axis" looks at the +z pole and crosses the atan2 seam; the DyNeRF-like rigs; one looking along the
# equator (+y); one with the seam (direction -x) in mid-image
POSES = {
    "axis": "axis",
    "rig1": "rig1",
    "rig2": "rig2",
    "equator": dict(pitch=-math.pi / 2, shift=(0.3, -0.2, 4.0)),
    "seam": dict(yaw=-math.pi / 2, pitch=-math.pi / 2, shift=(0.2, 0.1, 4.0), principal_off=(7.5, -3.25)),
}


# ------------------------------------------------------------------------------------------------------------------------------------
# Per element: taps, tile boxes, error bars, a float32 emulation and its mutants (numpy; tests/envmap_cases.py,
# tests/test_envmap_cases_host.py, tests/test_gpu_envmap_edges.py).  Nothing above changes meaning.
# ------------------------------------------------------------------------------------------------------------------------------------
U32 = 2.0 ** -24          # unit roundoff of float32 (round to nearest)
TILE = 16                 # ENV_TILE of csrc/envmap.hip
ENV_WIN = 3072            # ENV_WIN of csrc/envmap.hip: the largest LDS window, in texels
CORNERS = ((0, 0), (1, 0), (0, 1), (1, 1))     # (dx, dy) of corner k: the kernel's order (k & 1, k >> 1)
MUTANTS = ("wrap_seam", "clamp_pole", "align_corners", "swap_w12", "round_corner", "drop_clamped")   # (a) .. (f) of emulate_f32


def texcoord_atan2(x, R=60.0):
    """(u, v) with v = atan2(sqrt(x^2 + y^2), z) / pi: the kernel's form.  ``texcoord``'s acos(z / R) has derivative 1 / sin(theta) in
    z / R, whose own rounding (1e-16) then costs ~1e-8 of v next to the pole even in float64; this one is accurate everywhere."""
    u = torch.atan2(x[..., 1], x[..., 0]) / (2 * math.pi) + 0.5
    v = torch.atan2(torch.sqrt(x[..., 0] ** 2 + x[..., 1] ** 2), x[..., 2]) / math.pi
    return u, v


def _f32(x):
    return float(np.float32(float(x)))


def abi_camera(cam):
    """The camera as the C ABI receives it: matrix and centre as float32 tensors, the four intrinsics rounded to float32."""
    return PlainCamera(torch.as_tensor(cam.world_view_transform).detach().float().cpu(), torch.as_tensor(cam.camera_center).detach().float().cpu(),
                       _f32(cam.fl_x), _f32(cam.fl_y), _f32(cam.cx), _f32(cam.cy))


def exit_points(cam, H, W, R=60.0):
    """[H, W, 3] float64 numpy: where the pixel centres' rays leave the sphere (linalg.inv formulation, float32 ABI inputs)."""
    o, d = cam_rays(abi_camera(cam), H, W)
    return intersect(o, d, R).numpy()


def texel_coords(cam, H, W, eh, ew, R=60.0):
    """(ix, iy, X): grid_sample's unnormalised coordinates (align_corners = False) of the atan2 form, and the exit points."""
    X = exit_points(cam, H, W, R)
    u, v = texcoord_atan2(torch.from_numpy(X), R)
    u, v = u.numpy(), v.numpy()
    return ((u * 2 - 1 + 1) * ew - 1) / 2, ((v * 2 - 1 + 1) * eh - 1) / 2, X


def _det3(m):
    return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
            + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))


def kernel_texel_coords(cam, H, W, eh, ew, R=60.0):
    """(ix, iy) by the kernel's own float64 formulation (env_setup / env_tap of csrc/envmap.hip): the inverse of the view matrix by
    cofactors, the ray as a * c0 + b * c1 + (c2 + c3) - o, ix = u * ew - 0.5.  The largest difference from texel_coords over the
    cases is what DELTA of tests/envmap_cases.py stands on."""
    cam = abi_camera(cam)
    a = cam.world_view_transform.double().numpy()
    o = cam.camera_center.double().numpy().reshape(3)
    adj = np.empty((4, 4))
    for r in range(4):
        for c in range(4):
            minor = [[a[i][j] for j in range(4) if j != r] for i in range(4) if i != c]      # adj[r][c] = cofactor[c][r]
            adj[r, c] = (-1.0) ** (r + c) * _det3(minor)
    det = sum(a[0][k] * adj[k, 0] for k in range(4))
    inv = adj / det
    c2w = inv.T                                                                                   # inv(V^T)
    jj, ii = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    pa, pb = (ii + 0.5 - cam.cx) / cam.fl_x, (jj + 0.5 - cam.cy) / cam.fl_y
    d = np.stack([(pa * c2w[r, 0] + pb * c2w[r, 1] + (c2w[r, 2] + c2w[r, 3])) - o[r] for r in range(3)], -1)
    d = d / np.sqrt((d * d).sum(-1, keepdims=True))
    od, dd, oo = (d * o).sum(-1), (d * d).sum(-1), (o * o).sum()
    t = -od + np.sqrt(np.maximum(od * od - dd * (oo - R * R), 0.0)) / dd
    X = o + d * t[..., None]
    u = np.arctan2(X[..., 1], X[..., 0]) / (2.0 * math.pi) + 0.5
    v = np.arctan2(np.sqrt(X[..., 0] ** 2 + X[..., 1] ** 2), X[..., 2]) / math.pi
    return u * ew - 0.5, v * eh - 0.5


def taps(cam, H, W, eh, ew, R=60.0, mutant=None):
    """The bilinear tap of every pixel, float64: ``ix, iy`` [H, W], the corner ``x0, y0`` [H, W] (int64), the weights ``w`` [4, H, W]
    of the corners in the kernel's order, ``inmap`` [4, H, W] (the corner lies in the map; the others are zero padding), ``cx, cy``
    [4, H, W] (the texel a corner reads or writes where inmap) and the exit points ``X`` [H, W, 3].
    ``mutant``: one of MUTANTS (a) .. (e), a defective tap for emulate_f32 (never the reference)."""
    ix, iy, X = texel_coords(cam, H, W, eh, ew, R)
    if mutant == "align_corners":
        ix, iy = (ix + 0.5) / ew * (ew - 1), (iy + 0.5) / eh * (eh - 1)
    x0, y0 = (np.rint(ix), np.rint(iy)) if mutant == "round_corner" else (np.floor(ix), np.floor(iy))
    ax, ay = ix - x0, iy - y0
    w = np.stack([(1 - ax) * (1 - ay), ax * (1 - ay), (1 - ax) * ay, ax * ay])
    if mutant == "swap_w12":
        w = w[[0, 2, 1, 3]]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    cx = np.stack([x0 + dx for dx, _ in CORNERS])
    cy = np.stack([y0 + dy for _, dy in CORNERS])
    okx, oky = (cx >= 0) & (cx < ew), (cy >= 0) & (cy < eh)
    if mutant == "wrap_seam":
        cx, okx = cx % ew, np.ones_like(okx)
    if mutant == "clamp_pole":
        cy, oky = np.clip(cy, 0, eh - 1), np.ones_like(oky)
    return {"H": H, "W": W, "eh": eh, "ew": ew, "ix": ix, "iy": iy, "x0": x0, "y0": y0, "w": w, "inmap": okx & oky,
            "cx": np.clip(cx, 0, ew - 1), "cy": np.clip(cy, 0, eh - 1), "X": X}


def exempt(t, delta, R=60.0):
    """[H, W] bool: the ray leaves the sphere on the seam itself (X < 0, |Y| < delta R), where u jumps between 0 and 1."""
    return (t["X"][..., 0] < 0) & (np.abs(t["X"][..., 1]) < delta * R)


def tile_boxes(t):
    """Per 16 x 16 pixel tile, tiles in row-major order (blockIdx.y, blockIdx.x): ``box`` [n, 4] = x min, x max, y min, y max of
    the texel window (inclusive; -1 where no pixel contributes), ``area`` [n] = ww * wh and ``path`` (list of 'none' / 'window' /
    'direct') by the kernel's rule: each pixel's corner span is clamped into the map (max(x0, 0) .. min(x0 + 1, ew - 1), likewise
    y), a pixel whose clamped span is empty contributes nothing, and a window beyond ENV_WIN texels takes direct atomics.
    Also ``slices``: the tile's (row slice, column slice) of the image."""
    H, W, eh, ew = t["H"], t["W"], t["eh"], t["ew"]
    xs, xe = np.maximum(t["x0"], 0), np.minimum(t["x0"] + 1, ew - 1)
    ys, ye = np.maximum(t["y0"], 0), np.minimum(t["y0"] + 1, eh - 1)
    ok = (xs <= xe) & (ys <= ye)
    box, area, path, slices = [], [], [], []
    for ty in range(0, H, TILE):
        for tx in range(0, W, TILE):
            sl = (slice(ty, min(ty + TILE, H)), slice(tx, min(tx + TILE, W)))
            m = ok[sl]
            slices.append(sl)
            if not m.any():
                box.append((-1, -1, -1, -1)); area.append(0); path.append("none")
                continue
            b = (int(xs[sl][m].min()), int(xe[sl][m].max()), int(ys[sl][m].min()), int(ye[sl][m].max()))
            a = (b[1] - b[0] + 1) * (b[3] - b[2] + 1)
            box.append(b); area.append(a); path.append("direct" if a > ENV_WIN else "window")
    return {"box": np.array(box, np.int64), "area": np.array(area, np.int64), "path": path, "slices": slices}


def _scatter_index(t):
    """(flat texel index [4, H, W], inmap [4, H, W])."""
    return t["cy"] * t["ew"] + t["cx"], t["inmap"]


def reference(t, colour, T, env, g, prior_alpha=None, prior_env=None):
    """float64: (colour + T env(ray) [3, H, W], d / d alpha [H, W], d / d env [3, eh, ew]) from the taps, written out (no autograd;
    the host tests hold it to composite / composite_grads).  ``prior_*``: what accumulate adds to."""
    colour, T, env, g = (np.asarray(a, np.float64) for a in (colour, T, env, g))
    H, W, eh, ew = t["H"], t["W"], t["eh"], t["ew"]
    T = T.reshape(H, W)
    idx, ok = _scatter_index(t)
    flat = env.reshape(3, -1)
    e = np.zeros((3, H, W))
    ge = np.zeros((3, eh * ew)) if prior_env is None else np.asarray(prior_env, np.float64).reshape(3, -1).copy()
    for k in range(4):
        wk = np.where(ok[k], t["w"][k], 0.0)
        e += wk * flat[:, idx[k]]
        for c in range(3):
            np.add.at(ge[c], idx[k][ok[k]], (g[c] * T * wk)[ok[k]])
    ga = -(g * e).sum(0)
    if prior_alpha is not None:
        ga = ga + np.asarray(prior_alpha, np.float64).reshape(H, W)
    return colour + T * e, ga, ge.reshape(3, eh, ew)


def abs_scatter(t, T, g, delta):
    """Per texel: ``n`` [eh, ew] contributions (in-map corners of all pixels), ``A`` [3, eh, ew] = sum |g_c T w_k| and ``B``
    [3, eh, ew] = sum |g_c T| over the pixels whose tap touches the texel when ix or iy moves by +-delta."""
    H, W, eh, ew = t["H"], t["W"], t["eh"], t["ew"]
    T, g = np.asarray(T, np.float64).reshape(H, W), np.asarray(g, np.float64)
    idx, ok = _scatter_index(t)
    n = np.zeros(eh * ew, np.int64)
    A, B = np.zeros((3, eh * ew)), np.zeros((3, eh * ew))
    gT = np.abs(g * T)
    for k in range(4):
        np.add.at(n, idx[k][ok[k]], 1)
        for c in range(3):
            np.add.at(A[c], idx[k][ok[k]], (gT[c] * np.abs(t["w"][k]))[ok[k]])
    xlo, xhi = np.floor(t["ix"] - delta).astype(np.int64), np.floor(t["ix"] + delta).astype(np.int64) + 1
    ylo, yhi = np.floor(t["iy"] - delta).astype(np.int64), np.floor(t["iy"] + delta).astype(np.int64) + 1
    for dy in range(3):
        for dx in range(3):
            x, y = xlo + dx, ylo + dy
            m = (x <= xhi) & (y <= yhi) & (x >= 0) & (x < ew) & (y >= 0) & (y < eh)
            for c in range(3):
                np.add.at(B[c], (y * ew + x)[m], gT[c][m])
    return n.reshape(eh, ew), A.reshape(3, eh, ew), B.reshape(3, eh, ew)


def bars(t, colour, T, env, g, delta, prior_env=None):
    """The per-element bars (u = 2^-24; DESIGN.md, the environment-map row of section 1):
      forward        8 u (|colour| + T E_c) + 4 delta T max_k |env_ck|           E_c = sum_k w_k |env_ck| over the in-map corners
      d / d alpha    8 u sum_c |g_c| E_c + 4 delta sum_c |g_c| max_k |env_ck|
      d / d env      (n + 2) u (A + |prior|) + 2 delta B
    8 u: one weight rounding, one product, three additions, then the T multiply and the final add (forward) or the product and two
    additions of the dot product (alpha).  (n + 2) u: three roundings per term, any summation tree over n terms within (n - 1) u.
    Returns (bar_out [3, H, W], bar_alpha [H, W], bar_env [3, eh, ew], n [eh, ew])."""
    colour, T, env, g = (np.asarray(a, np.float64) for a in (colour, T, env, g))
    H, W = t["H"], t["W"]
    T = np.abs(T.reshape(H, W))
    idx, ok = _scatter_index(t)
    flat = np.abs(env.reshape(3, -1))
    E, M = np.zeros((3, H, W)), np.zeros((3, H, W))
    for k in range(4):
        ek = np.where(ok[k], flat[:, idx[k]], 0.0)
        E += np.abs(t["w"][k]) * ek
        M = np.maximum(M, ek)
    bar_out = 8 * U32 * (np.abs(colour) + T * E) + 4 * delta * T * M
    bar_alpha = 8 * U32 * (np.abs(g) * E).sum(0) + 4 * delta * (np.abs(g) * M).sum(0)
    n, A, B = abs_scatter(t, T, g, delta)
    prior = 0.0 if prior_env is None else np.abs(np.asarray(prior_env, np.float64))
    bar_env = (n + 2) * U32 * (A + prior) + 2 * delta * B
    return bar_out, bar_alpha, bar_env, n


def emulate_f32(t, colour, T, env, g, order="row", prior_alpha=None, prior_env=None, mutant=None):
    """The kernels in numpy float32: coordinates and weights in float64 (``t``: taps, or a mutant's taps), the weights rounded to
    float32, every later operation in float32 in the kernel's order (corners 0..3; products rounded before they are added: no FMA).
    The scatter is summed in one of two orders: ``row`` (pixels row-major, into the map directly) or ``tile`` (tile by tile: a
    window tile sums its terms in a zeroed window first and adds each non-zero window texel to the map once; a direct tile adds its
    terms to the map) -- the kernel's atomics arrive in neither order, and every order is within the same bar.
    ``mutant`` = 'drop_clamped' ((f): a pixel any of whose corners was clamped into the box scatters nothing); the mutants (a) .. (e)
    are taps(mutant=).  Returns float32 (out [3, H, W], d / d alpha [H, W], d / d env [3, eh, ew])."""
    f = np.float32
    H, W, eh, ew = t["H"], t["W"], t["eh"], t["ew"]
    colour, env, g = (np.asarray(a, f) for a in (colour, env, g))
    T = np.asarray(T, f).reshape(H, W)
    idx, ok = _scatter_index(t)
    w = t["w"].astype(f)
    flat = env.reshape(3, -1)
    e = np.zeros((3, H, W), f)
    for k in range(4):
        e = e + np.where(ok[k], w[k] * flat[:, idx[k]], f(0))
    out = colour + T * e
    ga = -((g[0] * e[0] + g[1] * e[1]) + g[2] * e[2])
    if prior_alpha is not None:
        ga = np.asarray(prior_alpha, f).reshape(H, W) + ga
    gw = g * T
    terms = np.stack([gw * w[k] for k in range(4)])                       # [4, 3, H, W]
    live = ok.copy()
    if mutant == "drop_clamped":
        live &= ok.all(0)
    ge = np.zeros((3, eh * ew), f) if prior_env is None else np.asarray(prior_env, f).reshape(3, -1).copy()

    def add(dst, sl):
        """dst[c][texel] += term, pixels of the slice row-major, corners 0..3 within a pixel."""
        i = np.moveaxis(idx[(slice(None),) + sl], 0, -1).reshape(-1)
        m = np.moveaxis(live[(slice(None),) + sl], 0, -1).reshape(-1)
        for c in range(3):
            v = np.moveaxis(terms[(slice(None), c) + sl], 0, -1).reshape(-1)
            np.add.at(dst[c], i[m], v[m])

    if order == "row":
        add(ge, (slice(0, H), slice(0, W)))
    else:
        tb = tile_boxes(t)
        for sl, path in zip(tb["slices"], tb["path"]):
            if path == "direct":
                add(ge, sl)
            elif path == "window":
                win = np.zeros((3, eh * ew), f)
                add(win, sl)
                ge = np.where(win != 0, ge + win, ge)
    return out, ga, ge.reshape(3, eh, ew)


def mutants(cam, H, W, eh, ew, colour, T, env, g, R=60.0, names=MUTANTS):
    """{name: emulate_f32's (out, d / d alpha, d / d env)} with one defect each: (a) 'wrap_seam' the seam wraps, (b) 'clamp_pole' the
    pole rows clamp instead of zero-padding, (c) 'align_corners' the align_corners = True unnormalisation, (d) 'swap_w12' the weights
    of corners 1 and 2 swapped, (e) 'round_corner' the tap corner by round instead of floor, (f) 'drop_clamped' the scatter drops
    the pixels a corner of which was clamped into the box.  The bars and cases must catch every one of them."""
    res = {}
    for name in names:
        t = taps(cam, H, W, eh, ew, R, mutant=None if name == "drop_clamped" else name)
        res[name] = emulate_f32(t, colour, T, env, g, "row", mutant=name)
    return res
