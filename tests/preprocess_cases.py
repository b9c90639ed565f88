"""Cases of the forward-preprocess tests (tests/test_preprocess_oracle_host.py on the CPU, tests/test_gpu_preprocess_edges.py on the
GPU): seeded, tiny, built by construction.  A case is a scene, its views (pose, timestamp), and the POPULATIONS it exists for; both
tests count them from the float64 oracle's evaluation of the very inputs the kernels get (``populations``) and fail when one is short.

Directed populations (``pops``; ``n`` Gaussians each, from the end of the index range; "lo" / "hi" = the two sides of the threshold,
reached by bisecting ONE fp32 input down to two adjacent fp32 values and stepping 0, 1, 3, ... inputs away from the boundary):
  near        view-space z around the 0.2 near cull                      (means3D.z bisected)
  marg        temporal marginal around 0.05                              (ts bisected; dim 4)
  opa         opacity around 1/255                                       (opacity bisected; ts == timestamp, so the marginal is 1),
              and "faint": 0.002 / 0.006, clearly either side
  clampx/y    view-space x/z (y/z) around 1.3 tan_fov, and far beyond    (means3D.x / .y bisected; a large splat so it reaches the image)
  edge        pix.x / pix.y an integer N and radius 8 with N - 8 or N + 8 + 15 a multiple of 16: the rectangle quotient is an integer
  outside     means up to half an image outside the frame: rectangles clamp to grid_x / grid_y and to 0
  zero_rect   small splats far outside: a rectangle of zero area (culled after the radius)
  needle      1:60 on screen, random orientation
  tiny_st     scales_t of 1e-4 with |dt| from 0 to the duration (rot_4d: c12 / cov_t * dt is huge where it survives)
  det0        a splat thousands of pixels long at 45 degrees: fp32 det = cx cz - cy cy cancels to (next to) nothing
  bits        all three colour channels clamped / exactly one
  dead_wave   Gaussians 0..63 behind the near plane: a wave with every Gaussian culled, its SH rows never fetched
P = 65 leaves 63 lanes of the last wave beyond P; P in {1, 63, 64, 65, 257, 1000}.
"""
import math
import os
import sys
from typing import NamedTuple

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import chain_oracle as co  # noqa: E402
import preprocess_oracle as po  # noqa: E402
from fdgs import synth  # noqa: E402

MARGIN = 4.0        # loss_cases.MARGIN's reason: another correct fp32 association may round four times worse than the reference's
FLAG_CAP = 0.005    # blend_cases.FLAG_CAP: at most 0.5 % of a case's Gaussians may sit on a decision's edge without having been put there
# K_tensor = MARGIN * r_port: r_port = the worst |port32 - f64| / (4 ulp32 of |f64_e| + sens_e) the fp32 port
# shows on that tensor over every case and view, measured by tests/test_preprocess_oracle_host.py::test_port_pinned_and_K, which fails
# when a constant drifts from 4 * r_port.  Nothing here comes from the kernels under test.
K = {"out_means3D": 1.70, "cov3D": 3.86, "pix": 2.14, "conic": 235.0, "opacity": 1.42, "depth": 0.907, "rgb": 5.58}
# (conic: a needle seen end-on -- the triple product T^T Vrk T of the EWA projection sums products that cancel, beyond the two
# cancellations preprocess_oracle.sensitivity models; r_port records it, BASELINE.md has the element)
K_TOLERANCE = 0.10
DURATION = 4.0
TIMESTAMP = 2.0


class Case(NamedTuple):
    name: str
    P: int
    dim: int
    rot_4d: bool
    D: int
    D_t: int
    M: int                     # 0: colors_precomp
    pops: tuple = ()
    raw: bool = False
    mod: float = 1.0
    pv: float = -1.0
    force_sh_3d: bool = False
    precomp_cov: bool = False
    poses: tuple = ("rig0",)   # one view per pose; view v at TIMESTAMP + 0.11 v
    W: int = 64
    H: int = 48
    sh_off: int = 0            # floats the SH tensor is moved off its 16-byte alignment on the GPU (scalar staging path)
    seed: int = 0


GEO = ("near", "clampx", "clampy", "edge", "outside", "zero_rect", "needle")
CASES = [
    # --- model and SH modes ------------------------------------------------------------------------------------------------------
    Case("c3d_d0_p1", 1, 3, False, 0, 0, 1, poses=("axis",), W=33, H=17),                                   # (0,0,1); one Gaussian
    Case("c3d_d1_mod07", 63, 3, False, 1, 0, 4, ("near", "opa"), mod=0.7, poses=("rig1",), W=33, H=17),      # (1,0,4); scale_modifier
    Case("c3d_d2_raw", 257, 3, False, 2, 0, 9, GEO + ("opa", "bits", "det0"), raw=True),                     # (2,0,9): 27-float rows; raw
    Case("c3d_d3", 1000, 3, False, 3, 0, 16, GEO + ("opa", "bits", "det0", "dead_wave"), poses=("rig3", "axis")),
    Case("dim4_d3t1", 65, 4, False, 3, 1, 32, ("marg", "near"), poses=("rig2",), W=33, H=17),               # centre-shift projection
    Case("dim4_d3t2_raw_pv", 64, 4, False, 3, 2, 48, ("marg", "opa"), raw=True, pv=0.3),                     # 1-D marginal, prefilter
    Case("rot4d_d3t2", 257, 4, True, 3, 2, 48, GEO + ("marg", "opa", "bits", "tiny_st"), poses=("slant", "rig0", "rig2")),
    Case("rot4d_raw_pv_mod", 1000, 4, True, 3, 2, 48, GEO + ("marg", "opa", "bits", "tiny_st", "dead_wave"), raw=True, mod=0.7, pv=0.3),
    Case("rot4d_alloc48_d10", 65, 4, True, 1, 0, 48, ("marg",), seed=3),                                     # 48 allocated, (1,0) active
    Case("rot4d_sh3d", 257, 4, True, 3, 0, 16, ("marg", "bits", "dead_wave"), force_sh_3d=True, poses=("rig1",)),
    Case("rot4d_d2m9", 63, 4, True, 2, 0, 9, ("marg", "bits"), W=33, H=17),                                  # 4D path without time blocks
    Case("sh_misaligned", 65, 4, True, 3, 2, 48, ("bits",), sh_off=1, seed=5),                                # scalar staging of full rows
    Case("precomp_cov", 257, 3, False, 1, 0, 4, ("near", "clampx", "clampy", "outside", "zero_rect"), precomp_cov=True),
    Case("precomp_col", 63, 4, True, 0, 0, 0, ("marg", "near"), raw=True, W=33, H=17),                       # colors_precomp: no SH
]
BY_NAME = {c.name: c for c in CASES}
REACH_CASES = ("c3d_d3", "rot4d_d3t2")            # needles and faint opacities: the reachable_rect check
TIED_CASES = ("c3d_d2_raw", "rot4d_d3t2", "rot4d_sh3d", "sh_misaligned", "rot4d_alloc48_d10")


def _world(cam, xv):
    wv = cam["world_view_transform"].numpy().astype(np.float64)
    return (xv - wv[3, :3]) @ np.linalg.inv(wv[:3, :3])


def _unit(q):
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _step(x, k):
    """x moved k fp32 values (k < 0: down)."""
    x = np.asarray(x, np.float32).copy()
    for _ in range(abs(int(k))):
        x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf))
    return x


def bisect(q, lo, hi):
    """``q``: fp32 array -> float64 array, of one sign at ``lo`` and the other at ``hi``, element by element.  -> (a, b): adjacent fp32
    values with q(a) <= 0 < q(b) (a may lie above b)."""
    lo, hi = np.asarray(lo, np.float32).copy(), np.asarray(hi, np.float32).copy()
    ql, qh = q(lo), q(hi)
    assert ((ql <= 0) != (qh <= 0)).all(), "bisect: no sign change (%r, %r)" % (ql, qh)
    swap = ql > 0
    lo, hi = np.where(swap, hi, lo), np.where(swap, lo, hi)        # now q(lo) <= 0 < q(hi)
    for _ in range(80):
        mid = ((lo.astype(np.float64) + hi.astype(np.float64)) * 0.5).astype(np.float32)
        done = (mid == lo) | (mid == hi)
        if done.all():
            break
        neg = q(mid) <= 0
        lo, hi = np.where(neg & ~done, mid, lo), np.where(~neg & ~done, mid, hi)
    return lo, hi


def _sides(a, b, n):
    """n values around the boundary between a (q <= 0) and b (q > 0): alternately 0, 0, 1, 1, 3, 3, ... fp32 steps beyond it."""
    out = np.empty(n, np.float32)
    up = np.where(b > a, 1, -1)
    for i in range(n):
        k = (0, 1, 3, 40)[min(i // 2, 3)]
        out[i] = _step(b[i], k * up[i]) if i % 2 else _step(a[i], -k * up[i])
    return out


def build(case):
    """-> dict(case, scene: scene dict of CPU tensors of view 0, views: per-view overrides (camera tensors, timestamp), planted: bool [P]
    -- the Gaussians put on a decision's edge on purpose)."""
    c = case
    P = c.P
    rng = np.random.default_rng(5000 + c.seed + 13 * P)
    cam = synth.camera_for(c.poses[0], c.W, c.H)
    tanx, tany = cam["tanfovx"], cam["tanfovy"]
    fpx = c.W / (2.0 * tanx)
    f = np.float32
    g = {}
    u, v, z = rng.uniform(-0.85, 0.85, P), rng.uniform(-0.85, 0.85, P), rng.uniform(2.5, 6.0, P)
    scales = 0.05 * np.exp(0.3 * rng.standard_normal((P, 3)))
    sct = 0.5 * np.exp(0.3 * rng.standard_normal(P))
    ts = TIMESTAMP + c.mod * rng.uniform(-0.3, 0.3, P)
    ident = np.array([1.0, 0.0, 0.0, 0.0])
    rot = _unit(ident + 0.3 * rng.standard_normal((P, 4))) if c.rot_4d else _unit(rng.standard_normal((P, 4)))
    rot_r = _unit(ident + 0.3 * rng.standard_normal((P, 4)))
    qn, qnr = rng.uniform(0.5, 2.0, P), rng.uniform(0.5, 2.0, P)
    opa = 1.0 / (1.0 + np.exp(-rng.standard_normal(P)))
    M = c.M
    shs = 0.2 * rng.standard_normal((P, max(M, 1), 3))
    shs[:, 0, :] = rng.uniform(0.2, 1.0, (P, 3))
    n = 8 if P >= 257 else (4 if P >= 63 else 0)
    cur = [P]
    idx = {}

    def take(name, k=None):
        k = n if k is None else k
        cur[0] -= k
        idx[name] = np.arange(cur[0], cur[0] + k)
        return idx[name]

    def still(i):
        """no temporal model in the way: identity 4D rotation, ts == timestamp (marginal 1, no mean shift)"""
        rot[i], rot_r[i], ts[i] = ident, ident, TIMESTAMP

    pops = c.pops if n else ()
    if "dead_wave" in pops:
        z[0:64] = 0.1
        still(np.arange(64))
    if "clampx" in pops:
        i = take("clampx"); still(i)
        u[i], v[i], z[i] = 1.3 * np.where(np.arange(n) % 4 < 2, 1.0, -1.0), rng.uniform(-0.3, 0.3, n), 4.0
        scales[i] = 0.7 / c.mod
        i = take("clampx_far", n // 2); still(i)
        u[i], v[i], z[i], scales[i] = 1.5 * np.where(np.arange(len(i)) % 2 == 0, 1.0, -1.0), 0.2, 4.0, 0.7 / c.mod
    if "clampy" in pops:
        i = take("clampy"); still(i)
        v[i], u[i], z[i] = 1.3 * np.where(np.arange(n) % 4 < 2, 1.0, -1.0), rng.uniform(-0.3, 0.3, n), 4.0
        scales[i] = 0.7 / c.mod
        i = take("clampy_far", n // 2); still(i)
        v[i], u[i], z[i], scales[i] = 1.5 * np.where(np.arange(len(i)) % 2 == 0, 1.0, -1.0), -0.2, 4.0, 0.7 / c.mod
    if "edge" in pops:
        i = take("edge"); still(i)
        z[i] = 4.0
        scales[i] = 2.44 * 4.0 / fpx / c.mod                               # 3 sqrt(2.44^2 + 0.3) = 7.5: radius 8
        u[i], v[i] = rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n)
        k = np.arange(n // 2)
        u[i[:n // 2]] = (2.0 * np.where(k % 2 == 0, 40.0, 41.0) + 1.0) / c.W - 1.0     # (the bisection below makes pix an integer)
        v[i[n // 2:]] = (2.0 * np.where(k % 2 == 0, 24.0, 25.0) + 1.0) / c.H - 1.0
    if "outside" in pops:
        i = take("outside"); still(i)
        side = np.arange(n) % 4
        far = rng.uniform(1.05, 2.0, n)
        u[i] = np.where(side == 0, far, np.where(side == 1, -far, rng.uniform(-0.5, 0.5, n)))
        v[i] = np.where(side == 2, far, np.where(side == 3, -far, rng.uniform(-0.5, 0.5, n)))
        z[i], scales[i] = 4.0, (rng.uniform(0.5, 1.2, n) / c.mod)[:, None]
    if "zero_rect" in pops:
        i = take("zero_rect"); still(i)
        u[i], v[i], z[i], scales[i] = 1.9 * np.where(np.arange(n) % 2 == 0, 1.0, -1.0), rng.uniform(-0.5, 0.5, n), 4.0, 0.01 / c.mod
    if "needle" in pops:
        i = take("needle")
        u[i], v[i], z[i] = rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n), 5.0
        scales[i] = 0.002 / c.mod
        scales[i, rng.integers(0, 3, n)] = 60.0 * 5.0 / fpx / c.mod           # sigma_long ~ 60 px against the low pass's 0.55 px
        if c.rot_4d:   # (a 4D rotation puts part of the long axis into time and the conditioning shortens the needle: keep it small)
            rot[i], rot_r[i] = _unit(ident + 0.05 * rng.standard_normal((n, 4))), _unit(ident + 0.02 * rng.standard_normal((n, 4)))
            sct[i], ts[i] = 60.0 / c.mod, TIMESTAMP + rng.uniform(-0.05, 0.05, n)
        else:
            rot[i] = _unit(rng.standard_normal((n, 4)))
    if "det0" in pops:
        i = take("det0", n // 2)
        u[i], v[i], z[i] = rng.uniform(-0.3, 0.3, len(i)), rng.uniform(-0.3, 0.3, len(i)), 4.0
        scales[i] = np.array([400.0, 1e-3, 1e-3]) / c.mod
        rot[i] = np.array([math.cos(math.pi / 8), 0.0, 0.0, math.sin(math.pi / 8)])   # 45 degrees about z
    if "tiny_st" in pops:
        i = take("tiny_st")
        sct[i] = 1e-4 / c.mod
        ts[i] = TIMESTAMP + np.array([0.0, 1e-4, -1e-4, 2e-4, 0.5, -1.0, DURATION - TIMESTAMP, -TIMESTAMP])[:n]
    if "bits" in pops and M > 0:
        i = take("clamp3"); shs[i, 0, :] = -12.0
        i = take("clamp1"); shs[i, 0, 1] = -12.0
    if "opa" in pops:
        i = take("opa"); still(i)
        u[i], v[i] = rng.uniform(-0.6, 0.6, n), rng.uniform(-0.6, 0.6, n)
        i = take("faint"); still(i)                                        # clearly either side of 1/255
        opa[i] = np.where(np.arange(n) % 2 == 0, 0.002, 0.006)
        u[i], v[i] = rng.uniform(-0.6, 0.6, n), rng.uniform(-0.6, 0.6, n)
    if "marg" in pops:
        i = take("marg")
        u[i], v[i] = rng.uniform(-0.4, 0.4, n), rng.uniform(-0.4, 0.4, n)
    if "near" in pops:
        i = take("near"); still(i)
        z[i] = 0.2
        u[i], v[i] = rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n)
    assert cur[0] >= P // 3, "the populations leave no generic Gaussians"

    xyz = _world(cam, np.stack([u * tanx * z, v * tany * z, z], axis=1))
    g["means3D"] = f(xyz)
    g["opacities"] = f(np.log(opa / (1 - opa)) if c.raw else opa).reshape(P, 1)
    g["scales"] = f(np.log(scales) if c.raw else scales)
    g["rotations"] = f(rot * qn[:, None] if c.raw else rot)
    g["ts"] = f(ts).reshape(P, 1)
    g["scales_t"] = f(np.log(sct) if c.raw else sct).reshape(P, 1)
    g["rotations_r"] = f(rot_r * qnr[:, None] if c.raw else rot_r)
    g["shs"] = f(shs)
    g["colors_precomp"] = f(rng.uniform(0.0, 1.0, (P, 3)))
    g["flow_2d"] = f(0.5 * rng.standard_normal((P, 2)))
    if c.precomp_cov:
        R = np.transpose(co.quat_to_R(rot), (0, 2, 1))
        S = R @ (scales[:, :, None] ** 2 * np.transpose(R, (0, 2, 1)))
        g["cov3D_precomp"] = f(np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], axis=1))

    def scene_of():
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))   # noqa: E731
        sc = dict(cam)
        sc.update({"P": P, "W": c.W, "H": c.H, "M": M, "bg": torch.tensor([0.1, 0.2, 0.3]), "means3D": t(g["means3D"]), "sh_degree": c.D,
                   "sh_degree_t": c.D_t, "timestamp": TIMESTAMP, "time_duration": DURATION, "rot_4d": c.rot_4d, "gaussian_dim": c.dim,
                   "force_sh_3d": c.force_sh_3d, "scale_modifier": c.mod, "prefilter_var": c.pv, "raw": c.raw, "flow_2d": t(g["flow_2d"]),
                   "opacities": t(g["opacities"])})
        if M > 0:
            sc["shs"] = t(g["shs"])
        else:
            sc["colors_precomp"] = t(g["colors_precomp"])
        if c.precomp_cov:
            sc["cov3D_precomp"] = t(g["cov3D_precomp"])
        else:
            sc["scales"], sc["rotations"] = t(g["scales"]), t(g["rotations"])
        if c.dim == 4:
            sc["ts"], sc["scales_t"] = t(g["ts"]), t(g["scales_t"])
        if c.rot_4d:
            sc["rotations_r"] = t(g["rotations_r"])
        return sc

    # ---- the bisected populations: one fp32 input of each Gaussian moved until the float64 quantity changes sign ----
    def probe(i, key, col, quantity):
        """q(x): the oracle's ``quantity`` of Gaussians i with g[key][i, col] = x"""
        def q(x):
            keep = g[key][i, col].copy()
            g[key][i, col] = x
            o = po.forward(sub_inputs(oracle_inputs(scene_of()), i))
            g[key][i, col] = keep
            return quantity(o)
        return q

    def plant(name, key, col, quantity, lo, hi):
        i = idx[name]
        a, b = bisect(probe(i, key, col, quantity), lo, hi)
        g[key][i, col] = _sides(a, b, len(i))

    vm = cam["world_view_transform"].numpy().astype(np.float64).reshape(-1)
    if "near" in idx:
        i = idx["near"]
        plant("near", "means3D", 2, lambda o: o["near"], g["means3D"][i, 2] - 0.15, g["means3D"][i, 2] + 0.15)
    if "marg" in idx:
        i = idx["marg"]
        # the marginal's variance from the marginal itself: var = -dt^2 / (2 ln m)
        dt0 = g["ts"][i, 0].astype(np.float64) - TIMESTAMP
        dt0 = np.where(np.abs(dt0) < 1e-3, 0.1, dt0)
        g["ts"][i, 0] = f(TIMESTAMP + dt0)
        o = po.forward(sub_inputs(oracle_inputs(scene_of()), i))
        var = -dt0 * dt0 / (2.0 * np.log(o["marg"] + 0.05))
        edge = np.sqrt(-2.0 * var * math.log(0.05)) * np.where(np.arange(len(i)) % 4 < 2, 1.0, -1.0)
        plant("marg", "ts", 0, lambda o: o["marg"], f(TIMESTAMP + 0.8 * edge), f(TIMESTAMP + 1.25 * edge))
    if "opa" in idx:
        i = idx["opa"]
        lo, hi = (f(-6.5), f(-4.5)) if c.raw else (f(0.002), f(0.008))
        plant("opa", "opacities", 0, lambda o: o["opa255"], np.full(len(i), lo), np.full(len(i), hi))
    for name, col, tan in (("clampx", 0, tanx), ("clampy", 1, tany)):
        if name in idx:
            i = idx[name]
            sgn = np.sign(u[i] if col == 0 else v[i])

            def beyond(o, col=col, tan=tan, sgn=sgn):
                m = o["out_means3D"]
                tz = vm[2] * m[:, 0] + vm[6] * m[:, 1] + vm[10] * m[:, 2] + vm[14]
                tx = vm[col] * m[:, 0] + vm[4 + col] * m[:, 1] + vm[8 + col] * m[:, 2] + vm[12 + col]
                return sgn * tx / tz - co.CLAMP * co.f32(tan)
            w = g["means3D"][i, col]
            plant(name, "means3D", col, beyond, w - f(0.6) * f(sgn), w + f(0.6) * f(sgn))
    if "edge" in idx:
        i = idx["edge"]
        # pix.x of the first half and pix.y of the second an integer N: N - 8 = 32 (16) or N + 8 + 15 = 64 (48)
        half = len(i) // 2
        Nx, Ny = (40.0, 41.0), (24.0, 25.0)
        for part, col, Ns in ((i[:half], 0, Nx), (i[half:], 1, Ny)):
            tgt = np.array([Ns[k % 2] for k in range(len(part))])
            w = g["means3D"][part, col]
            off = probe(part, "means3D", col, lambda o, col=col, tgt=tgt: o["pix_all"][:, col] - tgt)
            a, b = bisect(off, w - f(0.3), w + f(0.3))
            g["means3D"][part, col] = np.where(np.abs(off(a)) <= np.abs(off(b)), a, b)

    planted = np.zeros(P, bool)
    for name in ("near", "marg", "opa", "clampx", "clampy", "edge", "det0", "tiny_st"):
        if name in idx:
            planted[idx[name]] = True
    sc = scene_of()
    views = []
    for vw, pose in enumerate(c.poses):
        cv = synth.camera_for(pose, c.W, c.H)
        views.append(dict(cv, timestamp=TIMESTAMP + 0.11 * vw))
    return {"case": c, "scene": sc, "views": views, "planted": planted, "idx": idx}


def view_scene(built, v):
    return dict(built["scene"], **built["views"][v])


def oracle_inputs(scene):
    """preprocess_oracle.forward's ``inp`` of a scene dict: numpy arrays, every scalar as the fp32 value the C ABI receives."""
    n = int(scene["means3D"].shape[0])
    g = lambda k: None if scene.get(k) is None else scene[k].numpy()   # noqa: E731
    r = lambda k: None if g(k) is None else g(k).reshape(n)   # noqa: E731
    return {"P": n, "D": int(scene["sh_degree"]), "D_t": int(scene["sh_degree_t"]), "M": int(scene["M"]), "W": int(scene["W"]),
            "H": int(scene["H"]), "means3D": g("means3D"), "shs": g("shs"), "colors_precomp": g("colors_precomp"),
            "opacities": r("opacities"), "ts": r("ts"), "scales": g("scales"), "scales_t": r("scales_t"), "rotations": g("rotations"),
            "rotations_r": g("rotations_r"), "cov3D_precomp": g("cov3D_precomp"),
            "viewmatrix": scene["world_view_transform"].numpy().reshape(16), "projmatrix": scene["full_proj_transform"].numpy().reshape(16),
            "campos": scene["camera_center"].numpy(), "tan_fovx": co.f32(scene["tanfovx"]), "tan_fovy": co.f32(scene["tanfovy"]),
            "timestamp": co.f32(scene["timestamp"]), "time_duration": co.f32(scene["time_duration"]),
            "scale_modifier": co.f32(scene["scale_modifier"]), "prefilter_var": co.f32(scene["prefilter_var"]),
            "rot_4d": bool(scene["rot_4d"]), "gaussian_dim": int(scene["gaussian_dim"]), "force_sh_3d": bool(scene["force_sh_3d"]),
            "raw": bool(scene.get("raw"))}


PER_GAUSSIAN = ("means3D", "shs", "colors_precomp", "opacities", "ts", "scales", "scales_t", "rotations", "rotations_r", "cov3D_precomp")


def sub_inputs(inp, i):
    out = dict(inp)
    for k in PER_GAUSSIAN:
        if inp.get(k) is not None:
            out[k] = inp[k][i]
    out["P"] = len(i)
    return out


def activated(scene, act=None):
    """The scene with activated parameters, for the port, which has no raw mode.  ``act``: the kernels' own activations (opacity,
    scales, scales_t, rotations, rotations_r as numpy; the GPU test passes fdgs_debug_activations' so that a flagged decision is
    compared on the same fp32 inputs); None: fp32 torch exp / sigmoid / normalisation."""
    if not scene.get("raw"):
        return scene
    s = dict(scene)
    if act is not None:
        for k, a in zip(("opacities", "scales", "scales_t", "rotations", "rotations_r"), act):
            if s.get(k) is not None and a is not None:
                s[k] = torch.from_numpy(np.ascontiguousarray(a)).reshape(s[k].shape)
    else:
        for k in ("scales", "scales_t"):
            if s.get(k) is not None:
                s[k] = torch.exp(s[k])
        for k in ("rotations", "rotations_r"):
            if s.get(k) is not None:
                s[k] = s[k] / s[k].norm(dim=1, keepdim=True).clamp_min(1e-12)
        s["opacities"] = torch.sigmoid(s["opacities"])
    s["raw"] = False
    return s


def populations(inp, base, fl):
    """How many Gaussians of each population the float64 evaluation shows."""
    P, W, H = inp["P"], inp["W"], inp["H"]
    al = base["alive"]
    vm = np.asarray(inp["viewmatrix"], np.float64)
    m = base["out_means3D"]
    out = {"culled": int((~al).sum()), "alive": int(al.sum())}
    with np.errstate(all="ignore"):
        tz = vm[2] * m[:, 0] + vm[6] * m[:, 1] + vm[10] * m[:, 2] + vm[14]
        tx = np.abs((vm[0] * m[:, 0] + vm[4] * m[:, 1] + vm[8] * m[:, 2] + vm[12]) / tz) / (co.CLAMP * inp["tan_fovx"]) - 1.0
        ty = np.abs((vm[1] * m[:, 0] + vm[5] * m[:, 1] + vm[9] * m[:, 2] + vm[13]) / tz) / (co.CLAMP * inp["tan_fovy"]) - 1.0
        for nm, t in (("clampx", tx), ("clampy", ty)):
            out[nm + "_lo"] = int((al & (t <= 0) & (t > -1e-5)).sum())
            out[nm + "_hi"] = int((al & (t > 0) & (t < 1e-5)).sum())
            out[nm + "_far"] = int((al & (t > 0.1)).sum())
        for nm, q, f in (("near", base["near"], fl["near"]), ("marg", base["marg"], fl["marg"]), ("opa", base["opa255"], fl["opa"])):
            if q is not None:
                out[nm + "_lo"], out[nm + "_hi"] = int((f & (q <= 0)).sum()), int((f & (q > 0)).sum())
        qd = np.abs(base["quot"] - np.round(base["quot"]))
        out["edge"] = int((al & (base["radius"] == 8) & (qd < 1e-6).any(1)).sum())
        px = base["pix_all"]
        out["outside"] = int((al & ((px[:, 0] < 0) | (px[:, 0] > W) | (px[:, 1] < 0) | (px[:, 1] > H))).sum())
        gx, gy = (W + 15) // 16, (H + 15) // 16
        qt = base["quot"]
        out["rect_clamped"] = int((al & ((qt[:, 0] < 0) | (qt[:, 1] < 0) | (qt[:, 2] >= gx + 1) | (qt[:, 3] >= gy + 1))).sum())
        rad_ok = np.ceil(np.nan_to_num(base["rad"])) > 0
        out["zero_rect"] = int((~al & base["alive_n"] & (base["det"] != 0) & rad_ok).sum())
        a, b, c = (base["conic"][:, k] for k in range(3))
        mid, det = 0.5 * (a + c), a * c - b * b
        root = np.sqrt(np.maximum(mid * mid - det, 0.0))
        out["needle"] = int((al & (np.sqrt((mid + root) / np.maximum(mid - root, 1e-300)) >= 60.0)).sum())
    if inp.get("scales_t") is not None and inp["rot_4d"]:
        st = (np.exp(inp["scales_t"].astype(np.float64)) if inp["raw"] else inp["scales_t"].astype(np.float64)) * inp["scale_modifier"]
        out["tiny_st_alive"], out["tiny_st_culled"] = int((al & (st <= 1.01e-4)).sum()), int((~base["alive_t"] & (st <= 1.01e-4)).sum())
    out["det0"] = int(fl["det"].sum())
    if base["rgb_pre"] is not None:
        cl = base["clamped"].sum(1)
        out["clamp3"], out["clamp1"], out["clamp0"] = int((al & (cl == 3)).sum()), int((al & (cl == 1)).sum()), int((al & (cl == 0)).sum())
    full = [al[k:k + 64] for k in range(0, P - 63, 64)]
    out["dead_wave"] = int(sum(1 for w in full if not w.any()))
    return out


NEED = {"near": ("near_lo", "near_hi"), "marg": ("marg_lo", "marg_hi"), "opa": ("opa_lo", "opa_hi"),
        "clampx": ("clampx_lo", "clampx_hi", "clampx_far"), "clampy": ("clampy_lo", "clampy_hi", "clampy_far"), "edge": ("edge",),
        "outside": ("outside", "rect_clamped"), "zero_rect": ("zero_rect",), "needle": ("needle",), "tiny_st": ("tiny_st_alive", "tiny_st_culled"),
        "det0": ("det0",), "bits": ("clamp3", "clamp1", "clamp0"), "dead_wave": ("dead_wave",)}


def assert_populations(case, inp, base, fl, planted):
    """The populations of view 0 are there (two of a side at least), and the flag cap holds: at most FLAG_CAP of the case's Gaussians
    have a flagged decision without having been planted on its edge."""
    got = populations(inp, base, fl)
    if case.P >= 63:
        short = {k: got.get(k, 0) for p in case.pops for k in NEED[p] if got.get(k, 0) < (1 if k in ("dead_wave", "det0") else 2)}
        assert not short, "%s: populations short: %r (all: %r)" % (case.name, short, got)
    stray = (fl["geo"] | fl["rgb"].any(1) | fl["opa"]) & ~planted
    got["flagged"], got["stray"] = int((fl["geo"] | fl["rgb"].any(1) | fl["opa"]).sum()), int(stray.sum())
    assert stray.sum() <= FLAG_CAP * case.P, "%s: %d Gaussians sit on a decision's edge by accident (cap %.1f): %r" % (
        case.name, int(stray.sum()), FLAG_CAP * case.P, np.nonzero(stray)[0][:10])
    return got


def worst(got, exp, core):
    return_value = np.nan_to_num(np.abs(np.asarray(got, np.float64).reshape(exp.shape) - exp), nan=np.inf) / core
    if return_value.size == 0:
        return 0.0, ()
    i = np.unravel_index(int(np.argmax(return_value)), return_value.shape)
    return float(return_value[i]), i
