"""Scenes, cameras and the CASES table shared by tests/test_flow_host.py and tests/test_gpu_flow.py: 64 x 48 images (one case 17 x 9),
at most 1000 Gaussians."""
import numpy as np
import torch

import flow_oracle as fo
from fdgs import synth

W, H = 64, 48
T0, T1 = 0.4, 0.5          # source and target time, duration 1
ROT_SIGMA = 0.3            # far enough from the identity that the Gaussians move by tens of pixels per unit of time


class Cam:
    """The camera members render() and gaussian_flow() read, from a synth scene dict."""

    def __init__(self, scene, dev="cpu", timestamp=None):
        self.FoVx, self.FoVy, self.image_height, self.image_width = scene["FoVx"], scene["FoVy"], scene["H"], scene["W"]
        self.world_view_transform = scene["world_view_transform"].to(dev)
        self.full_proj_transform = scene["full_proj_transform"].to(dev)
        self.camera_center = scene["camera_center"].to(dev)
        self.timestamp = scene["timestamp"] if timestamp is None else float(timestamp)


def make_scene(P, rot_4d, pose, t, seed=3, gaussian_dim=4, W=W, H=H):
    cfg = synth.SceneConfig("flow", P, W, H, 0, 0, 0.03, 1.0, rot_4d, gaussian_dim, False)
    return synth.make_scene(cfg, seed=seed, pose=pose, timestamp_frac=t, rot_sigma=ROT_SIGMA)


def pair(P, rot_4d, poses, seed=3, gaussian_dim=4, t1=T1, W=W, H=H):
    """(source scene at T0 seen from poses[0], target scene at t1 seen from poses[1]): the same Gaussians."""
    return make_scene(P, rot_4d, poses[0], T0, seed, gaussian_dim, W, H), make_scene(P, rot_4d, poses[1], t1, seed, gaussian_dim, W, H)


def params_of(scene, raw):
    """The six tensors by flow_oracle.NAMES; ``raw``: logarithms of the scales and quaternions of norm 0.5 .. 1.5."""
    par = {n: scene[n].clone() for n in fo.NAMES}
    if raw:
        P = par["means3D"].shape[0]
        par["scales"], par["scales_t"] = par["scales"].log(), par["scales_t"].log()
        g = torch.Generator().manual_seed(5)
        par["rotations"] = par["rotations"] * (0.5 + torch.rand(P, 1, generator=g))
        par["rotations_r"] = par["rotations_r"] * (0.5 + torch.rand(P, 1, generator=g))
    return par


def cam_args(s0, s1):
    """The leading arguments of flow_oracle.gaussian_flow for the two scenes' cameras."""
    return (s0["world_view_transform"], s0["full_proj_transform"], s0["timestamp"], s1["world_view_transform"], s1["full_proj_transform"],
            s1["timestamp"], int(s0["W"]), int(s0["H"]))


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------------
# Cases of the element-by-element comparison (tests/test_flow_host.py on the CPU, tests/test_gpu_flow.py on the GPU)
#
# Two families, each with its own K per output tensor, so that the hard inputs do not price the bar of the ordinary ones:
#   generic   the fc.pair scenes above: every P around the 64-lane wave and the 256-thread workgroup, raw and activated parameters,
#             modifier 1 and 0.7, the three camera forms (two cameras; one camera as NULL target matrices; one camera as equal but
#             distinct matrix buffers), plain 4D and 3D models with two cameras, one 17 x 9 image.
#   hard      P = 257 and 1000, two cameras; populations placed by index from the end of the index range (n = 4 / 8 members each) and
#             counted again from the float64 oracle by ``populations`` -- a seed that loses one must not pass empty:
#     behind_src / behind_tgt / behind_both   view-space z <= 0.2 at the source only, the target only, both: no flow, no gradient
#     near_z       valid, view-space z in (0.2, 0.25] at one end: 1 / h_w at its largest
#     far_pix      valid, projecting beyond 4 max(W, H) at one end
#     ts_t0 / ts_t1   t_i == t_0 / t_1 exactly: one dt is 0
#     far_time     |t - t_i| of 50 durations
#     identity     both quaternions (1, 0, 0, 0): c = 0 and w = 0 exactly
#     needle       scales of ratio 1:100
#     st_small / st_big   temporal scale 1e-4 / 60
#     qnorm_small / qnorm_big   raw quaternions of norm 1e-3 / 1e3 (raw cases)
#     qnorm_free   activated quaternions of norm 0.5 .. 1.5, which enter as passed (activated cases)
#     dl_zero / dl_one / dl_big   dL_dflows rows that are zero, have one component, are of magnitude 1e3 (by index % 16)
# The near cull is a discrete decision: every case keeps every view-space z, at both ends and for every perturbed draw, away from 0.2
# by a relative 1e-4 (flow_oracle.sensitivity asserts it), so the validity mask must equal the oracle's and no element is exempt.
# ---------------------------------------------------------------------------------------------------------------------------------
import functools  # noqa: E402
from typing import NamedTuple  # noqa: E402

import chain_oracle as co  # noqa: E402

SCALE = 0.37    # the ``scale`` argument of fdgs_gaussian_flow_backward in the value tests
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)
SEEDS = {1: 4, 63: 4, 64: 4, 65: 4, 255: 3, 256: 3, 257: 3, 1000: 3}
CAMS = ("two", "null", "equal")


class Case(NamedTuple):
    name: str
    family: str              # generic | hard
    P: int
    raw: bool = False
    mod: float = 1.0
    cams: str = "two"        # two | null (one camera: NULL target matrices) | equal (one camera: equal but distinct matrix buffers)
    rot_4d: bool = True
    dim: int = 4
    W: int = W
    H: int = H


def _generic():
    out = []
    for raw in (True, False):
        for k, P in enumerate(SIZES):   # k -> (modifier, camera form): all six pairs occur for raw and for activated parameters
            mod, cams = (1.0, 0.7)[k % 2], CAMS[(k // 2) % 3]
            out.append(Case("%s_p%d_%s_mod%g" % ("raw" if raw else "act", P, cams, mod), "generic", P, raw, mod, cams))
    out.append(Case("plain4d_p257", "generic", 257, rot_4d=False, dim=4))
    out.append(Case("plain3d_p65", "generic", 65, rot_4d=False, dim=3))
    out.append(Case("raw_p65_17x9", "generic", 65, True, 0.7, W=17, H=9))
    return out


CASES = _generic() + [
    Case("hard_raw_p257", "hard", 257, True, 0.7), Case("hard_act_p257", "hard", 257, False, 1.0),
    Case("hard_raw_p1000", "hard", 1000, True, 1.0), Case("hard_act_p1000", "hard", 1000, False, 0.7)]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

POSITIONAL = ("behind_src", "behind_tgt", "behind_both", "near_z", "far_pix")
HARD_POPULATIONS = POSITIONAL + ("ts_t0", "ts_t1", "far_time", "identity", "needle", "st_small", "st_big", "dl_zero", "dl_one", "dl_big")


def need(case):
    if case.family != "hard":
        return ()
    return HARD_POPULATIONS + (("qnorm_small", "qnorm_big") if case.raw else ("qnorm_free",))


def members(case):
    return 4 if case.P < 1000 else 8


def _world(scene, xv):
    """World points of view-space points xv [n,3] (float64): x_view = [x, 1] world_view_transform."""
    wv = scene["world_view_transform"].numpy().astype(np.float64)
    return (xv - wv[3, :3]) @ np.linalg.inv(wv[:3, :3])


def _ends(scene0, scene1, p, w, ti):
    """(z0, z1, max|pix0|, max|pix1|) in float64 of candidate means p [n,3] of ONE Gaussian with velocity w and time ti."""
    f = lambda s, k: s[k].numpy().astype(np.float64)   # noqa: E731
    Wd, Hd = int(scene0["W"]), int(scene0["H"])
    t0, t1 = float(np.float32(scene0["timestamp"])), float(np.float32(scene1["timestamp"]))
    pix0, z0, _, _ = fo._end(p + w * (t0 - ti), f(scene0, "world_view_transform"), f(scene0, "full_proj_transform"), Wd, Hd, np.float64)
    pix1, z1, _, _ = fo._end(p + w * (t1 - ti), f(scene1, "world_view_transform"), f(scene1, "full_proj_transform"), Wd, Hd, np.float64)
    return z0, z1, np.abs(pix0).max(1), np.abs(pix1).max(1)


def _hard(case, s0, s1, par_act, rng):
    """The activated parameters with the hard populations written in by index -> (parameters, dL_dflows, {population: indices})."""
    P, n = case.P, members(case)
    a = {k: v.numpy().astype(np.float64) for k, v in par_act.items()}
    qn, qnr = np.ones(P), np.ones(P)
    if case.raw:
        qn, qnr = rng.uniform(0.5, 2.0, P), rng.uniform(0.5, 2.0, P)
    unit = lambda q: q / np.linalg.norm(q, axis=1, keepdims=True)   # noqa: E731
    ident = np.array([1.0, 0.0, 0.0, 0.0])
    cur, pops = [P], {}

    def take(name):
        cur[0] -= n
        pops[name] = np.arange(cur[0], cur[0] + n)
        return pops[name]

    for name in POSITIONAL:
        take(name)
    a["ts"][take("ts_t0"), 0] = np.float32(T0)
    a["ts"][take("ts_t1"), 0] = np.float32(T1)
    i = take("far_time")       # (a small 4D rotation: w = tan of its angle, and the mean travels 50 w)
    a["ts"][i, 0] = T0 + 50.0 * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    a["rotations"][i], a["rotations_r"][i] = unit(ident + 0.01 * rng.standard_normal((n, 4))), unit(ident + 0.01 * rng.standard_normal((n, 4)))
    i = take("identity")
    a["rotations"][i], a["rotations_r"][i] = ident, ident
    qn[i], qnr[i] = 1.0, 1.0
    i = take("needle")
    a["scales"][i] = 0.003
    a["scales"][i, rng.integers(0, 3, n)] = 0.3
    a["scales_t"][take("st_small"), 0] = 1e-4 / case.mod
    a["scales_t"][take("st_big"), 0] = 60.0 / case.mod
    if case.raw:
        i = take("qnorm_small"); qn[i] = 1e-3; qnr[i[n // 2:]] = 1e-3     # noqa: E702
        i = take("qnorm_big"); qn[i] = 1e3; qnr[i[n // 2:]] = 1e3         # noqa: E702
    else:
        i = take("qnorm_free")   # (0.5 .. 0.9 and 1.1 .. 1.5: none that is a unit quaternion by chance)
        qn[i] = 1.0 + rng.uniform(0.1, 0.5, n) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        qnr[i] = 1.0 + rng.uniform(0.1, 0.5, n) * np.where(np.arange(n) % 4 < 2, 1.0, -1.0)
    assert cur[0] >= P // 3, "the populations leave no generic Gaussians"

    t = lambda x: torch.from_numpy(np.ascontiguousarray(np.float32(x)))   # noqa: E731
    par = {"means3D": t(a["means3D"]), "ts": t(a["ts"]),
           "scales": t(np.log(a["scales"]) if case.raw else a["scales"]), "scales_t": t(np.log(a["scales_t"]) if case.raw else a["scales_t"]),
           "rotations": t(a["rotations"] * qn[:, None]), "rotations_r": t(a["rotations_r"] * qnr[:, None])}

    # positions: the velocity does not depend on them, so each member takes the first unused candidate its population accepts
    w = fo.analytic(*cam_args(s0, s1), par, torch.zeros(P, 2), rot_4d=True, raw=case.raw, scaling_modifier=case.mod)["w"]
    ti = par["ts"].numpy().astype(np.float64).reshape(P)
    t0, t1 = float(np.float32(s0["timestamp"])), float(np.float32(s1["timestamp"]))
    big = 4.0 * max(case.W, case.H)
    box = np.stack([rng.uniform(-3.0, 3.0, 6000), rng.uniform(-3.0, 3.0, 6000), rng.uniform(-6.5, 2.0, 6000)], axis=1)

    def slab(scene, zlo, zhi, ulo, uhi, m=400):
        z = rng.uniform(zlo, zhi, m)
        u = rng.uniform(ulo, uhi, m) * np.where(rng.random(m) < 0.5, -1.0, 1.0)
        v = rng.uniform(-0.5, 0.5, m)
        return _world(scene, np.stack([u * scene["tanfovx"] * z, v * scene["tanfovy"] * z, z], axis=1))

    accept = {
        "ordinary": lambda z0, z1, p0, p1: (z0 > 0.5) & (z1 > 0.5) & (p0 <= 0.5 * big) & (p1 <= 0.5 * big),
        "behind_src": lambda z0, z1, p0, p1: (z0 < 0.15) & (z1 > 0.3),
        "behind_tgt": lambda z0, z1, p0, p1: (z1 < 0.15) & (z0 > 0.3),
        "behind_both": lambda z0, z1, p0, p1: (z0 < 0.15) & (z1 < 0.15),
        "near_z0": lambda z0, z1, p0, p1: (z0 > 0.202) & (z0 < 0.248) & (z1 > 0.3),
        "near_z1": lambda z0, z1, p0, p1: (z1 > 0.202) & (z1 < 0.248) & (z0 > 0.3),
        "far_pix0": lambda z0, z1, p0, p1: (z0 > 0.3) & (z1 > 0.3) & (p0 > 1.1 * big),
        "far_pix1": lambda z0, z1, p0, p1: (z0 > 0.3) & (z1 > 0.3) & (p1 > 1.1 * big),
    }
    pools = {"near_z0": slab(s0, 0.205, 0.245, 0.0, 0.6), "near_z1": slab(s1, 0.205, 0.245, 0.0, 0.6),
             "far_pix0": slab(s0, 0.6, 1.5, 9.0, 14.0), "far_pix1": slab(s1, 0.6, 1.5, 9.0, 14.0)}
    used = {k: np.zeros(len(v), bool) for k, v in dict(pools, box=box).items()}
    xyz = a["means3D"].copy()

    def place(i, rule):
        pool = rule if rule in pools else "box"
        cand = box
        if rule in pools:   # the pool holds where the mean is to BE at that end: step back along the Gaussian's own motion
            cand = pools[rule] - w[i] * ((t0 if rule.endswith("0") else t1) - ti[i])
        good = accept[rule](*_ends(s0, s1, cand, w[i], ti[i])) & ~used[pool]
        if not good.any() and rule.endswith("1"):   # (the rig leaves no room in front of the target's near plane: the other end)
            return place(i, rule[:-1] + "0")
        assert good.any(), "%s: no candidate position for Gaussian %d (%s)" % (case.name, i, rule)
        j = int(np.argmax(good))
        used[pool][j] = True
        xyz[i] = cand[j]

    for name, idx in pops.items():
        for k, i in enumerate(idx):
            rule = name if name in ("behind_src", "behind_tgt", "behind_both") else (
                name + "01"[k % 2] if name in ("near_z", "far_pix") else ("ordinary" if name in ("far_time", "st_small") else None))
            if rule:
                place(int(i), rule)
    par["means3D"] = t(xyz)

    dL = rng.standard_normal((P, 2))
    idx = np.arange(P)
    dL[idx % 16 == 3] = 0.0
    one = np.nonzero(idx % 16 == 5)[0]
    dL[one, (one // 16) % 2] = 0.0
    dL[idx % 16 == 7] *= 1e3
    return par, t(dL), pops


@functools.lru_cache(maxsize=None)
def build(case):
    """-> dict(case, s0, s1: the two scene dicts, cam: flow_oracle's leading arguments, par: the six CPU float32 tensors by
    flow_oracle.NAMES, dL: [P,2] float32, placed: {population: indices} as placed).  Cached: nobody changes what it returns."""
    poses = ("rig0", "rig1") if case.cams == "two" else ("rig0", "rig0")
    s0, s1 = pair(case.P, case.rot_4d, poses, seed=SEEDS[case.P], gaussian_dim=case.dim, W=case.W, H=case.H)
    rng = np.random.default_rng(500 + case.P + (7 if case.raw else 0))
    if case.family == "hard":
        par, dL, placed = _hard(case, s0, s1, params_of(s0, False), rng)
    else:
        par, placed = params_of(s0, case.raw), {}
        dL = torch.randn(case.P, 2, generator=torch.Generator().manual_seed(11 + case.P))
    return {"case": case, "s0": s0, "s1": s1, "cam": cam_args(s0, s1), "par": par, "dL": dL, "placed": placed}


def settings(case):
    return dict(rot_4d=case.rot_4d, raw=case.raw, scaling_modifier=case.mod)


@functools.lru_cache(maxsize=None)
def oracle(case):
    """-> (float64 result, sens) of flow_oracle.sensitivity for the case at scale SCALE, by flow_oracle.OUTPUTS (+ ok, z, pix).  Cached."""
    b = build(case)
    return fo.sensitivity(*b["cam"], b["par"], b["dL"], scale=SCALE, **settings(case))


def float32_statement(case):
    b = build(case)
    return fo.analytic(*b["cam"], b["par"], b["dL"], scale=SCALE, dtype=np.float32, **settings(case))


def populations(case, f64, flows=None):
    """How many Gaussians of each population the float64 oracle shows (and, with ``flows``, this run's flows agree on: a valid Gaussian
    has a finite flow, one behind a camera the bits of (0, 0))."""
    b = build(case)
    par = {k: v.numpy().astype(np.float64) for k, v in b["par"].items()}
    P = case.P
    ok, z0, z1 = f64["ok"].copy(), f64["z0"], f64["z1"]
    b0, b1 = z0 <= 0.2, z1 <= 0.2
    if flows is not None:
        fl = np.asarray(flows, np.float32).reshape(P, 2)
        zero = (bits(fl) == 0).all(1)
        ok, b0, b1 = ok & np.isfinite(fl).all(1), b0 & zero, b1 & zero
    big = 4.0 * max(case.W, case.H)
    out = {"behind_src": b0 & ~b1, "behind_tgt": b1 & ~b0, "behind_both": b0 & b1,
           "near_z": ok & (((z0 > 0.2) & (z0 <= 0.25)) | ((z1 > 0.2) & (z1 <= 0.25))),
           "far_pix": ok & ((np.abs(f64["pix0"]).max(1) > big) | (np.abs(f64["pix1"]).max(1) > big))}
    if case.rot_4d:
        ts = b["par"]["ts"].numpy().reshape(P)
        t0, t1 = np.float32(b["s0"]["timestamp"]), np.float32(b["s1"]["timestamp"])
        out["ts_t0"], out["ts_t1"] = ok & (ts == t0), ok & (ts == t1)
        out["far_time"] = ok & (np.abs(float(t0) - ts.astype(np.float64)) >= 49.9)
        ident = np.array([1.0, 0.0, 0.0, 0.0])
        out["identity"] = ok & (par["rotations"] == ident).all(1) & (par["rotations_r"] == ident).all(1)
        sc = np.exp(par["scales"]) if case.raw else par["scales"]
        sct = (np.exp(par["scales_t"]) if case.raw else par["scales_t"]).reshape(P) * float(np.float32(case.mod))
        out["needle"] = ok & (sc.max(1) / sc.min(1) >= 99.0)
        out["st_small"], out["st_big"] = ok & (sct <= 1.01e-4), ok & (sct >= 59.0)
        qn, qnr = np.linalg.norm(par["rotations"], axis=1), np.linalg.norm(par["rotations_r"], axis=1)
        if case.raw:
            out["qnorm_small"], out["qnorm_big"] = ok & (np.minimum(qn, qnr) < 2e-3), ok & (np.maximum(qn, qnr) > 5e2)
        else:
            out["qnorm_free"] = ok & (np.abs(qn - 1.0) > 0.02) & (np.abs(qnr - 1.0) > 0.02) & (qn > 0.49) & (qn < 1.51)
    dL = b["dL"].numpy()
    out["dl_zero"], out["dl_one"] = ok & (dL == 0).all(1), ok & ((dL != 0).sum(1) == 1)
    out["dl_big"] = ok & (np.abs(dL).max(1) >= 500.0)
    return {k: int(v.sum()) for k, v in out.items()}


def assert_populations(case, f64, flows=None):
    got = populations(case, f64, flows)
    short = {k: got.get(k, 0) for k in need(case) if got.get(k, 0) < 4}
    assert not short, "%s: populations short of 4 Gaussians: %r (all: %r)" % (case.name, short, got)
    return got


# K[family][tensor] = 4 * r32: r32 = the worst ratio |float32 statement - f64| / (4 ulp32 of |f64_e| + sens_e) on that tensor over the
# family's cases, measured on the CPU by tests/test_flow_host.py::test_float32_statement_pins_K (which fails if a constant drifts from
# 4 * r32 by more than K_TOLERANCE); the factor 4 is the project's margin for another legal float32 evaluation (chain_cases.K): the
# kernels' expf, reciprocal and sum orders differ from numpy's.  Never from a kernel's output.  BASELINE.md section 7b has the table.
K = {
    "generic": {"flows": 518.0, "means3D": 710.0, "ts": 762.0, "scales": 20.9, "scales_t": 799.0, "rotations": 26.3, "rotations_r": 41.1},
    "hard": {"flows": 38.5, "means3D": 63.3, "ts": 27.2, "scales": 18.1, "scales_t": 3.41e6, "rotations": 22.0, "rotations_r": 41.8},
}
K_TOLERANCE = 0.10


def ratios(got, f64, sens):
    """{tensor: (worst ratio, element)} of ``got`` (by flow_oracle.OUTPUTS) against the float64 result and its sensitivity."""
    out = {}
    for k in fo.OUTPUTS:
        r = co.ratio(got[k], f64[k], sens[k])
        out[k] = (float(r.max()), np.unravel_index(int(r.argmax()), r.shape)) if r.size else (0.0, ())
    return out
