"""Cases of the per-Gaussian backward tests (tests/test_chain_oracle_host.py on the CPU, tests/test_gpu_gaussian_backward.py on the
GPU): seeded, tiny, built by construction.  A case is a scene (one view or several), the accumulator records [P,12] of every view
(tests/chain_oracle.py for the word layout), a mode, and the POPULATIONS it exists for; both tests count those populations from the
forward's own radii and records (``populations``) and fail when one is short -- a seed that loses a population must not pass empty.

Which path a case exists for is in its line of CASES.  Populations (``need``), at least 8 Gaussians each where P allows:
  clamp_x / clamp_y / clamp_xy   visible, view-space x/z (y/z, both) beyond 1.3 * tan_fov: x_grad_mul / y_grad_mul = 0 (backward.cu:540-543);
                                 a large splat, or they would not reach the image
  ts_equal                       ts == timestamp exactly (dt = 0: the marginal chain's dt factors vanish)
  near_cull                      temporal marginal within 10 % above the 0.05 cull
  needle                         1:100 on screen (from the conic record)
  tiny                           scales of 1e-4: the 0.3 low-pass dominates the 2D covariance
  qnorm_small / qnorm_big        raw quaternions of norm 1e-3 / 1e3
  opac_pos / opac_neg            raw opacity +15 / -15
  clamp3 / clamp1 / clamp0       all three colour channels clamped, exactly one, none
  rec_zero / rec_colour / rec_moments / rec_negzero / rec_culled
                                 accumulator records: all zero on a visible Gaussian; colour words only (SH live, geometry moments
                                 zero); moments only (SH dead, geometry active); a -0.0 word (the bit test of the re-zero); non-zero
                                 on a culled Gaussian
  culled                         radii == 0
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
from fdgs import synth  # noqa: E402

# K_tensor = 4 * r_port (BASELINE.md section "Per-Gaussian backward against float64"): r_port = the worst ratio
# |port32 - f64| / (4 ulp32 of |f64_e| + sens_e) the fp32 port shows on that tensor over every case, measured by
# tests/test_chain_oracle_host.py::test_port_pinned_and_K (which fails if a constant drifts from 4 * r_port); the factor 4 because the
# HIP kernels are another legal fp32 evaluation (their expf, sigmoid, reciprocal and three-term sum orders differ), not the port's own.
# The port exposes neither the hand-over words' time word behind rot_4d nor the stage records: "stage" (a copy of dRGB, one
# normalisation, one cosine evaluated in double) is held to r = 1, and "sh_words" to the larger of its own r_port (mean words of every
# SH case, time word of the cases without rot_4d) and dL_dmean3D's.
K = {
    "dL_dmean2D": 1.20, "dL_dcolor": 0.0, "dL_dflows": 0.0, "dL_dcov3D": 884.0, "dL_dmean3D": 21.5, "dL_dopacity": 3.13e5, "dL_dts": 3.33,
    "dL_dscale": 1.99e5, "dL_dscale_t": 7.69e8, "dL_drot": 1.08e4, "dL_drot_r": 2.26e4, "dL_dsh": 3.62, "sh_words": 21.5, "stage": 4.0,
}
# What the large constants say (BASELINE.md has the elements): sens_e sees what an ulp on the INPUTS does, not what an ulp on an
# intermediate does to a sum that cancels by structure for every input -- dL_dscale of a needle's short axes, dL_dscale_t where the
# mean shift c12 / cov_t does not depend on it (1e-4 scales, a temporal extent of 60), o (1 - o) at a raw opacity of +15.  There any
# fp32 evaluation, the port's included, is off by ulps of the cancelling terms; r_port records it, and it prices the whole tensor.
K_TOLERANCE = 0.10   # |K - 4 r_port| <= 10 % of K: another libm may move an expf by an ulp, nothing moves r_port by more


class Case(NamedTuple):
    name: str
    P: int
    dim: int                 # gaussian_dim
    rot_4d: bool
    D: int
    D_t: int
    M: int                   # 0: colors_precomp, no SH
    raw: bool = False
    mod: float = 1.0
    pv: float = -1.0         # prefilter_var
    analytic: bool = False
    force_sh_3d: bool = False
    precomp_cov: bool = False
    live: str = "all"        # all | none | alternate | 64plus1 | lastwave: which Gaussians carry a colour gradient (SH wave compaction)
    mode: str = "overwrite"  # overwrite | accumulate (onto a seeded prefill) | noperview (per_view_outputs=False)
    views: int = 1           # staged views, flushed with sh_flush in view order (views > 1: gradient accumulation over them)
    need: tuple = ()
    seed: int = 0
    W: int = 64
    H: int = 48
    period: int = 0          # > 0: Gaussian i is Gaussian i % period (the large case: the oracle runs on one period)


GEO = ("clamp_x", "clamp_y", "clamp_xy", "needle", "tiny", "culled")
RECS = ("rec_zero", "rec_colour", "rec_moments", "rec_negzero", "rec_culled")
COL = ("clamp3", "clamp1", "clamp0")
TIME = ("ts_equal", "near_cull")
RAWP = ("qnorm_small", "qnorm_big", "opac_pos", "opac_neg")

CASES = [
    # --- configurations -------------------------------------------------------------------------------------------------------
    Case("c3d_act", 257, 3, False, 3, 0, 16, need=GEO + RECS + COL, live="alternate"),                  # cov3_backward, 3D SH degree 3
    Case("c3d_raw_m9", 1000, 3, False, 2, 0, 9, raw=True, need=GEO + RECS + COL + RAWP),                # activations; 27-float rows (unaligned)
    Case("c3d_mod05", 65, 3, False, 1, 0, 4, mod=0.5, need=("culled",)),                                 # scale_modifier, (1,0,4)
    Case("dim4_act", 65, 4, False, 3, 2, 48, need=TIME + ("culled",), live="lastwave"),                  # Q6; both time blocks, Q1-Q3
    Case("dim4_raw_pv", 63, 4, False, 2, 1, 27, raw=True, pv=0.3, need=TIME + ("culled",)),              # (2,1,27): 81-float rows
    Case("rot4d_act", 257, 4, True, 3, 2, 48, mod=0.5, need=GEO + RECS + COL + TIME),                    # cov4 chain, Q5, Q7
    Case("rot4d_raw_pv_ana", 1000, 4, True, 3, 2, 48, raw=True, pv=0.3, analytic=True, need=GEO + RECS + COL + TIME + RAWP),
    Case("rot4d_raw_d1", 64, 4, True, 1, 0, 4, raw=True, need=TIME),                                     # (1,0,4), one full wave
    Case("rot4d_p1", 1, 4, True, 0, 0, 1, raw=True),                                                     # (0,0,1), one Gaussian
    Case("rot4d_sh3d", 65, 4, True, 3, 0, 16, force_sh_3d=True, need=TIME + ("culled",), live="none"),   # force_sh_3d; nobody live
    Case("rot4d_ana_dt1", 64, 4, True, 3, 1, 32, analytic=True, need=TIME),                              # analytic, one time block
    Case("precomp_cov", 257, 3, False, 1, 0, 4, precomp_cov=True, need=("clamp_x", "clamp_y", "culled") + RECS),
    Case("precomp_col", 257, 4, True, 0, 0, 0, raw=True, need=GEO + TIME + RAWP),                        # colors_precomp: no SH at all
    Case("m18_unaligned", 63, 4, True, 2, 1, 18, need=("culled",)),                                      # a second unaligned row length
    # --- live patterns of the SH wave compaction (rot_4d raw, M = 48) -----------------------------------------------------------
    Case("live_all", 257, 4, True, 3, 2, 48, raw=True, live="all", need=COL, seed=11),
    Case("live_none", 257, 4, True, 3, 2, 48, raw=True, live="none", seed=12),
    Case("live_alternate", 257, 4, True, 3, 2, 48, raw=True, live="alternate", seed=13),
    Case("live_64plus1", 257, 4, True, 3, 2, 48, raw=True, live="64plus1", seed=14),
    Case("live_lastwave", 257, 4, True, 3, 2, 48, raw=True, live="lastwave", seed=15),
    # --- modes ----------------------------------------------------------------------------------------------------------------
    Case("accumulate", 257, 4, True, 3, 2, 48, raw=True, mode="accumulate", need=RECS, seed=21),
    Case("noperview", 65, 4, True, 3, 2, 48, raw=True, mode="noperview", seed=22),
    Case("views2", 257, 4, True, 3, 2, 48, raw=True, views=2, need=RECS, seed=23),
    Case("views5", 65, 4, True, 3, 2, 48, raw=True, views=5, seed=24),
    Case("views2_c3d", 63, 3, False, 3, 0, 16, views=2, seed=25),
]
# P = 2^20 + 3 selects preprocess_bwd_kernel_w4 (launch_preprocess_bwd): rot_4d raw, D = 0, 512 x 512, one period of 4099 Gaussians
# repeated -- every element is compared, the float64 oracle runs on one period.  ~1024 entries per tile list.
LARGE = Case("large_w4", (1 << 20) + 3, 4, True, 0, 0, 1, raw=True, W=512, H=512, period=4099, seed=31)
BY_NAME = {c.name: c for c in CASES + [LARGE]}

DURATION = 4.0
TIMESTAMP = 2.0


def _world(cam, xv):
    """World points of view-space points xv [n,3] (float64) for the camera dict ``cam`` (row-vector convention: x_view = [x, 1] wv)."""
    wv = cam["world_view_transform"].numpy().astype(np.float64)
    return (xv - wv[3, :3]) @ np.linalg.inv(wv[:3, :3])


def _cov_t(scl, q, qr):
    """Sigma[3][3] of the 4D covariance (forward.cu:279-332) in float64: scl [n,4] the modified scales, q / qr unit quaternions."""
    a_, b_, c_, d_ = q.T
    p_, q_, r_, s_ = qr.T
    Ml = co.cols([[a_, b_, -c_, d_], [-b_, a_, d_, c_], [c_, -d_, a_, b_], [-d_, -c_, -b_, a_]])
    Mr = co.cols([[p_, q_, -r_, -s_], [-q_, p_, s_, -r_], [r_, -s_, p_, -q_], [s_, r_, q_, p_]])
    Mm = co.mul(Mr, Ml) * scl[:, None, :]
    return co.mul(co.tr(Mm), Mm)[:, 3, 3]


def build(case):
    """-> dict(scene: synth-style scene dict of CPU tensors of view 0 (+ "raw"), views: per-view overrides (timestamp), acc: per-view
    [P,12] float32 records, prefill: {tensor: float32 array} or None)."""
    c = case
    Pn = c.period if c.period else c.P
    rng = np.random.default_rng(1000 + c.seed + 7 * c.P)
    cam = synth.camera_for("rig0", c.W, c.H)
    tanx, tany = cam["tanfovx"], cam["tanfovy"]
    # generic Gaussians: inside the image, moderate footprint
    u, v = rng.uniform(-0.85, 0.85, Pn), rng.uniform(-0.85, 0.85, Pn)
    z = rng.uniform(2.5, 6.0, Pn)
    s0 = 0.05 if not c.period else 0.004
    scales = s0 * np.exp(0.3 * rng.standard_normal((Pn, 3)))
    sct_act = 0.5 * np.exp(0.3 * rng.standard_normal(Pn))                 # scales_t (rot_4d: a std; else the variance itself)
    ts = TIMESTAMP + c.mod * rng.uniform(-0.3, 0.3, Pn)                   # (well inside the temporal cull: the culled ones are planted)
    unit = lambda q: q / np.linalg.norm(q, axis=1, keepdims=True)   # noqa: E731
    # rot_4d: a general left factor turns the temporal axis into space and cov_t collapses: both factors stay within reach of identity
    rot = unit(np.array([1.0, 0, 0, 0]) + 0.3 * rng.standard_normal((Pn, 4))) if c.rot_4d else unit(rng.standard_normal((Pn, 4)))
    rot_r = unit(np.array([1.0, 0, 0, 0]) + 0.3 * rng.standard_normal((Pn, 4)))
    qnorm, qnorm_r = rng.uniform(0.5, 2.0, Pn), rng.uniform(0.5, 2.0, Pn)
    opa_raw = rng.standard_normal(Pn)
    M = c.M
    shs = 0.2 * rng.standard_normal((Pn, max(M, 1), 3))
    shs[:, 0, :] = rng.uniform(0.2, 1.0, (Pn, 3))                         # DC positive: nothing clamped unless planted
    ident = np.array([1.0, 0.0, 0.0, 0.0])

    # populations by construction: 8 each, from the end of the index range so that index 0.. stay generic (P < 257: only time / culled)
    n = 8 if Pn >= 257 else (4 if Pn >= 63 else 0)
    cur = [Pn]

    def take(k=n):
        cur[0] -= k
        return np.arange(cur[0], cur[0] + k)

    culled_idx = []
    big = Pn >= 257 and not c.period   # (the large case keeps its tile lists short: no image-sized splats)
    if big:
        for name, uu, vv in (("clamp_x", 1.5, 0.3), ("clamp_y", -0.2, -1.5), ("clamp_xy", -1.45, 1.5)):
            i = take()
            u[i], v[i], z[i] = uu * np.where(np.arange(n) % 2 == 0, 1.0, -1.0), vv, 4.0
            scales[i] = 0.7 / c.mod * np.exp(0.1 * rng.standard_normal((n, 3)))
            if c.rot_4d:   # (a splat this large: keep the 4D rotation and dt small, or the mean shift carries it back inside the clamp)
                rot[i], rot_r[i] = unit(ident + 0.02 * rng.standard_normal((n, 4))), unit(ident + 0.02 * rng.standard_normal((n, 4)))
                ts[i] = TIMESTAMP + rng.uniform(-0.01, 0.01, n)
        i = take()   # needles: 1:100 on screen -- sigma_long ~ 58 px against the low-pass's 0.55 px
        u[i], v[i], z[i] = rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n), 5.0
        scales[i] = np.array([0.003, 0.003, 0.003])
        scales[i, rng.integers(0, 2, n)] = 5.6 / c.mod
        # (rot_4d: a 4D rotation puts part of the long axis into time and the conditioning shortens the needle unless the temporal
        # extent dwarfs it; no exactly axis-aligned needle: a zero covariance entry has no one-ulp neighbour to be perturbed to)
        rot[i] = unit(ident + 0.05 * rng.standard_normal((n, 4)))
        rot_r[i] = unit(ident + 0.02 * rng.standard_normal((n, 4)))
        sct_act[i] = 60.0 / c.mod
        ts[i] = TIMESTAMP + rng.uniform(-0.05, 0.05, n)
        i = take()
        scales[i] = 1e-4 / c.mod                                           # tiny
        if c.raw:
            i = take(); qnorm[i] = 1e-3
            i = take(); qnorm_r[i] = 1e-3; qnorm[i] = 1e3
            i = take(); qnorm[i] = 1e3; qnorm_r[i] = 1e3
            i = take(); opa_raw[i] = 15.0
            i = take(); opa_raw[i] = -15.0
        if M > 0:
            i = take(); shs[i, 0, :] = -12.0                               # all three channels clamped
            i = take(); shs[i, 0, 1] = -12.0                               # one channel clamped
    if n and c.dim == 4:
        i = take(); ts[i] = TIMESTAMP                                      # ts == timestamp exactly
        i = take()                                                         # marginal 0.0525: within 10 % above the cull
        u[i], v[i] = rng.uniform(-0.4, 0.4, len(i)), rng.uniform(-0.4, 0.4, len(i))   # (rot_4d: the mean shift at this dt stays on screen)
        var = _cov_t(c.mod * np.concatenate([scales[i], sct_act[i, None]], axis=1), rot[i], rot_r[i]) if c.rot_4d else c.mod * sct_act[i]
        if c.pv > 0:
            var = var + c.pv
        ts[i] = TIMESTAMP + np.where(np.arange(len(i)) % 2 == 0, 1, -1) * np.sqrt(-2.0 * var * math.log(0.0525))
        i = take(); ts[i] = TIMESTAMP + 3.9                                # culled by the marginal
        culled_idx.extend(i)
    if n:
        i = take(); z[i] = 0.1                                             # culled: behind the near plane (0.2)
        culled_idx.extend(i)
    assert cur[0] >= Pn // 3, "the populations leave no generic Gaussians"

    xyz = _world(cam, np.stack([u * tanx * z, v * tany * z, z], axis=1))
    f = np.float32
    rep = (lambda a: np.resize(a, (c.P,) + a.shape[1:])) if c.period else (lambda a: a)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(rep(f(a))))   # noqa: E731
    sc = dict(cam)
    sc.update({"P": c.P, "W": c.W, "H": c.H, "M": M, "bg": torch.tensor([0.1, 0.2, 0.3]), "means3D": t(xyz),
               "sh_degree": c.D, "sh_degree_t": c.D_t, "timestamp": TIMESTAMP, "time_duration": DURATION, "rot_4d": c.rot_4d,
               "gaussian_dim": c.dim, "force_sh_3d": c.force_sh_3d, "scale_modifier": c.mod, "prefilter_var": c.pv,
               "analytic_sh_grad": c.analytic, "raw": c.raw, "flow_2d": t(0.5 * rng.standard_normal((Pn, 2)))})
    sc["opacities"] = t(opa_raw[:, None] if c.raw else 1.0 / (1.0 + np.exp(-opa_raw[:, None])))
    if M > 0:
        sc["shs"] = t(shs)
    else:
        sc["colors_precomp"] = t(rng.uniform(0.0, 1.0, (Pn, 3)))
    if c.precomp_cov:
        R = np.transpose(co.quat_to_R(rot), (0, 2, 1))                    # [P, row, col]
        S = R @ (scales[:, :, None] ** 2 * np.transpose(R, (0, 2, 1)))
        sc["cov3D_precomp"] = t(np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], axis=1))
    else:
        sc["scales"] = t(np.log(scales) if c.raw else scales)
        sc["rotations"] = t(rot * qnorm[:, None] if c.raw else rot)
    if c.dim == 4:
        sc["ts"] = t(ts[:, None])
        sc["scales_t"] = t(np.log(sct_act[:, None]) if c.raw else sct_act[:, None])
    if c.rot_4d:
        sc["rotations_r"] = t(rot_r * qnorm_r[:, None] if c.raw else rot_r)

    # ---- accumulator records, per view ----
    accs, views = [], []
    for vw in range(c.views):
        a = rng.standard_normal((Pn, 12))
        idx = np.arange(Pn)
        a[idx % 16 == 3] = 0.0                                             # all zero
        a[np.ix_(idx % 16 == 5, np.arange(3, 12))] = 0.0                   # colour words only
        a[np.ix_(idx % 16 == 7, np.arange(0, 3))] = 0.0                    # moments (and the rest) only
        one = np.nonzero(idx % 16 == 9)[0]
        a[one, (one // 16) % 12] = -0.0                                    # one -0.0 word
        a[idx % 16 == 11] = -0.0                                           # a record of them
        a[culled_idx] = rng.standard_normal((len(culled_idx), 12))         # culled Gaussians: non-zero records
        dead = np.zeros(Pn, bool)
        if c.live == "none":
            dead[:] = True
        elif c.live == "alternate":
            dead[(idx + vw) % 2 == 0] = True
        elif c.live == "64plus1":
            dead[:] = True
            dead[64:129] = False                                           # the second wave's 64 and one more
            a[64:129, 0] = rng.uniform(0.5, 1.0, 65)
        elif c.live == "lastwave":
            dead[:64 * ((Pn - 1) // 64)] = True
        a[np.ix_(dead, np.arange(0, 3))] = 0.0
        accs.append(np.ascontiguousarray(rep(f(a))))
        views.append({"timestamp": TIMESTAMP + 0.11 * vw})
    prefill = None
    if c.mode == "accumulate":
        shapes = {"dL_dopacity": (1,), "dL_dmean3D": (3,), "dL_dts": (1,), "dL_dscale": (3,), "dL_dscale_t": (1,), "dL_drot": (4,),
                  "dL_drot_r": (4,)}
        prefill = {k: f(rng.standard_normal((c.P,) + s)) for k, s in shapes.items()}
    return {"case": c, "scene": sc, "views": views, "acc": accs, "prefill": prefill}


def view_scene(built, v):
    return dict(built["scene"], **built["views"][v])


def activated(scene):
    """The scene with fp32-activated parameters (numpy float32 exp / sigmoid / normalisation): what the port, which has no raw mode,
    is given for a raw case."""
    if not scene.get("raw"):
        return scene
    s = dict(scene)
    for k in ("scales", "scales_t"):
        if s.get(k) is not None:
            s[k] = torch.exp(s[k])
    for k in ("rotations", "rotations_r"):
        if s.get(k) is not None:
            s[k] = s[k] / s[k].norm(dim=1, keepdim=True).clamp_min(1e-12)
    s["opacities"] = torch.sigmoid(s["opacities"])
    s["raw"] = False
    return s


def oracle_inputs(scene, period=0):
    """tests/chain_oracle.chain's ``inp`` of a scene dict: numpy arrays, every scalar as the fp32 value the C ABI receives."""
    n = period if period else int(scene["means3D"].shape[0])
    g = lambda k: None if scene.get(k) is None else scene[k].numpy()[:n]   # noqa: E731
    r = lambda k: None if g(k) is None else g(k).reshape(n)   # noqa: E731
    return {"P": n, "D": int(scene["sh_degree"]), "D_t": int(scene["sh_degree_t"]), "M": int(scene["M"]), "W": int(scene["W"]),
            "H": int(scene["H"]), "shs": g("shs"), "opacities": r("opacities"), "ts": r("ts"), "scales": g("scales"),
            "scales_t": r("scales_t"), "rotations": g("rotations"), "rotations_r": g("rotations_r"), "cov3D_precomp": g("cov3D_precomp"),
            "viewmatrix": scene["world_view_transform"].numpy().reshape(16), "projmatrix": scene["full_proj_transform"].numpy().reshape(16),
            "campos": scene["camera_center"].numpy(), "tan_fovx": co.f32(scene["tanfovx"]), "tan_fovy": co.f32(scene["tanfovy"]),
            "timestamp": co.f32(scene["timestamp"]), "time_duration": co.f32(scene["time_duration"]),
            "scale_modifier": co.f32(scene["scale_modifier"]), "prefilter_var": co.f32(scene["prefilter_var"]),
            "rot_4d": bool(scene["rot_4d"]), "gaussian_dim": int(scene["gaussian_dim"]), "force_sh_3d": bool(scene["force_sh_3d"]),
            "raw": bool(scene.get("raw")), "analytic_sh": bool(scene.get("analytic_sh_grad"))}


def records_of(fwd, period=0):
    """``rec`` of tests/chain_oracle.chain from a forward's outputs (the port's dict or tests/util.collect_forward's)."""
    n = period if period else fwd["radii"].shape[0]
    return {k: np.asarray(fwd[k])[:n] for k in ("radii", "out_means3D", "cov3D", "conic_opacity", "clamped")}


def populations(inp, rec, acc):
    """How many Gaussians of each population the forward's own radii and records show (float64 host arithmetic)."""
    P = inp["P"]
    vis = rec["radii"] > 0
    m = rec["out_means3D"].astype(np.float64)
    vm = inp["viewmatrix"].astype(np.float64)
    with np.errstate(all="ignore"):
        tz = vm[2] * m[:, 0] + vm[6] * m[:, 1] + vm[10] * m[:, 2] + vm[14]
        bx = np.abs((vm[0] * m[:, 0] + vm[4] * m[:, 1] + vm[8] * m[:, 2] + vm[12]) / tz) > co.CLAMP * inp["tan_fovx"]
        by = np.abs((vm[1] * m[:, 0] + vm[5] * m[:, 1] + vm[9] * m[:, 2] + vm[13]) / tz) > co.CLAMP * inp["tan_fovy"]
        a, b, c = (rec["conic_opacity"][:, i].astype(np.float64) for i in range(3))
        mid, det = 0.5 * (a + c), a * c - b * b
        root = np.sqrt(np.maximum(mid * mid - det, 0.0))
        aniso = np.sqrt((mid + root) / np.maximum(mid - root, 1e-300))
    out = {"culled": int((~vis).sum()), "clamp_x": int((vis & bx & ~by).sum()), "clamp_y": int((vis & by & ~bx).sum()),
           "clamp_xy": int((vis & bx & by).sum()), "needle": int((vis & (aniso >= 100.0)).sum())}
    raw = inp["raw"]
    if inp["scales"] is not None:
        s = np.exp(inp["scales"].astype(np.float64)) if raw else inp["scales"].astype(np.float64)
        out["tiny"] = int((vis & (s.max(1) * inp["scale_modifier"] <= 1.01e-4)).sum())
        qn = np.linalg.norm(inp["rotations"].astype(np.float64), axis=1)
        out["qnorm_small"], out["qnorm_big"] = int((vis & (qn < 2e-3)).sum()), int((vis & (qn > 5e2)).sum())
    out["opac_pos"], out["opac_neg"] = int((vis & (inp["opacities"] == 15.0)).sum()), int((vis & (inp["opacities"] == -15.0)).sum())
    if inp["ts"] is not None:
        out["ts_equal"] = int((vis & (inp["ts"] == np.float32(inp["timestamp"]))).sum())
        dt = inp["timestamp"] - inp["ts"].astype(np.float64)
        sct = np.exp(inp["scales_t"].astype(np.float64)) if raw else inp["scales_t"].astype(np.float64)
        if inp["rot_4d"]:
            sc = np.exp(inp["scales"].astype(np.float64)) if raw else inp["scales"].astype(np.float64)
            q, _ = co.normalize(inp["rotations"].astype(np.float64)) if raw else (inp["rotations"].astype(np.float64), None)
            qr, _ = co.normalize(inp["rotations_r"].astype(np.float64)) if raw else (inp["rotations_r"].astype(np.float64), None)
            scl = inp["scale_modifier"] * np.concatenate([sc, sct[:, None]], axis=1)
            var = _cov_t(scl, q, qr)
        else:
            var = sct * inp["scale_modifier"]
        if inp["prefilter_var"] > 0:
            var = var + inp["prefilter_var"]
        marg = np.exp(-0.5 * dt * dt / var)
        out["near_cull"] = int((vis & (marg > 0.05) & (marg <= 0.055)).sum())
    cl = rec["clamped"].reshape(P, 3).astype(bool).sum(1)
    if inp["shs"] is not None:
        out["clamp3"], out["clamp1"], out["clamp0"] = int((vis & (cl == 3)).sum()), int((vis & (cl == 1)).sum()), int((vis & (cl == 0)).sum())
    a = np.asarray(acc)[:P]
    nz = a.view(np.uint32) != 0
    col, rest = (a[:, 0:3] != 0).any(1), (a[:, 6:11] != 0).any(1)
    out["rec_zero"] = int((vis & ~nz.any(1)).sum())
    out["rec_colour"] = int((vis & col & ~rest).sum())
    out["rec_moments"] = int((vis & ~col & rest).sum())
    out["rec_negzero"] = int((vis & (np.signbit(a) & (a == 0)).any(1)).sum())
    out["rec_culled"] = int((~vis & nz.any(1)).sum())
    return out


def assert_populations(case, inp, rec, acc):
    got = populations(inp, rec, acc)
    n = 8 if case.P >= 257 else 4
    short = {k: got.get(k, 0) for k in case.need if got.get(k, 0) < n}
    assert not short, "%s: populations short of %d Gaussians: %r (all: %r)" % (case.name, n, short, got)
    live = (rec["radii"] > 0) & (np.where(rec["clamped"].reshape(-1, 3) != 0, 0.0, np.asarray(acc)[:inp["P"], 0:3]) != 0).any(1)
    nl = int(live.sum())
    if inp["shs"] is not None:
        if case.live == "none":
            assert nl == 0, (case.name, nl)
        elif case.live == "64plus1":
            assert nl == 65 and live[64:129].all(), (case.name, nl)
        elif case.live == "lastwave":
            assert nl > 0 and not live[:64 * ((inp["P"] - 1) // 64)].any(), (case.name, nl)
        elif case.P >= 63:
            assert nl >= inp["P"] // 8, (case.name, nl)
    return got


# ---------------------------------------------------------------------------------------------------------------------------------
# Expected values and bars of a whole case (views, accumulation) from the per-view float64 results
# ---------------------------------------------------------------------------------------------------------------------------------
def expected(case, per_view, radii, prefill):
    """``per_view``: [(f64 outputs, sens)] of every view in order.  -> (expected {tensor: f64}, core bar {tensor: f64}) of what the
    LAST call leaves: the per-view outputs of the last view; the parameter gradients view 0 writes (or adds to the prefill) and the
    later views add to (chain_oracle.accumulate: fp32 additions, each as accurate as its addends at best: one ulp of the larger
    addend joins the bar per addition); dL_dsh = the views' rows summed in view order by the flush."""
    f64, sens = per_view[-1]
    exp = {k: v for k, v in f64.items()}
    core = {k: co.core_bar(f64[k], sens[k]) for k in f64}
    tot, bar = None, None
    for v, (fv, sv) in enumerate(per_view):
        vis = (radii[v] > 0)
        part, pbar = {}, {}
        for k in co.PARAM_GRADS + ("dL_dsh",):
            m = vis.reshape((-1,) + (1,) * (fv[k].ndim - 1)) if k != "dL_dsh" else True
            cur = fv[k]
            cb = co.core_bar(fv[k], sv[k])
            if v == 0 and (prefill is None or k == "dL_dsh"):
                part[k], pbar[k] = cur, cb
                continue
            if v == 0:
                base, bb = prefill[k].astype(np.float64).reshape(cur.shape), co.ulp32(prefill[k].astype(np.float64).reshape(cur.shape))
            else:
                base, bb = tot[k], bar[k]
            add = np.where(m, cur, 0.0) if k != "dL_dsh" else cur
            part[k] = base + add
            pbar[k] = bb + np.where(m, cb, 0.0) + np.where(m, co.ulp32(np.maximum(np.abs(base), np.abs(add))), 0.0)
        tot, bar = part, pbar
    exp.update(tot)
    core.update(bar)
    return exp, core


def worst(got, exp, core):
    """max over the elements of |got - exp| / core, and where."""
    d = np.nan_to_num(np.abs(np.asarray(got, np.float64).reshape(exp.shape) - exp), nan=np.inf) / core
    if d.size == 0:
        return 0.0, ()
    i = np.unravel_index(int(np.argmax(d)), d.shape)
    return float(d[i]), i


def tile(a, P, period):
    """The period's rows repeated to P rows (the large case)."""
    return np.resize(a, (P,) + a.shape[1:]) if period else a


def oracle_case(built, fwds):
    """The float64 side of a whole case from the forwards' records (one per view): -> (expected, core bar, per-view (f64, sens),
    per-view populations); P rows each (the large case: one period evaluated, then repeated)."""
    c = built["case"]
    per_view, radii, pops = [], [], []
    for v in range(c.views):
        inp = oracle_inputs(view_scene(built, v), c.period)
        rec = records_of(fwds[v], c.period)
        acc = built["acc"][v][:inp["P"]]
        pops.append(assert_populations(c, inp, rec, acc) if v == 0 else None)
        f64, sens = co.sensitivity(inp, rec, acc, seed=v)
        if c.period:
            f64 = {k: tile(a, c.P, c.period) for k, a in f64.items()}
            sens = {k: tile(a, c.P, c.period) for k, a in sens.items()}
        per_view.append((f64, sens))
        radii.append(np.asarray(fwds[v]["radii"]))
    exp, core = expected(c, per_view, radii, built["prefill"])
    return exp, core, per_view, pops
