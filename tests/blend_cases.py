"""Cases of the blend tests (tests/test_blend_oracle_host.py on the CPU, tests/test_gpu_blend.py on the GPU): seeded, tiny, built by
construction from precomputed covariances and colours under the unrotated on-axis camera, so that a splat lands on the pixel, with the
footprint, opacity and depth rank the case wants.  A case is a scene, the forward options it is run with (``modes``), and the
POPULATIONS it exists for (``need``); both tests count them from THIS forward's lists, records and n_contrib (``populations``, which
replays the kernels' survivor compaction per 8x8 block on the CPU) and fail when one is missing.

Populations (per wave = 8x8 block; counts):
  pair_both / pair_first / pair_second / pair_neither   queue pairs of the backward by which entries have active pixels
  drain_N (N = 1..15), drain_kinds     groups of ACC_GROUP entries drained with staging mask N; how many of the fifteen masks occur
                                       (a need may ask for a count: "drain_kinds>=12")
  tail_group                           a group that ends a chunk with npairs odd
  odd_chunk / one_survivor / empty_between   a chunk with an odd survivor count (the inert half), with exactly one survivor, with none between
                                       two chunks that have some
  deep_N (N = 1, 63, 64, 65, 127, 128, 129), deep_gt256   a block whose deepest contributor is list position N (1-based)
  list_past_deep                       a block whose list goes on >= 64 entries past its deepest contributor
  fwd_break_inside / fwd_break_between the forward's done == ~0 break before the last pair of a chunk / with further chunks left
  range_unaligned                      non-empty tiles whose range.x is no multiple of 64
  partial_block                        blocks partly outside the image;  returned_block: blocks of the grid entirely outside
  atomics48                            a record that 48 blocks add to;  one_block_record: records exactly one block adds to
  clamp99                              (pixel, entry) contributions at the 0.99 clamp
  alpha_low                            contributions with alpha in [1.2/255, 2/255]
  T_near_min / T_near_one              pixels with contributors and final_T < 2e-4 / > 0.9
  bg_live                              pixels with contributors, final_T > 0.01 and bg != 0
  listed_unaccepted / unlisted         Gaussians in some list that no pixel accepts / in no list
"""
import os
import sys
from typing import NamedTuple

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import blend_oracle as bo  # noqa: E402
import chain_cases as cc  # noqa: E402
from fdgs import synth  # noqa: E402

# K per class = 4 * r_ref32 rounded up to a power of two: r_ref32 = the worst |ref32 - f64| / unit of
# blend_oracle's fp32 restatement of the reference over every case and variant, measured by
# tests/test_blend_oracle_host.py::test_ref32_pinned_and_K, which fails if 4 * r_ref32 leaves (K / 2, K] by more than K_TOLERANCE.
# The HIP kernels play no part in them.
K = {"colour": 2.0, "depth": 2.0, "flow": 2.0, "T": 2.0, "w0_2": 1.0, "w3": 1.0, "w4_5": 0.5, "w6_7": 0.5, "w8_10": 0.5, "w11": 0.5}
K_TOLERANCE = 0.10
FLAG_CAP = 0.005
ACC_GROUP = 4

VARIANTS = {  # upstream images given: (colour, depth, alpha, flow)
    "colour": (True, False, False, False), "depth": (False, True, False, False), "alpha": (False, False, True, False),
    "flow": (False, False, False, True), "all": (True, True, True, True), "nocolour": (False, True, True, True),
}
MODES = {"default": dict(tile_cull=False, sparse=False), "tile_cull": dict(tile_cull=True, sparse=False),
         "sparse": dict(tile_cull=True, sparse=True)}


class Case(NamedTuple):
    name: str
    W: int
    H: int
    gen: str                     # the generator below
    bg: tuple = (0.0, 0.0, 0.0)
    flow: bool = True            # the scene has flow_2d (FLOW = true)
    modes: tuple = ("default",)
    need: tuple = ()
    seed: int = 0


PAIRS = ("pair_both", "pair_first", "pair_second", "pair_neither")
BG = (0.3, 0.6, 0.9)
CASES = [
    # every staging mask 1..15 of a drained group, by construction: one block, one chunk, groups of four survivors back to front
    Case("masks_8x8", 8, 8, "masks", bg=BG, need=PAIRS + tuple("drain_%d" % m for m in range(1, 16)) + ("drain_kinds>=15",), seed=12),
    Case("one_block_8x8", 8, 8, "few", need=("returned_block", "T_near_one"), seed=1),                       # one live block, three returned
    Case("dense_16x16", 16, 16, "dense", bg=BG, need=PAIRS[0:3] + ("tail_group", "odd_chunk", "deep_gt256", "alpha_low", "bg_live"), seed=2),
    Case("dense_16x16_noflow", 16, 16, "dense", flow=False, need=PAIRS[0:3] + ("tail_group", "odd_chunk"), seed=3),   # FLOW = false
    Case("ladder_32x16", 32, 16, "ladder", bg=BG, need=tuple("deep_%d" % d for d in (1, 63, 64, 65, 127, 128, 129)) + (
        "deep_gt256", "one_survivor", "empty_between", "listed_unaccepted", "unlisted"), seed=4),
    Case("half_dark_32x32", 32, 32, "opaque", need=PAIRS + ("drain_kinds>=12", "T_near_min", "range_unaligned"), modes=("default", "tile_cull", "sparse"), seed=5),
    Case("dark_32x32", 32, 32, "dark", need=("list_past_deep", "fwd_break_inside", "fwd_break_between", "T_near_min"), seed=11),
    Case("cover_64x48", 64, 48, "cover", bg=BG, need=("atomics48", "one_block_record", "bg_live", "range_unaligned"),
         modes=("default", "tile_cull", "sparse"), seed=6),
    Case("clamp_16x16", 16, 16, "clamp", bg=BG, need=("clamp99",), seed=7),
    Case("ragged_17x9", 17, 9, "random", bg=BG, need=("partial_block", "pair_both"), seed=8),
    Case("ragged_23x31", 23, 31, "random", need=("partial_block", "range_unaligned", "pair_both"), seed=9),
    Case("ragged_40x24", 40, 24, "random", bg=BG, flow=False, need=("range_unaligned", "pair_both", "bg_live"),
         modes=("default", "tile_cull", "sparse"), seed=10),
]
BY_NAME = {c.name: c for c in CASES}


# ---------------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------------
def _splats(case, rng):
    """-> x, y (pixel), sigma (pixels, before the 0.3 low-pass), opacity -- in depth order, front first."""
    W, H = case.W, case.H
    col = lambda *a: np.concatenate([np.atleast_1d(np.asarray(v, np.float64)) for v in a])   # noqa: E731
    if case.gen == "few":
        return col(2.3, 5.6, 4.1), col(3.2, 1.7, 6.4), col(1.2, 0.8, 2.0), col(0.3, 0.5, 0.2)
    if case.gen == "masks":
        # back to front, group by group, entry b of the group with mask m is a real splat if bit b of m is set, else a survivor nobody accepts:
        # centre inside the block (the cull keeps it: opacity 0.00391 >= 0.0039) and alpha <= 0.00391 < 1/255 on every pixel.  The deepest
        # entry must be real (it is the block's last contributor): the group with mask 15 goes first.
        real = np.array([bool((m >> b) & 1) for m in [15] + list(range(1, 15)) for b in range(4)])[::-1]
        n = real.size
        return (np.where(real, rng.uniform(0.5, 6.5, n), 3.5), np.where(real, rng.uniform(0.5, 6.5, n), 3.5), np.where(real, rng.uniform(0.6, 1.2, n), 1.0),
                np.where(real, rng.uniform(0.08, 0.2, n), 0.00391))
    if case.gen == "dense":
        n = 300
        op = rng.uniform(0.02, 0.35, n)
        low = np.arange(n) % 7 == 3
        op[low] = rng.uniform(1.3, 1.9, low.sum()) / 255.0
        sg = np.where(low, 4.0, rng.uniform(0.5, 1.6, n))
        return rng.uniform(0.0, 15.0, n), rng.uniform(0.0, 15.0, n), sg, op
    if case.gen == "random":
        n = 120
        return rng.uniform(-2.0, W + 1.0, n), rng.uniform(-2.0, H + 1.0, n), rng.uniform(0.5, 3.0, n), rng.uniform(0.01, 0.7, n)
    if case.gen == "clamp":
        n = 24
        x, y = np.floor(rng.uniform(1, 15, n)) + 0.02, np.floor(rng.uniform(1, 15, n)) + 0.01
        return x, y, rng.uniform(0.6, 1.5, n), np.where(np.arange(n) % 2 == 0, 1.0, rng.uniform(0.2, 0.6, n))
    if case.gen == "dark":
        n = 160
        x, y = rng.uniform(0, W, n), rng.uniform(0, H, n)
        sg, op = rng.uniform(0.5, 2.0, n), rng.uniform(0.05, 0.6, n)
        x[:8], y[:8], sg[:8], op[:8] = rng.uniform(12, 20, 8), rng.uniform(12, 20, 8), 40.0, 0.93   # every pixel is finished by the fourth or fifth
        return x, y, sg, op
    if case.gen == "opaque":
        n = 300
        x, y = rng.uniform(0, W, n), rng.uniform(0, H, n)
        sg, op = rng.uniform(0.5, 2.0, n), rng.uniform(0.05, 0.6, n)
        front = np.arange(n) < 6                       # six wide splats in front: T falls below 1e-4 behind the fourth where they are dense
        x[front], y[front] = rng.uniform(8, 24, 6), rng.uniform(8, 24, 6)
        sg[front], op[front] = 14.0, 0.93
        return x, y, sg, op
    if case.gen == "cover":
        bx, by = np.meshgrid(np.arange(8), np.arange(6))
        cx, cy = 8.0 * bx.reshape(-1) + 3.4, 8.0 * by.reshape(-1) + 3.7
        n1 = cx.size
        x = col(cx, 31.3, cx)                      # one small splat per block, the cover splat, one more per block behind it
        y = col(cy, 23.6, cy + 0.5)
        sg = col(np.full(n1, 0.7), 40.0, np.full(n1, 0.6))
        op = col(np.full(n1, 0.4), 0.5, np.full(n1, 0.6))
        return x, y, sg, op
    if case.gen == "ladder":
        # tile 0 (x 0..15): blocks' deepest contributors at 1, 63, 64, 65; tile 1 (x 16..31): 127, 128, 129 and 260 behind four front splats
        # (list positions 1-4, one per block).  Fillers: opacity 0.003 < 1/255 -- listed, accepted by nobody, culled for every block.
        xs, ys, sg, op = [], [], [], []
        centre = {0: (3.4, 3.6), 1: (11.4, 3.6), 2: (3.4, 11.6), 3: (11.4, 11.6)}

        def real(tile, sub, o=0.5):
            xs.append(16 * tile + centre[sub][0]); ys.append(centre[sub][1]); sg.append(0.6); op.append(o)

        def fill(tile, count):
            xs.extend([16 * tile + 7.5] * count); ys.extend([7.5] * count); sg.extend([0.5] * count); op.extend([0.003] * count)

        # the two tiles' lists interleave in depth, which does not matter: a list position is a rank inside the tile's own list
        real(0, 0); fill(0, 61); real(0, 1); real(0, 2); real(0, 3); fill(0, 20)
        for s in range(4):
            real(1, s, 0.3)
        fill(1, 122); real(1, 0); real(1, 1); real(1, 2); fill(1, 130); real(1, 3); fill(1, 10)
        return col(xs), col(ys), col(sg), col(op)
    raise ValueError(case.gen)


def build(case):
    """-> scene dict of CPU tensors (tests/util.native_args_fwd's keys).  Gaussian i is the i-th in depth; two extra Gaussians end the
    arrays: one far outside the image and one behind the camera (in no list)."""
    rng = np.random.default_rng(4000 + case.seed)
    W, H = case.W, case.H
    cam = synth.camera_for("axis", W, H)
    x, y, sg, op = _splats(case, rng)
    x, y, sg, op = (np.concatenate([a, b]) for a, b in ((x, [5.0 * W + 40.0, 0.5 * W]), (y, [0.5 * H, 0.5 * H]), (sg, [0.5, 1.0]), (op, [0.5, 0.5])))
    n = x.size
    z = 3.0 + 2.0 * np.arange(n) / max(n, 1)              # depth rank = index
    z[-1] = -1.0                                           # behind the camera
    tanx, tany = cam["tanfovx"], cam["tanfovy"]
    u, v = (2.0 * x + 1.0) / W - 1.0, (2.0 * y + 1.0) / H - 1.0
    xyz = cc._world(cam, np.stack([u * tanx * z, v * tany * z, z], axis=1))
    s3 = sg * np.abs(z) / (W / (2.0 * tanx))               # isotropic: sigma_px = f sigma / z (the Jacobian's skew off axis is part of the case)
    cov = np.zeros((n, 6))
    cov[:, 0] = cov[:, 3] = cov[:, 5] = s3 * s3
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32)))   # noqa: E731
    sc = dict(cam)
    sc.update({"P": n, "W": W, "H": H, "M": 0, "bg": torch.tensor(case.bg, dtype=torch.float32), "means3D": t(xyz), "sh_degree": 0,
               "sh_degree_t": 0, "timestamp": 0.0, "time_duration": 1.0, "rot_4d": False, "gaussian_dim": 3, "force_sh_3d": False,
               "scale_modifier": 1.0, "prefilter_var": -1.0, "opacities": t(op[:, None]), "cov3D_precomp": t(cov),
               "colors_precomp": t(rng.uniform(0.05, 1.0, (n, 3)))})
    if case.flow:
        sc["flow_2d"] = t(rng.standard_normal((n, 2)))
    return sc


def upstream(case, variant, seed=0):
    """{grad_color, grad_depth, grad_alpha, grad_flow}: CPU float32 tensors or None, by VARIANTS."""
    g = synth.make_upstream_grads(case.W, case.H, seed=11 + seed, scale=1.0)
    use = VARIANTS[variant]
    return {k: (g[k] if u else None) for k, u in zip(("grad_color", "grad_depth", "grad_alpha", "grad_flow"), use)}


def mask_upstream(up, flagged):
    """The upstream images with exact zeros on the flagged pixels."""
    keep = torch.from_numpy(~np.asarray(flagged, bool))
    return {k: (None if a is None else (a * keep[None]).contiguous()) for k, a in up.items()}


# ---------------------------------------------------------------------------------------------------------------------------------
# populations: the kernels' survivor compaction replayed per 8x8 block
# ---------------------------------------------------------------------------------------------------------------------------------
def block_reaches(a, rx0, rx1, ry0, ry1):
    """blend_common.h's block cull in numpy float32 on rows (x, y, A, B, C, opacity).  A survivor set for counting populations: an entry
    within rounding of the bound may differ from the device's, which moves a count by one, never a value."""
    f = np.float32
    x, y, A, B, Cc, op = (a[:, i].astype(f) for i in range(6))
    with np.errstate(all="ignore"):
        convex = (A > 0) & (Cc > 0) & (A * Cc > f(1.00001) * (B * B))
        dx0, dx1, dy0, dy1 = f(rx0) - x, f(rx1) - x, f(ry0) - y, f(ry1) - y
        xin, yin = (dx0 <= 0) & (dx1 >= 0), (dy0 <= 0) & (dy1 >= 0)
        tau = np.log(f(255.0) * op) + f(0.05)
        ex, ey = np.where(dx0 > 0, dx0, dx1), np.where(dy0 > 0, dy0, dy1)
        dyv = np.clip(-B * ex / Cc, dy0, dy1)
        qv = f(0.5) * (A * ex * ex + Cc * dyv * dyv) + B * ex * dyv
        dxh = np.clip(-B * ey / A, dx0, dx1)
        qh = f(0.5) * (A * dxh * dxh + Cc * ey * ey) + B * dxh * ey
        qmin = np.minimum(np.where(xin, f(3e38), qv), np.where(yin, f(3e38), qh))
        reach = np.where(~convex, True, np.where(xin & yin, True, qmin <= tau))
    return np.where(op >= f(0.0039), reach, False)


def populations(case, fwd, f64, trace=None):
    """``fwd``: this forward's records, lists, n_contrib, final_T (tests/util.collect_forward's keys); ``f64``: blend_oracle.forward on
    them.  -> {population: count}.  ``trace``: a dict that receives {Gaussian: [(tile, sub-block, chunk, path, staging mask of its group)]} for
    every queued entry with an active pixel -- path = "pair" (both entries of the queue pair active), "single0" / "single1" (it alone, as
    first / second entry of its pair)."""
    W, H = case.W, case.H
    gx, gy = (W + 15) // 16, (H + 15) // 16
    rec = np.concatenate([fwd["means2D"], fwd["conic_opacity"]], axis=1)
    rec64 = rec.astype(np.float64)
    rg = fwd["ranges"].astype(np.int64)
    pl = fwd["point_list"].astype(np.int64)
    nc = np.asarray(fwd["n_contrib"]).astype(np.int64)
    done_at = f64["done_at"]
    P = rec.shape[0]
    out = {k: 0 for k in PAIRS + ("tail_group", "odd_chunk", "one_survivor", "empty_between", "deep_gt256", "list_past_deep", "fwd_break_inside",
                                  "fwd_break_between", "partial_block", "returned_block", "clamp99", "alpha_low")}
    masks = set()
    touched = np.zeros(P, np.int64)
    for t in range(gx * gy):
        n = int(rg[t, 1] - rg[t, 0])
        ids = pl[rg[t, 0]:rg[t, 0] + n]
        for sub in range(4):
            bx0, by0 = (t % gx) * 16 + (sub & 1) * 8, (t // gx) * 16 + (sub >> 1) * 8
            if bx0 >= W or by0 >= H:
                out["returned_block"] += 1
                continue
            xs, ys = np.arange(bx0, min(bx0 + 8, W)), np.arange(by0, min(by0 + 8, H))
            if xs.size * ys.size < 64:
                out["partial_block"] += 1
            last = nc[np.ix_(ys, xs)].reshape(-1)
            wave_last = int(last.max())
            if wave_last:
                out["deep_%d" % wave_last] = out.get("deep_%d" % wave_last, 0) + 1
                out["deep_gt256"] += wave_last > 256
                out["list_past_deep"] += n - wave_last >= 64
            if n == 0:
                continue
            keep = block_reaches(rec[ids], xs[0], xs[-1], ys[0], ys[-1])
            X, Y = np.meshgrid(xs.astype(np.float64), ys.astype(np.float64))
            dx, dy = rec64[ids, 0:1] - X.reshape(1, -1), rec64[ids, 1:2] - Y.reshape(1, -1)
            power = -0.5 * (rec64[ids, 2:3] * dx * dx + rec64[ids, 4:5] * dy * dy) - rec64[ids, 3:4] * dx * dy
            alpha = np.minimum(bo.ALPHA_MAX, rec64[ids, 5:6] * np.exp(np.minimum(power, 50.0)))
            act = (np.arange(n)[:, None] < last[None, :]) & ~(power > 0) & ~(alpha < bo.ALPHA_MIN)        # [entry, pixel]
            anyact = act.any(1)
            touched[ids[anyact]] += 1
            out["clamp99"] += int((act & (alpha >= bo.ALPHA_MAX)).sum())
            out["alpha_low"] += int((act & (alpha >= 1.2 / 255) & (alpha <= 2.0 / 255)).sum())
            # forward: where the block's 64 pixels are all done
            d = done_at[np.ix_(ys, xs)].reshape(-1)
            if (d >= 0).all():
                at = int(d.max())
                s = np.nonzero(keep[(at // 64) * 64:min((at // 64 + 1) * 64, n)])[0] + (at // 64) * 64
                i = int(np.searchsorted(s, at))
                out["fwd_break_inside"] += (i >> 1) < ((s.size + 1) >> 1) - 1
                out["fwd_break_between"] += (at // 64 + 1) * 64 < n
            # backward: chunks from the deepest contributor's down, survivors back to front, pairs, groups
            counts = []
            for chunk in range((wave_last - 1) >> 6, -1, -1) if wave_last else ():
                pos = np.arange(min(chunk * 64 + 63, wave_last - 1), chunk * 64 - 1, -1)
                s = pos[keep[pos]]
                counts.append(s.size)
                out["odd_chunk"] += s.size & 1
                out["one_survivor"] += s.size == 1
                npairs = (s.size + 1) >> 1
                a = np.concatenate([anyact[s], [False]]) if s.size & 1 else anyact[s]
                grp, pend = 0, []
                for i in range(npairs):
                    a0, a1 = bool(a[2 * i]), bool(a[2 * i + 1])
                    out[PAIRS[0 if a0 and a1 else 1 if a0 else 2 if a1 else 3]] += 1
                    ip = i & (ACC_GROUP // 2 - 1)
                    grp |= (int(a0) | int(a1) << 1) << (2 * ip)
                    if a0:
                        pend.append((int(ids[s[2 * i]]), "pair" if a1 else "single0"))
                    if a1:
                        pend.append((int(ids[s[2 * i + 1]]), "pair" if a0 else "single1"))
                    if ip == ACC_GROUP // 2 - 1 or i == npairs - 1:
                        if grp:
                            masks.add(grp)
                        if trace is not None:
                            for gid, kind in pend:
                                trace.setdefault(gid, []).append((t, sub, chunk, kind, grp))
                        pend = []
                        if i == npairs - 1 and (npairs & 1):
                            out["tail_group"] += 1
                        grp = 0
            cs = np.asarray(counts)
            nz = np.nonzero(cs)[0]
            if nz.size >= 2:
                out["empty_between"] += int((cs[nz[0]:nz[-1]] == 0).sum())
    for m in masks:
        out["drain_%d" % m] = 1
    out["drain_kinds"] = len(masks)
    out["range_unaligned"] = int(((rg[:, 1] > rg[:, 0]) & (rg[:, 0] % 64 != 0)).sum())
    out["atomics48"] = int((touched == 48).sum())
    out["one_block_record"] = int((touched == 1).sum())
    listed = np.zeros(P, bool)
    for t in range(gx * gy):
        listed[pl[rg[t, 0]:rg[t, 1]]] = True
    out["listed_unaccepted"] = int((listed & (touched == 0)).sum())
    out["unlisted"] = int((~listed).sum())
    fT = np.asarray(fwd["final_T"], np.float64)
    out["T_near_min"] = int(((nc > 0) & (fT < 2e-4)).sum())
    out["T_near_one"] = int(((nc > 0) & (fT > 0.9)).sum())
    out["bg_live"] = int(((nc > 0) & (fT > 0.01)).sum()) if any(case.bg) else 0
    return out


def assert_populations(case, mode, pops):
    need = [k for k in case.need if not (mode == "sparse" and k == "range_unaligned")]   # sparse lists: ranges[t] = (t cap, ..), cap % 64 == 0
    short = [k for k in need if pops.get(k.split(">=")[0], 0) < int((k.split(">=") + ["1"])[1])]
    assert not short, "%s [%s]: populations missing: %r (all: %r)" % (case.name, mode, short, {k: v for k, v in pops.items() if v})


def assert_flag_cap(case, flagged):
    share = float(np.asarray(flagged).mean())
    assert share <= FLAG_CAP, "%s: %.3f %% of the pixels sit on a cliff (cap %.1f %%)" % (case.name, 100 * share, 100 * FLAG_CAP)
    return share

