"""The cases of the environment-map edge tests (tests/test_envmap_cases_host.py on the CPU, tests/test_gpu_envmap_edges.py on the
GPU): small images and maps chosen for the pixels, texels and tiles at which csrc/envmap.hip can go wrong, each tagged with the
populations it exists for.  The host test counts every tag from envmap_oracle.taps / tile_boxes; nothing here looks at a kernel.

Populations (``tags``):
  x0=-1, x0=ew-1     pixels whose tap hangs over the seam's left / right edge (corner columns -1 / ew: zero padding, no wrap)
  seam_tile          a 16 x 16 tile that holds both: its window box spans the full map width
  y0=-1, y0=eh-1     pixels whose tap hangs over the +z / -z pole row
  in1, in2           pixels with exactly one / two of their four corners in the map (three cannot be: see section 2 below)
  sub_tile           an image smaller than one tile;  ragged: a partial tile at the right or bottom edge;  multi_tile: > 1 tile
  window, direct     a tile on the LDS-window path / on the direct-atomics path
  win3072, win4096   a tile whose box is exactly 3072 texels (the largest window) / 4096 texels (direct)
  signed             a map with negative values (E_c is not |e_c|)
  T0, g0tile         T = 0 on a block of pixels; g = 0 on the whole first tile (its window stays zero: nothing is flushed)
  n0                 texels no pixel contributes to (exact +0, or the prior's bits under accumulate)
A tile none of whose pixels touches the map cannot occur: u and v lie in [0, 1], so ix lies in [-0.5, ew - 0.5], x0 in [-1, ew - 1],
and one of x0, x0 + 1 is always a map column (likewise rows); the host test asserts that no tile takes the path 'none'.
"""
import functools
import math

import numpy as np
import torch

import envmap_oracle as eo

R = 60.0

# delta, in texels: what the float64 coordinate may differ by between the kernel's formulation (cofactor inverse, device atan2) and
# the oracle's (linalg.inv): 10 x the largest |ix - ix'|, |iy - iy'| between envmap_oracle.kernel_texel_coords and texel_coords
# over all CASES, rounded up to a power of ten.  Measured on the CPU (test_delta_stands_on_the_measured_difference); never from a GPU.
MEASURED_F64_DIFF = (4.55e-13, 1.60e-14)     # (max |ix - ix'|, max |iy - iy'|), texels
DELTA = 1e-11

# eh of the two boundary cases (ew = 1024, pose 'polar': the +z pole inside tile 0, the seam through it): found by
# search_boundary_eh(), the smallest eh at which tile 0's box is 1024 x 3 = ENV_WIN (window) and 1024 x 4 (direct)
EH_3072, EH_4096 = 12, 20

POSES = {
    "rig2": "rig2",
    "seam": eo.POSES["seam"],
    "axis": dict(),                                              # looks at +z from (0, 0, -4): the pole in mid-image, the seam through it
    "nadir": dict(yaw=math.pi, shift=(0.15, -0.1, 8.5)),         # the mirror image: looks at -z
    "polar": dict(roll=0.004),                                   # axis with the seam at a shallow angle to a pixel row
}


def _c(name, pose, W, H, eh, ew, env="noise", up="plain", off=None, tags=()):
    return dict(name=name, pose=pose, W=W, H=H, eh=eh, ew=ew, env=env, up=up, off=off, tags=tuple(tags))


POLAR_OFF = (-7.7, -7.52)      # 32 x 32: the pole at pixel (8.3, 8.48), inside tile 0; the seam along row 8, crossing it in mid-tile

SHAPES = [(1, 1), (7, 1), (1, 7), (15, 16), (16, 16), (17, 19), (33, 31), (50, 36)]       # W x H
_SHAPE_TAGS = {
    (1, 1): ("sub_tile", "ragged"), (7, 1): ("sub_tile", "ragged"), (1, 7): ("sub_tile", "ragged"), (15, 16): ("sub_tile", "ragged"),
    (16, 16): (), (17, 19): ("ragged", "multi_tile"), (33, 31): ("ragged", "multi_tile"), (50, 36): ("ragged", "multi_tile"),
}
# what the two poses put under each image shape (counted by the host test): rig2's upper left corner looks past the seam from 15 x 16 on
_RIG2_TAGS = {(15, 16): ("x0=-1", "x0=ew-1", "seam_tile", "in2"), (16, 16): ("x0=-1", "x0=ew-1", "seam_tile", "in2"),
              (17, 19): ("x0=-1", "x0=ew-1", "seam_tile", "in2"), (33, 31): ("x0=-1", "x0=ew-1", "seam_tile", "in2"),
              (50, 36): ("x0=-1", "x0=ew-1", "seam_tile", "in2")}
_SEAM_TAGS = {(15, 16): ("x0=-1", "in2"), (16, 16): ("x0=ew-1", "in2"), (17, 19): ("x0=-1", "x0=ew-1", "in2"),
              (33, 31): ("x0=-1", "x0=ew-1", "seam_tile", "in2"), (50, 36): ("x0=-1", "x0=ew-1", "in2")}

CASES = []
# 1. image shapes on the two general poses; the 40 x 72 and 64 x 64 maps, in both forms, alternate over them
for _n, (_W, _H) in enumerate(SHAPES):
    for _pose, _extra in (("rig2", _RIG2_TAGS), ("seam", _SEAM_TAGS)):
        _eh, _ew = ((40, 72), (64, 64))[(_n + (_pose == "seam")) % 2]
        _env = ("noise", "signed")[(_n // 2 + (_pose == "seam")) % 2]
        CASES.append(_c("%s-%dx%d-map%dx%d-%s" % (_pose, _W, _H, _eh, _ew, _env), _pose, _W, _H, _eh, _ew, _env,
                        tags=("window", "n0") + _SHAPE_TAGS[(_W, _H)] + _extra.get((_W, _H), ()) + (("signed",) if _env == "signed" else ())))
# 2. tiny maps (eh x ew), both forms: every pixel has one or two corners in the map (three cannot be: in-map is a product of a column
#    test and a row test, so the count is 1, 2 or 4); the pole-facing pose (principal point nudged off the seam: with H odd the middle
#    pixel row of 'axis' lies on the seam itself) and the seam pose
for _eh, _ew, _t in ((1, 1, ("in1", "y0=-1", "y0=eh-1")), (1, 7, ("in1", "in2", "y0=-1", "y0=eh-1")), (7, 1, ("in2",)), (2, 3, ("in2",))):
    CASES.append(_c("seam-17x19-map%dx%d-noise" % (_eh, _ew), "seam", 17, 19, _eh, _ew, "noise",
                    tags=("x0=-1", "x0=ew-1", "ragged", "multi_tile", "window") + _t))
    CASES.append(_c("axis-17x19-map%dx%d-signed" % (_eh, _ew), "axis", 17, 19, _eh, _ew, "signed", off=(0.3, 0.2),
                    tags=("x0=-1", "x0=ew-1", "seam_tile", "y0=-1", "in1", "signed", "window")))
# 3. the poles: +z ('axis', 'polar') and -z ('nadir') in mid-image, the seam running out of them
CASES += [
    _c("axis-32x32-map40x72-noise", "axis", 32, 32, 40, 72, "noise", tags=("x0=-1", "x0=ew-1", "y0=-1", "in2", "multi_tile", "window", "n0")),
    _c("axis-33x31-map64x64-signed", "axis", 33, 31, 64, 64, "signed", off=(-4.2, -3.52),
       tags=("x0=-1", "x0=ew-1", "seam_tile", "y0=-1", "in2", "ragged", "signed", "n0")),
    _c("nadir-32x32-map40x72-signed", "nadir", 32, 32, 40, 72, "signed", tags=("x0=-1", "x0=ew-1", "y0=eh-1", "in2", "signed", "n0")),
    _c("nadir-33x31-map2x3-noise", "nadir", 33, 31, 2, 3, "noise", off=(-4.2, -3.7),
       tags=("x0=-1", "x0=ew-1", "seam_tile", "y0=eh-1", "in1", "in2", "ragged")),
]
# 4. the window boundary: tile 0 holds the pole and both sides of the seam, so its box is 1024 texels wide and 3 or 4 rows high
CASES += [
    _c("polar-32x32-map%dx1024-win3072" % EH_3072, "polar", 32, 32, EH_3072, 1024, "noise", off=POLAR_OFF,
       tags=("win3072", "window", "x0=-1", "x0=ew-1", "seam_tile", "y0=-1", "n0")),
    _c("polar-32x32-map%dx1024-win4096" % EH_4096, "polar", 32, 32, EH_4096, 1024, "signed", off=POLAR_OFF,
       tags=("win4096", "direct", "window", "x0=-1", "x0=ew-1", "seam_tile", "y0=-1", "n0", "signed")),
    _c("polar-32x32-map8x4096-wide", "polar", 32, 32, 8, 4096, "noise", off=POLAR_OFF, tags=("direct", "window", "y0=-1", "n0")),
]
# 5. degenerate upstream
CASES += [
    _c("rig2-33x31-map40x72-T0", "rig2", 33, 31, 40, 72, "signed", up="T0", tags=("T0", "multi_tile", "signed")),
    _c("rig2-33x31-map40x72-g0tile", "rig2", 33, 31, 40, 72, "noise", up="g0tile", tags=("g0tile", "multi_tile", "x0=-1", "x0=ew-1")),
    _c("polar-32x32-map8x4096-g0tile", "polar", 32, 32, 8, 4096, "signed", up="g0tile", off=POLAR_OFF, tags=("g0tile", "direct", "signed")),
]


def camera_of(case):
    """The case's camera (CPU float32 tensors; intrinsics as Python floats, rounded to float32 by the C ABI and by the oracle)."""
    from fdgs import synth
    pose = POSES[case["pose"]]
    kw = dict(synth.POSES[pose] if isinstance(pose, str) else pose)
    if case["off"] is not None:
        kw["principal_off"] = case["off"]
    return eo.camera(kw, case["W"], case["H"])


def populations(t, tb=None, up="plain", env="noise"):
    """{tag: count} of everything countable from the taps and the tile boxes."""
    tb = eo.tile_boxes(t) if tb is None else tb
    H, W, eh, ew = t["H"], t["W"], t["eh"], t["ew"]
    left, right = t["x0"] == -1, t["x0"] == ew - 1
    nin = t["inmap"].sum(0)
    n = np.zeros(eh * ew, np.int64)
    for k in range(4):
        np.add.at(n, (t["cy"][k] * ew + t["cx"][k])[t["inmap"][k]], 1)
    pop = {
        "x0=-1": int(left.sum()), "x0=ew-1": int(right.sum()),
        "seam_tile": sum(1 for sl in tb["slices"] if left[sl].any() and right[sl].any()),
        "y0=-1": int((t["y0"] == -1).sum()), "y0=eh-1": int((t["y0"] == eh - 1).sum()),
        "in1": int((nin == 1).sum()), "in2": int((nin == 2).sum()), "in3": int((nin == 3).sum()),
        "sub_tile": int(H < eo.TILE or W < eo.TILE), "ragged": int(H % eo.TILE != 0 or W % eo.TILE != 0),
        "multi_tile": int(len(tb["path"]) > 1),
        "window": tb["path"].count("window"), "direct": tb["path"].count("direct"), "none": tb["path"].count("none"),
        "win3072": int(((tb["area"] == 3072) & (np.array(tb["path"]) == "window")).sum()),
        "win4096": int(((tb["area"] == 4096) & (np.array(tb["path"]) == "direct")).sum()),
        "signed": int(env == "signed"), "T0": int(up == "T0"), "g0tile": int(up == "g0tile"),
        "n0": int((n == 0).sum()),
    }
    return pop


@functools.lru_cache(maxsize=None)
def build(name):
    """Everything of one case, computed once and shared read-only: camera, taps, tile boxes, float32 inputs (numpy), priors for the
    accumulate runs, the float64 reference and the bars (both without and with the priors)."""
    case = BY_NAME[name]
    H, W, eh, ew = case["H"], case["W"], case["eh"], case["ew"]
    cam = camera_of(case)
    t = eo.taps(cam, H, W, eh, ew, R)
    tb = eo.tile_boxes(t)
    g = torch.Generator().manual_seed(1000 + [c["name"] for c in CASES].index(name))
    colour = torch.rand(3, H, W, generator=g).numpy()
    T = (1 - torch.rand(1, H, W, generator=g) * 0.9).numpy()
    up = torch.randn(3, H, W, generator=g).numpy()
    env = torch.rand(3, eh, ew, generator=g).numpy()
    if case["env"] == "signed":
        env = (2 * env - 1).astype(np.float32)
    prior_alpha = torch.randn(1, H, W, generator=g).numpy()
    prior_env = torch.randn(3, eh, ew, generator=g).numpy()
    if case["up"] == "T0":
        T[:, H // 4:H // 2 + 1, W // 4:W // 2 + 1] = 0.0
    if case["up"] == "g0tile":
        up[:, :eo.TILE, :eo.TILE] = 0.0
    d = dict(case=case, cam=cam, taps=t, tiles=tb, colour=colour, T=T, g=up, env=env, prior_alpha=prior_alpha, prior_env=prior_env)
    d["out"], d["ga"], d["ge"] = eo.reference(t, colour, T, env, up)
    _, d["ga_acc"], d["ge_acc"] = eo.reference(t, colour, T, env, up, prior_alpha, prior_env)
    d["bar_out"], d["bar_ga"], d["bar_ge"], d["n"] = eo.bars(t, colour, T, env, up, DELTA)
    d["bar_ge_acc"] = eo.bars(t, colour, T, env, up, DELTA, prior_env)[2]
    return d


def search_boundary_eh(area, lo=4, hi=64):
    """The smallest eh in [lo, hi) at which tile 0 of the 'polar' 32 x 32 image over an eh x 1024 map has a box of ``area`` texels."""
    for eh in range(lo, hi):
        case = _c("search", "polar", 32, 32, eh, 1024, off=POLAR_OFF)
        tb = eo.tile_boxes(eo.taps(camera_of(case), 32, 32, eh, 1024, R))
        if tb["area"][0] == area:
            return eh
    return None


BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
