"""TEST INFRASTRUCTURE -- a hand-built table of rows for fdgs_densify_classify (csrc/densify.hip) with the flag byte each row must
get, shared by tests/test_densify_cases_host.py and tests/test_gpu_densify_edges.py.

The expected flags are a plain float64 restatement, written here, of the reference's decisions (scene/gaussian_model.py:
densify_and_prune's gradient = accum / denom with NaN -> 0; densify_and_clone's ``>= grad_threshold`` and ``<= percent_dense *
extent``; densify_and_split's ``>`` of the same limit; the final prune mask: opacity below min_opacity, and -- only ``if
max_screen_size`` -- max_radii2D above it or the largest scale above 0.1 * extent).  It does not use oracle/densify_oracle.py.

    CLONE        gradient >= max_grad and largest scale <= percent_dense * extent          (not with prune_only)
    SPLIT        gradient >= max_grad and largest scale >  percent_dense * extent          (not with prune_only)
    PRUNE        the Gaussian itself fails the final test; the reference resets max_radii2D in densification_postfix before it
                 looks at it, so the screen-size term acts only with prune_only
    PRUNE_CHILD  a split child of it -- same opacity, scales / (0.8 N), max_radii2D = 0 -- fails the final test

A row sits either EXACTLY on a threshold, by construction and without any transcendental rounding (raw scale 0 -> exp = 1 against
a limit that is 1.0; accum = max_grad with denom = 1 and max_grad a power of two; max_radii2D == max_screen_size), or at least
MARGIN = 1e-4 relative away from every threshold, where fp32 expf / sigmoid / division on the device (1e-7) cannot flip it: the GPU
test demands equality on every row.  tests/test_densify_cases_host.py asserts that property of the table.
"""
import itertools

import numpy as np

CLONE, SPLIT, PRUNE, PRUNE_CHILD = 1, 2, 4, 8
MARGIN = 1e-4
NEAR = 2e-4          # the rows 'just below / just above' a threshold
F32 = np.float32

# extent and percent_dense chosen so that one limit is exactly 1.0 = exp(0):
#   "small1": percent_dense * extent = 2^-7 * 128 = 1 (the clone / split limit), 0.1 * extent = 12.8
#   "big1"  : 0.1 * extent = 0.1 * 10 = 1 in double (the world-size prune limit), percent_dense * extent = 0.1
# max_grad = 2^-12 is an fp32 number, so accum = max_grad, denom = 1 is exactly on it.
BASES = {"small1": dict(extent=128.0, percent_dense=2.0 ** -7, max_grad=2.0 ** -12, min_opacity=0.005),
         "big1": dict(extent=10.0, percent_dense=0.01, max_grad=2.0 ** -12, min_opacity=0.3)}
SCREENS = [20.0, None, 0.0]
P_SIZES = [1, 255, 256, 257]
NS = [1, 2, 3]


def calls():
    """Every combination of base, max_screen_size (a value, None, 0), prune_only and N: (id, dict)."""
    out = []
    for (bname, base), screen, prune_only, N in itertools.product(BASES.items(), SCREENS, (False, True), NS):
        tag = "%s-screen%s-%s-N%d" % (bname, "None" if screen is None else "%g" % screen, "pruneonly" if prune_only else "densify", N)
        out.append((tag, dict(base, max_screen_size=screen, prune_only=prune_only, N=N)))
    return out


# (gradient, largest scale, max_radii2D, opacity):
#   gradient   "nan": accum = denom = 0;  "inf": accum > 0, denom = 0;  "on": accum = max_grad, denom = 1;  x: max_grad * x (denom = 3)
#   scale      "one": raw 0;  ("small", x) / ("big", x): x times the clone / split limit, the world-size limit
#   radius     offset from max_screen_size (from 20 where there is none): -1, 0 (on it), +1
#   opacity    a multiple of min_opacity; None: 0.9
_ROWS = [
    ("nan", ("small", 0.5), -1, None), ("inf", ("small", 0.5), -1, None), ("inf", ("small", 2.0), -1, None),
    (1 - NEAR, ("small", 0.5), -1, None), ("on", ("small", 0.5), -1, None), (1 + NEAR, ("small", 0.5), -1, None),
    ("on", ("small", 2.0), -1, None), (1 - NEAR, ("small", 2.0), -1, None),
    (3.0, ("small", 1 - NEAR), -1, None), (3.0, "one", -1, None), (3.0, ("small", 1 + NEAR), -1, None),
    (0.5, ("big", 1 - NEAR), -1, None), (0.5, ("big", 1 + NEAR), -1, None), (0.5, "one", -1, None),
    (3.0, ("big", 0.9), -1, None),      # N = 1: the child (scale / 0.8) is over the world-size limit, the parent is not
    (3.0, ("big", 1.2), -1, None),      # N >= 2: the parent is over it, the child is not
    (3.0, ("big", 3.0), -1, None),      # both
    ("nan", ("big", 3.0), -1, None),
    (0.5, ("small", 0.5), 0, None), (0.5, ("small", 0.5), 1, None), (3.0, ("small", 2.0), 1, None), (3.0, ("small", 0.5), 0, None),
    (0.5, ("small", 0.5), -1, 0.8), (0.5, ("small", 0.5), -1, 1 - 3 * MARGIN), (0.5, ("small", 0.5), -1, 1 + 3 * MARGIN),
    (0.5, ("small", 0.5), -1, 1.2),
    (3.0, ("small", 2.0), -1, 0.8), (3.0, ("small", 0.5), -1, 0.8),
    ("on", "one", 0, 1 + 3 * MARGIN),   # on three thresholds at once
    ("inf", ("big", 1.2), 1, 0.8),
]


def table(call, P):
    """The rows, repeated / truncated to P, as the fp32 inputs of fdgs_densify_classify for ``call``: dict of arrays
    (xyz_gradient_accum [P,1], denom [P,1], scaling_raw [P,3], opacity_raw [P,1], max_radii2D [P])."""
    small, big = call["percent_dense"] * call["extent"], 0.1 * call["extent"]
    screen = call["max_screen_size"] if call["max_screen_size"] else 20.0
    acc, den, sc, op, rad = [], [], [], [], []
    for i, (g, s, r, o) in enumerate(_ROWS):
        if g == "nan":
            acc.append(0.0); den.append(0.0)
        elif g == "inf":
            acc.append(1e-3); den.append(0.0)
        elif g == "on":
            acc.append(call["max_grad"]); den.append(1.0)
        else:
            acc.append(call["max_grad"] * g * 3.0); den.append(3.0)
        raw = 0.0 if s == "one" else float(np.log((small if s[0] == "small" else big) * s[1]))
        three = [raw - 1.0, raw - 0.25, raw - 3.0]
        three[i % 3] = raw                       # the largest scale sits on another axis from row to row
        sc.append(three)
        rad.append(screen + r)
        a = 0.9 if o is None else call["min_opacity"] * o
        op.append(float(np.log(a / (1 - a))))
    idx = np.arange(P) % len(_ROWS)
    return dict(xyz_gradient_accum=np.asarray(acc, F32)[idx, None], denom=np.asarray(den, F32)[idx, None],
                scaling_raw=np.asarray(sc, F32)[idx], opacity_raw=np.asarray(op, F32)[idx, None], max_radii2D=np.asarray(rad, F32)[idx])


def quantities(call, t):
    """float64: what the decisions compare -- (gradient, largest scale, largest scale of a child, max_radii2D, opacity) -- and their
    thresholds (None: not tested in this call)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        g = t["xyz_gradient_accum"][:, 0].astype(np.float64) / t["denom"][:, 0].astype(np.float64)
    g[np.isnan(g)] = 0.0
    smax = np.exp(t["scaling_raw"].astype(np.float64)).max(1)
    child = smax / (0.8 * call["N"])
    opacity = 1.0 / (1.0 + np.exp(-t["opacity_raw"][:, 0].astype(np.float64)))
    has_screen = bool(call["max_screen_size"])
    thr = dict(max_grad=call["max_grad"], small=call["percent_dense"] * call["extent"], big=0.1 * call["extent"] if has_screen else None,
               screen=call["max_screen_size"] if has_screen else None, min_opacity=call["min_opacity"])
    return dict(g=g, smax=smax, child=child, radius=t["max_radii2D"].astype(np.float64), opacity=opacity), thr


def expected_flags(call, t):
    """The flag byte of every row: the restatement described in the module docstring."""
    q, thr = quantities(call, t)
    flags = np.zeros(q["g"].shape[0], np.uint8)
    if not call["prune_only"]:
        hot = q["g"] >= thr["max_grad"]
        flags[hot & (q["smax"] <= thr["small"])] |= CLONE
        flags[hot & (q["smax"] > thr["small"])] |= SPLIT
    prune = q["opacity"] < thr["min_opacity"]
    prune_child = prune.copy()
    if thr["screen"] is not None:
        if call["prune_only"]:
            prune = prune | (q["radius"] > thr["screen"])
        prune = prune | (q["smax"] > thr["big"])
        prune_child = prune_child | (q["child"] > thr["big"])
    flags[prune] |= PRUNE
    flags[prune_child] |= PRUNE_CHILD
    return flags


def distances(call, t):
    """Relative distance of every compared quantity from its threshold, [rows, comparisons] (inf: gradient 0 or inf, or a
    threshold this call does not have)."""
    q, thr = quantities(call, t)
    pairs = [("g", "max_grad"), ("smax", "small"), ("smax", "big"), ("child", "big"), ("radius", "screen"), ("opacity", "min_opacity")]
    out = np.full((q["g"].shape[0], len(pairs)), np.inf)
    for k, (a, b) in enumerate(pairs):
        if thr[b] is None:
            continue
        with np.errstate(invalid="ignore"):
            d = np.abs(q[a] / thr[b] - 1.0)
        out[:, k] = np.where(np.isfinite(q[a]) & (q[a] != 0), d, np.inf)
    return out, [a + " vs " + b for a, b in pairs]
