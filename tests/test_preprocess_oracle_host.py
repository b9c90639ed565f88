"""Host: the float64 oracle of the per-Gaussian forward (tests/preprocess_oracle.py) against the fp32 port (run_oracle(kind="port"),
oracle/fdgs_oracle.c) on every case of tests/preprocess_cases.py, and against itself with one term planted wrong.  No GPU.

  test_port_pinned_and_K   every case and view: the populations the case exists for are there and the flag cap holds, both from the
                           float64 oracle alone; the port, one legal fp32 evaluation of the same function on the same inputs, takes
                           every decision (alive, radius, tile count, clamp bits) as float64 does wherever no decision is flagged, and
                           is within r_port * (4 ulp32 |f64_e| + sens_e) of it on every float element; preprocess_cases.K = 4 r_port
  test_planted_errors      each single-term error (preprocess_oracle.PLANTS) is flagged by the comparison on the case named for it
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_oracle as co  # noqa: E402
import preprocess_cases as pc  # noqa: E402
import preprocess_oracle as po  # noqa: E402
from util import run_oracle  # noqa: E402


def port_outputs(ref):
    """The port's forward under the float64 oracle's names."""
    return {"out_means3D": ref["out_means3D"], "cov3D": ref["cov3D"], "pix": ref["means2D"], "conic": ref["conic_opacity"][:, 0:3],
            "opacity": ref["conic_opacity"][:, 3], "depth": ref["depths"], "rgb": ref["rgb"], "radius": ref["radii"],
            "tiles": ref["tiles_touched"], "clamped": ref["clamped"]}


def compared(case):
    """the float tensors the port writes for this case (the reference never writes its cov3D / rgb scratch for a precomputed one)"""
    return tuple(k for k in po.FLOATS if not (k == "cov3D" and case.precomp_cov) and not (k == "rgb" and case.M == 0))


def decisions_differ(case, got, base, fl):
    """Gaussians whose decisions differ from float64's although none of theirs is flagged: -> {what: indices}."""
    ok = ~fl["geo"]
    alive = np.asarray(got["radius"]) > 0
    bad = {"alive": np.nonzero(ok & (alive != base["alive"]))[0], "radius": np.nonzero(ok & (np.asarray(got["radius"]) != base["radius"]))[0],
           "tiles": np.nonzero(ok & (np.asarray(got["tiles"]).astype(np.int64) != base["tiles"]))[0]}
    if case.M > 0:
        both = (alive & base["alive"])[:, None] & ~fl["rgb"]
        bad["clamped"] = np.nonzero((both & (np.asarray(got["clamped"]).astype(bool) != base["clamped"])).any(1))[0]
    return {k: v for k, v in bad.items() if len(v)}


@pytest.fixture(scope="module")
def evaluated():
    """per case: [(inp, f64, sens, flags, port outputs)] of every view, and the populations of view 0"""
    out = {}
    for case in pc.CASES:
        built = pc.build(case)
        views = []
        for v in range(len(case.poses)):
            scene = pc.view_scene(built, v)
            inp = pc.oracle_inputs(scene)
            base, sens = po.sensitivity(inp, seed=v)
            fl = po.flags(inp, base, sens)
            ref, _ = run_oracle(pc.activated(scene), None, kind="port")
            views.append((inp, base, sens, fl, port_outputs(ref)))
        inp, base, sens, fl, _ = views[0]
        pops = pc.assert_populations(case, inp, base, fl, built["planted"])
        for (i2, b2, s2, f2, _) in views[1:]:
            pc.assert_populations(case._replace(pops=()), i2, b2, f2, built["planted"])
        out[case.name] = (views, pops)
    return out


def test_port_pinned_and_K(evaluated):
    worst = {}
    for case in pc.CASES:
        views, pops = evaluated[case.name]
        print(case.name, {k: v for k, v in pops.items() if v})
        for v, (inp, base, sens, fl, port) in enumerate(views):
            bad = decisions_differ(case, port, base, fl)
            assert not bad, "%s view %d: the port decides differently from float64 on unflagged Gaussians: %r" % (case.name, v, bad)
            both = (port["radius"] > 0) & base["alive"]
            for k in compared(case):
                f64, s = base[k][both], sens[k][both]
                r, at = pc.worst(port[k][both], f64, co.core_bar(f64, s))
                if r > worst.get(k, (-1.0,))[0]:
                    worst[k] = (r, case.name, v, (int(np.nonzero(both)[0][at[0]]),) + tuple(int(a) for a in at[1:]))
    for k, (r, name, v, at) in sorted(worst.items()):
        print("r_port %-12s %10.4f  (%s view %d, element %s)   K = %g" % (k, r, name, v, at, pc.K[k]))
    assert set(worst) == set(pc.K)
    for k, (r, *_) in worst.items():
        w = pc.MARGIN * r
        assert np.isfinite(w), (k, worst[k])
        assert abs(pc.K[k] - w) <= pc.K_TOLERANCE * pc.K[k], "preprocess_cases.K[%r] = %g drifted from 4 * r_port = %g (%r)" % (k, pc.K[k], w, worst[k])


def test_flag_cap_and_populations_from_the_oracle_alone(evaluated):
    for case in pc.CASES:
        views, pops = evaluated[case.name]
        assert pops["stray"] <= pc.FLAG_CAP * case.P, (case.name, pops)
        if case.P == 65:
            assert case.P % 64 == 1   # 63 lanes of the last wave beyond P
    # the directed populations sit on both sides of their thresholds, a handful of fp32 steps away
    views, pops = evaluated["rot4d_d3t2"]
    for k in ("near_lo", "near_hi", "marg_lo", "marg_hi", "opa_lo", "opa_hi", "clampx_lo", "clampx_hi", "clampy_lo", "clampy_hi", "edge"):
        assert pops[k] >= 2, (k, pops)


PLANT_CASE = {"lowpass_one": "c3d_d3", "lambda2": "c3d_d3", "shifted_dir": "rot4d_d3t2", "ndc_no_minus1": "c3d_d1_mod07",
              "dt_sign": "rot4d_d3t2", "k2_no_times2": "rot4d_d3t2", "trunc_radius": "c3d_d3"}


@pytest.mark.parametrize("plant", po.PLANTS)
def test_planted_errors(plant, evaluated):
    """The oracle evaluated with one wrong term stands in for a kernel with that bug: the comparison the GPU test makes, at its bars
    (preprocess_cases.K, the decisions of the unflagged Gaussians), must flag it -- and flags nothing of the unplanted evaluation."""
    case = pc.BY_NAME[PLANT_CASE[plant]]
    inp, base, sens, fl, _ = evaluated[case.name][0][0]
    bad = po.forward(inp, plant=plant)
    hits = {}
    for label, got in (("clean", base), ("planted", bad)):
        g = dict(got)
        g["clamped"] = got["clamped"]
        d = decisions_differ(case, g, base, fl)
        both = got["alive"] & base["alive"]
        for k in po.FLOATS:
            h = co.flagged(got[k][both].astype(np.float32), base[k][both], sens[k][both], pc.K[k])
            if len(h):
                d[k] = h
        if label == "clean":
            assert not d, "the unplanted evaluation, rounded to fp32, is flagged: %r" % d
        else:
            hits = d
    print("%s: flagged %r" % (plant, {k: len(v) for k, v in hits.items()}))
    assert hits, "%s: the planted error passes every bar" % plant
