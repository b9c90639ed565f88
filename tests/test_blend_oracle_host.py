"""Host: the float64 blend oracle (tests/blend_oracle.py) against the fp32 port (pyoracle.Oracle(kind="port"), which shares no code with
it), against finite differences of its own forward, and against itself with one term planted wrong.  The forward's records, lists,
n_contrib and final_T come from the port's forward.  No GPU.

  test_forward_ties_port        n_contrib equal and pixels within K * unit of the port's on the unflagged pixels, every case
  test_records_tie_port         the float64 records through tests/chain_oracle.chain's record -> gradient map against the port's backward
                                with double-accumulated sums (mode 2): dL_dmean2D, dL_dconic, dL_dopacity, dL_dcolor, dL_dflows
  test_finite_differences       the records against central differences of the float64 forward in mean, conic, opacity, colour, depth, flow
  test_planted_errors           each single-term error of blend_oracle.PLANTS is flagged at the K the GPU test uses
  test_populations_and_cap      every need of every case is present and the flagged share is inside the cap, with the port's forward
  test_ref32_pinned_and_K       K per class = 4 * r_ref32 rounded up to a power of two, at most 64, pinned in blend_cases.K
"""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blend_cases as bc  # noqa: E402
import blend_oracle as bo  # noqa: E402
import chain_cases as cc  # noqa: E402
import chain_oracle as co  # noqa: E402
from util import pyoracle  # noqa: E402

FWD_CLASSES = (("colour", "out_color", "u_color"), ("depth", "out_depth", "u_depth"), ("flow", "out_flow", "u_flow"), ("T", "out_T", "u_T"))


def port_forward(case, keep=False):
    """The port's forward as the blend kernels' inputs (tests/util.collect_forward's keys).  With colors_precomp the port never writes
    its rgb scratch: the record's colour is the input colour, its depth the view depth, its flow the flow_2d input."""
    sc = bc.build(case)
    o = pyoracle.Oracle(sc, kind="port")
    f = {k: np.array(v, copy=True) for k, v in o.forward().items()}
    f["rgb"] = sc["colors_precomp"].numpy()
    f["rec_depth"] = f["depths"]
    f["rec_flow"] = sc["flow_2d"].numpy() if case.flow else np.zeros((sc["P"], 2), np.float32)
    f["final_T"] = f["out_T"]
    if keep:
        return sc, f, o
    o.close()
    return sc, f


@pytest.fixture(scope="module")
def cases():
    out = {}
    for case in bc.CASES:
        sc, f = port_forward(case)
        f64 = bo.forward(f, f["point_list"], f["ranges"], case.bg, case.W, case.H)
        out[case.name] = (case, sc, f, f64)
    return out


def _np(up):
    return tuple(None if up[k] is None else up[k].numpy() for k in ("grad_color", "grad_depth", "grad_alpha", "grad_flow"))


def _backward(case, f, f64, variant, fn=bo.backward, **kw):
    up = bc.mask_upstream(bc.upstream(case, variant), f64["flagged"])
    return fn(f, f["point_list"], f["ranges"], case.bg, case.W, case.H, f["n_contrib"], f["final_T"], *_np(up), **kw)


def test_forward_ties_port(cases):
    for name, (case, sc, f, f64) in cases.items():
        ok = ~f64["flagged"]
        assert np.array_equal(f["n_contrib"].astype(np.int64)[ok], f64["n_contrib"][ok]), name
        for cls, key, ukey in FWD_CLASSES:
            if cls == "flow" and not case.flow:
                continue
            r = bo.ratio(f[key], f64[key], f64[ukey])[..., ok]
            assert r.max() <= bc.K[cls], (name, cls, float(r.max()))


def test_records_tie_port():
    """The port evaluates each term in fp32 and sums in double (mode 2); the map from records to the five gradients is linear with
    per-Gaussian coefficients, so the bar of an output is the same map applied to K * unit with the coefficients' absolute values, plus
    8 ulp32 of the output for the map's own roundings."""
    for name in ("dense_16x16", "half_dark_32x32", "cover_64x48", "clamp_16x16", "ragged_23x31"):
        case = bc.BY_NAME[name]
        sc, f, o = port_forward(case, keep=True)
        f64 = bo.forward(f, f["point_list"], f["ranges"], case.bg, case.W, case.H)
        up = bc.mask_upstream(bc.upstream(case, "all"), f64["flagged"])
        try:
            pyoracle.set_accumulation(2)
            zero = lambda k, c: up[k] if up[k] is not None else np.zeros((c, case.H, case.W), np.float32)   # noqa: E731
            g = {k: v.copy() for k, v in o.backward(zero("grad_color", 3), zero("grad_depth", 1), zero("grad_alpha", 1), zero("grad_flow", 2)).items()}
        finally:
            pyoracle.set_accumulation(0)
            o.close()
        b = bo.backward(f, f["point_list"], f["ranges"], case.bg, case.W, case.H, f["n_contrib"], f["final_T"], *_np(up))
        inp, rec = cc.oracle_inputs(sc), cc.records_of(f)
        want = co.chain(inp, rec, b["words"])
        Kw = np.asarray([bc.K[c] for c in bo.WORD_CLASS])
        bar = co.chain(inp, dict(rec, conic_opacity=np.abs(rec["conic_opacity"])), -(Kw[None, :] * b["unit"]))   # the map on |coefficients|: all terms add
        vis = f["radii"] > 0
        pairs = (("dL_dmean2D", g["dL_dmean2D"][:, 0:2], want["dL_dmean2D"][:, 0:2], np.abs(bar["dL_dmean2D"][:, 0:2])),
                 ("dL_dconic", g["dL_dconic"][:, [0, 1, 3]], want["dL_dconic"], np.abs(bar["dL_dconic"])),
                 ("dL_dopacity", g["dL_dopacity"], want["dL_dopacity"], np.abs(bar["dL_dopacity"])),
                 ("dL_dcolor", g["dL_dcolor"], want["dL_dcolor"], np.abs(bar["dL_dcolor"])),
                 ("dL_dflows", g["dL_dflows"], want["dL_dflows"], np.abs(bar["dL_dflows"])))
        for k, got, w, u in pairs:
            r = bo.ratio(got[vis], w[vis], u[vis] + 8.0 * co.ulp32(w[vis]))
            print("%s %s: worst |port - f64| / bar = %.3f" % (name, k, float(r.max())))
            assert r.max() <= 1.0, (name, k, float(r.max()))


def test_finite_differences():
    """An un-clamped, cliff-free case on one tile: L = sum dL_colour . colour + dL_depth depth + dL_flow . flow + dL_alpha (1 - T) of the
    float64 forward, differenced centrally (h = 1e-6) in every record component of every Gaussian; the records imply
    dL/dmean = -o (A Mx + B My, B Mx + C My), dL/dA = -o Mxx / 2, dL/dB = -o Mxy, dL/dC = -o Myy / 2, dL/dopacity = M, and words 0-5 are
    dL/dcolour, dL/ddepth, dL/dflow.  Bar: 1e-6 of the row's largest |gradient| (h^2 terms: 1e-12)."""
    case = bc.Case("fd", 16, 16, "random", bg=bc.BG, seed=21)
    sc, f = port_forward(case)
    keep = np.unique(f["point_list"])[:14]
    pl = f["point_list"][np.isin(f["point_list"], keep)]
    rg = np.array([[0, pl.size]], np.uint32)
    rec = {k: f[k].astype(np.float64) for k in ("means2D", "conic_opacity", "rgb", "rec_depth", "rec_flow")}
    rec["conic_opacity"][:, 3] = np.minimum(rec["conic_opacity"][:, 3], 0.6)
    up = bc.upstream(case, "all")
    gc, gd, ga, gf = (a.astype(np.float64) for a in _np(up))

    def loss(r):
        o = bo.forward(r, pl, rg, case.bg, 16, 16)
        return o, (gc * o["out_color"]).sum() + (gd[0] * o["out_depth"]).sum() + (gf * o["out_flow"]).sum() + (ga[0] * (1.0 - o["out_T"])).sum()

    base, _ = loss(rec)
    assert not base["flagged"].any() and (base["n_contrib"] > 0).sum() > 100
    b = bo.backward(rec, pl, rg, case.bg, 16, 16, base["n_contrib"], base["out_T"], gc, gd, ga, gf)["words"]
    A, B, Cc, op = rec["conic_opacity"].T
    implied = {"means2D": np.stack([-op * (A * b[:, 6] + B * b[:, 7]), -op * (B * b[:, 6] + Cc * b[:, 7])], 1),
               "conic_opacity": np.stack([-0.5 * op * b[:, 8], -op * b[:, 10], -0.5 * op * b[:, 9], b[:, 11]], 1),
               "rgb": b[:, 0:3], "rec_depth": b[:, 3:4], "rec_flow": b[:, 4:6]}
    h = 1e-6
    for k, want in implied.items():
        for g in keep:
            for j in range(want.shape[1]):
                d = []
                for s in (1.0, -1.0):
                    r2 = {kk: v.copy() for kk, v in rec.items()}
                    r2[k].reshape(rec["means2D"].shape[0], -1)[g, j] += s * h
                    o2, L = loss(r2)
                    assert np.array_equal(o2["n_contrib"], base["n_contrib"])
                    d.append(L)
                fd = (d[0] - d[1]) / (2 * h)
                scale = max(np.abs(want[g]).max(), 1e-12)
                assert abs(fd - want[g, j]) <= 1e-6 * scale, (k, int(g), j, fd, want[g, j])


PLANT_CASE = {"swap89": ("dense_16x16", "colour"), "xy_as_xx": ("dense_16x16", "colour"), "no_bg": ("cover_64x48", "colour"),
              "cur_alpha": ("dense_16x16", "all"), "row_dropped": ("cover_64x48", "all"), "pair_other": ("cover_64x48", "all"),
              "no_mask": ("half_dark_32x32", "alpha")}


@pytest.mark.parametrize("plant", bo.PLANTS)
def test_planted_errors(plant, cases):
    """The oracle with one wrong term stands in for a kernel with that bug: the GPU test's comparison, at blend_cases.K, must flag it --
    and flags nothing of the unplanted evaluation rounded to fp32."""
    name, variant = PLANT_CASE[plant]
    case, sc, f, f64 = cases[name]
    good = _backward(case, f, f64, variant)
    bad = _backward(case, f, f64, variant, plant=plant, plant_block=(1, 1))
    Kw = np.asarray([bc.K[c] for c in bo.WORD_CLASS])
    clean = bo.ratio(good["words"].astype(np.float32), good["words"], good["unit"]) > Kw[None, :]
    assert not clean.any()
    hit = bo.ratio(bad["words"].astype(np.float32), good["words"], good["unit"]) > Kw[None, :]
    print("%s on %s [%s]: flags %d of %d elements, words %r" % (plant, name, variant, int(hit.sum()), hit.size, np.nonzero(hit.any(0))[0].tolist()))
    assert hit.any(), plant + ": the planted error passes the bar on every element"


def test_populations_and_cap(cases):
    kinds = set()
    for name, (case, sc, f, f64) in cases.items():
        share = bc.assert_flag_cap(case, f64["flagged"])
        pops = bc.populations(case, f, f64)
        bc.assert_populations(case, "default", pops)
        kinds |= {k for k in pops if k.startswith("drain_") and k != "drain_kinds"}
        print("%-20s flagged %.3f %%" % (name, 100 * share))
    assert len(kinds) == 15, sorted(kinds)


def test_ref32_pinned_and_K(cases):
    worst = {}

    def take(cls, r, where):
        if r.size and float(r.max()) > worst.get(cls, (-1.0,))[0]:
            worst[cls] = (float(r.max()), where, tuple(int(i) for i in np.unravel_index(int(np.argmax(r)), r.shape)))

    for name, (case, sc, f, f64) in cases.items():
        ok = ~f64["flagged"]
        r32 = bo.forward32(f, f["point_list"], f["ranges"], case.bg, case.W, case.H)
        assert np.array_equal(r32["n_contrib"][ok], f64["n_contrib"][ok]), name
        for cls, key, ukey in FWD_CLASSES:
            take(cls, np.where(ok, bo.ratio(r32[key], f64[key], f64[ukey]), 0.0), name)
        for variant in bc.VARIANTS:
            want = _backward(case, f, f64, variant)
            got = _backward(case, f, f64, variant, fn=bo.backward32)
            r = bo.ratio(got, want["words"], want["unit"])
            for j, cls in enumerate(bo.WORD_CLASS):
                take(cls, r[:, j], "%s [%s] word %d" % (name, variant, j))
    for cls, (r, where, at) in sorted(worst.items()):
        want = 2.0 ** math.ceil(math.log2(max(4.0 * r, 1e-30)))
        print("r_ref32 %-7s %8.4f  (%s, element %s)   4 r -> K = %g (pinned %g)" % (cls, r, where, at, want, bc.K[cls]))
        # the path: a pixel's block and list depth (the forward has one path); a record's queue path and drain mask in every block that adds to it
        case, sc, f, f64 = cases[where.split(" ")[0]]
        if cls in ("colour", "depth", "flow", "T"):
            y, x = at[-2], at[-1]
            print("        block (%d, %d), n_contrib %d of a list of %d" % (x // 8, y // 8, int(f["n_contrib"][y, x]),
                                                                       int(np.diff(f["ranges"][(y // 16) * ((case.W + 15) // 16) + x // 16].astype(np.int64))[0])))
        else:
            trace = {}
            bc.populations(case, f, f64, trace=trace)
            print("        Gaussian %d: (tile, sub-block, chunk, path, drain mask) %r" % (at[0], trace.get(at[0])))
    assert set(worst) == set(bc.K)
    for cls, (r, where, at) in worst.items():
        assert np.isfinite(r)
        near = {2.0 ** math.ceil(math.log2(max(4.0 * r * s, 1e-30))) for s in (1.0 - bc.K_TOLERANCE, 1.0, 1.0 + bc.K_TOLERANCE)}
        assert bc.K[cls] in near, "blend_cases.K[%r] = %g drifted from 4 * r_ref32 = %g rounded up to a power of two (%s)" % (cls, bc.K[cls], 4 * r, where)
        assert bc.K[cls] <= 64.0, cls
