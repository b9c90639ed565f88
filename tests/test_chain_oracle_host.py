"""Host: the float64 oracle of the per-Gaussian backward (tests/chain_oracle.py) against the fp32 port (oracle_chain,
oracle/fdgs_oracle.c), against finite differences of the float64 forward (oracle/torch_oracle.preprocess), and against itself with one
term planted wrong.  The forward's records come from the port's forward.  No GPU.

  test_port_pinned_and_K     every case of tests/chain_cases.py: the populations the case exists for are there; the port, one correct
                             fp32 evaluation of the same function on the same inputs, is within r_port * (4 ulp32 |f64_e| + sens_e) of
                             the float64 oracle on every element, and the constants K of chain_cases are 4 * r_port per tensor
  test_finite_differences    where the reference's backward IS the forward's derivative (3D, un-clamped, no Q4 / Q5): central
                             differences of the float64 forward through a loss that is linear in the forward's per-Gaussian outputs
  test_planted_errors        each single-term error (chain_oracle.PLANTS) is flagged by the comparison on the case built for it
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_cases as cc  # noqa: E402
import chain_oracle as co  # noqa: E402
from util import pyoracle  # noqa: E402
from oracle import torch_oracle  # noqa: E402

PORT_TENSORS = ("dL_dmean2D", "dL_dcolor", "dL_dflows", "dL_dcov3D", "dL_dmean3D", "dL_dopacity", "dL_dts", "dL_dscale", "dL_dscale_t",
                "dL_drot", "dL_drot_r", "dL_dsh")


def port_forward(scene):
    o = pyoracle.Oracle(cc.activated(scene), kind="port")
    fwd = {k: v.copy() for k, v in o.forward().items()}
    return o, fwd


def port_chain(o, fwd, scene, acc, colour_only=False):
    """The port's chain on the accumulator records: the blend backward's sums from the moments and the activations' backward are
    evaluated here in fp32 numpy, in the order preprocess_bwd.hip writes them (one legal fp32 evaluation)."""
    f = np.float32
    a = acc.astype(f)
    P = a.shape[0]
    if colour_only:
        a = a.copy()
        a[:, 3:] = 0
    vis = fwd["radii"] > 0
    cA, cB, cC, oe = (fwd["conic_opacity"][:, i] for i in range(4))
    hw, hh = f(0.5 * scene["W"]), f(0.5 * scene["H"])
    m2 = np.zeros((P, 3), f)
    m2[:, 0] = np.where(vis, -oe * hw * (cA * a[:, 6] + cB * a[:, 7]), f(0))
    m2[:, 1] = np.where(vis, -oe * hh * (cB * a[:, 6] + cC * a[:, 7]), f(0))
    m2[:, 2] = a[:, 3]
    con = np.zeros((P, 4), f)
    con[:, 0], con[:, 1], con[:, 3] = f(-0.5) * oe * a[:, 8], f(-0.5) * oe * a[:, 10], f(-0.5) * oe * a[:, 9]
    con[~vis] = 0
    g = {k: v.copy() for k, v in o.chain(m2, con, a[:, 11], a[:, 0:3], a[:, 4:6]).items()}
    if scene.get("raw"):
        act = cc.activated(scene)
        if scene.get("scales") is not None:
            g["dL_dscale"] = g["dL_dscale"] * act["scales"].numpy()
            q, inv = act["rotations"].numpy(), (1.0 / scene["rotations"].norm(dim=1).clamp_min(1e-12)).numpy()
            d = (q * g["dL_drot"]).sum(1, keepdims=True, dtype=f)
            g["dL_drot"] = (g["dL_drot"] - q * d) * inv[:, None]
        if scene["rot_4d"]:
            g["dL_dscale_t"] = g["dL_dscale_t"] * act["scales_t"].numpy().reshape(P)
            q, inv = act["rotations_r"].numpy(), (1.0 / scene["rotations_r"].norm(dim=1).clamp_min(1e-12)).numpy()
            d = (q * g["dL_drot_r"]).sum(1, keepdims=True, dtype=f)
            g["dL_drot_r"] = (g["dL_drot_r"] - q * d) * inv[:, None]
        op = act["opacities"].numpy().reshape(P)
        g["dL_dopacity"] = g["dL_dopacity"] * (op * (f(1) - op))
    return g


@pytest.fixture(scope="module")
def port_ratios():
    """{tensor: (r_port, case, element)} over every case and view, and {case: populations}."""
    assert pyoracle.have_chain("port")
    worst, pops = {}, {}
    for case in cc.CASES:
        built = cc.build(case)
        for v in range(case.views):
            scene = cc.view_scene(built, v)
            o, fwd = port_forward(scene)
            inp, rec, acc = cc.oracle_inputs(scene), cc.records_of(fwd), built["acc"][v]
            if v == 0:
                pops[case.name] = cc.assert_populations(case, inp, rec, acc)
            f64, sens = co.sensitivity(inp, rec, acc, seed=v)
            g = port_chain(o, fwd, scene, acc)
            for k in PORT_TENSORS:
                r, at = cc.worst(g[k], f64[k], co.core_bar(f64[k], sens[k]))
                if r > worst.get(k, (-1.0,))[0]:
                    worst[k] = (r, case.name, at)
            if case.M > 0:
                # the hand-over words: colour words only -> the port's dL_dmean3D is the mean words (0 + x), its dL_dts the time word
                # where no rot_4d chain adds to it
                a0 = acc.copy()
                a0[:, 3:] = 0
                f0, s0 = co.sensitivity(inp, rec, a0, seed=v)
                g0 = port_chain(o, fwd, scene, acc, colour_only=True)
                r, at = cc.worst(g0["dL_dmean3D"], f0["sh_words"][:, 0:3], co.core_bar(f0["sh_words"][:, 0:3], s0["sh_words"][:, 0:3]))
                if not case.rot_4d:
                    r2, at2 = cc.worst(g0["dL_dts"], f0["sh_words"][:, 3], co.core_bar(f0["sh_words"][:, 3], s0["sh_words"][:, 3]))
                    r, at = (r2, at2) if r2 > r else (r, at)
                if r > worst.get("sh_words", (-1.0,))[0]:
                    worst["sh_words"] = (r, case.name, at)
            o.close()
    return worst, pops


def test_port_pinned_and_K(port_ratios):
    worst, pops = port_ratios
    for k, (r, name, at) in sorted(worst.items()):
        print("r_port %-12s %10.3f  (%s, element %s)   K = %g" % (k, r, name, at, cc.K[k]))
    want = {k: 4.0 * worst[k][0] for k in PORT_TENSORS}
    want["sh_words"] = 4.0 * max(worst["sh_words"][0], worst["dL_dmean3D"][0])
    want["stage"] = 4.0
    for k, w in want.items():
        assert np.isfinite(w), (k, worst.get(k))
        assert abs(cc.K[k] - w) <= cc.K_TOLERANCE * max(cc.K[k], 1e-30) or (w == 0.0 and cc.K[k] == 0.0), \
            "chain_cases.K[%r] = %g drifted from 4 * r_port = %g (%r)" % (k, cc.K[k], w, worst.get(k))
    assert set(cc.K) == set(want)


def test_q7_changes_no_number():
    """Q7 (cov12 read as Sigma[3][k], the forward reads Sigma[k][3]): Sigma = M^T M is symmetric term by term -- entry [3][k] and entry
    [k][3] are the same products summed in the same order -- so the quirk, and a plant that transposes it back, changes no bit."""
    built = cc.build(cc.BY_NAME["rot4d_act"])
    scene = cc.view_scene(built, 0)
    o, fwd = port_forward(scene)
    o.close()
    inp, rec, acc = cc.oracle_inputs(scene), cc.records_of(fwd), built["acc"][0]
    a, b = co.chain(inp, rec, acc), co.chain(inp, rec, acc, plant="q7")
    for k in co.OUTPUTS:
        assert a[k].tobytes() == b[k].tobytes(), k


PLANT_CASE = {"half": "c3d_act", "clamp": "c3d_act", "quat_sign": "rot4d_act", "q1": "dim4_act", "sh_c3": "c3d_act", "sigmoid2": "c3d_raw_m9"}


@pytest.mark.parametrize("plant", [p for p in co.PLANTS if p != "q7"])
def test_planted_errors(plant):
    """The oracle evaluated with one wrong term stands in for a kernel with that bug: the comparison function, at the bar the GPU test
    uses (chain_cases.K), must flag it on the case built for it -- and flags nothing of the unplanted evaluation."""
    case = cc.BY_NAME[PLANT_CASE[plant]]
    built = cc.build(case)
    scene = cc.view_scene(built, 0)
    o, fwd = port_forward(scene)
    o.close()
    inp, rec, acc = cc.oracle_inputs(scene), cc.records_of(fwd), built["acc"][0]
    f64, sens = co.sensitivity(inp, rec, acc)
    bad = co.chain(inp, rec, acc, plant=plant)
    hits = {}
    for k in co.OUTPUTS:
        assert len(co.flagged(f64[k].astype(np.float32), f64[k], sens[k], cc.K[k])) == 0, k   # the unplanted evaluation, rounded to fp32
        h = co.flagged(bad[k].astype(np.float32), f64[k], sens[k], cc.K[k])
        if len(h):
            hits[k] = h
    print("%s: flagged %r" % (plant, {k: "%d of %d" % (len(h), f64[k].size) for k, h in hits.items()}))
    assert hits, "%s: the planted error passes the bar on every tensor" % plant
    if plant == "clamp":
        # the Gaussians beyond the x clamp are the ones flagged
        m = rec["out_means3D"].astype(np.float64)
        vm = inp["viewmatrix"].astype(np.float64)
        txtz = (vm[0] * m[:, 0] + vm[4] * m[:, 1] + vm[8] * m[:, 2] + vm[12]) / (vm[2] * m[:, 0] + vm[6] * m[:, 1] + vm[10] * m[:, 2] + vm[14])
        assert (np.abs(txtz[np.unique(hits["dL_dmean3D"][:, 0])]) > co.CLAMP * inp["tan_fovx"]).all()


def test_finite_differences():
    """3D Gaussians, SH degree 3, nobody beyond the clamp, nothing clamped: the reference's backward is the derivative of the forward
    (torch_oracle.preprocess, float64) -- up to its two regularisers, 1e-7 in denom2inv (backward.cu:548) and in m_w (:880), which move
    a term by at most 1e-7 / denom^2 <= 1.3e-5 of itself (denom >= 0.09, the low-pass's).  The loss is linear in the forward's
    per-Gaussian outputs with the weights the accumulator record stands for: L = sum gpix . pix + gconic . conic + gop opacity +
    gcol . rgb + gz depth.  Bar per Gaussian and tensor: 1e-4 of the row's largest |term| (central differences, h = 1e-6: 1e-9)."""
    case = cc.Case("fd3d", 65, 3, False, 3, 0, 16, seed=41)
    built = cc.build(case)
    scene = cc.view_scene(built, 0)
    o, fwd = port_forward(scene)
    o.close()
    inp, rec, acc = cc.oracle_inputs(scene), cc.records_of(fwd), built["acc"][0]
    vis = rec["radii"] > 0
    assert vis.sum() >= 40 and not rec["clamped"][vis].any()
    f64 = co.chain(inp, rec, acc)
    W, H = inp["W"], inp["H"]
    gpix = f64["dL_dmean2D"][:, 0:2] / np.array([0.5 * W, 0.5 * H])
    gcon = f64["dL_dconic"] * np.array([1.0, 2.0, 1.0])   # the record's xy word is half of dL/d(conic xy) (Q12)
    a64 = acc.astype(np.float64)
    names = ("means3D", "scales", "rotations", "opacities", "shs")
    base = {k: scene[k].double() for k in names}

    def loss_rows(p):
        pre = torch_oracle.preprocess(scene, p)
        L = (torch.from_numpy(gpix) * pre["pix"]).sum(1) + (torch.from_numpy(gcon) * pre["conic"]).sum(1)
        L = L + torch.from_numpy(a64[:, 11]) * pre["opacity"] + (torch.from_numpy(a64[:, 0:3]) * pre["rgb"]).sum(1)
        return (L + torch.from_numpy(a64[:, 3]) * pre["depth"]).numpy()

    h = 1e-6
    pairs = {"means3D": "dL_dmean3D", "scales": "dL_dscale", "rotations": "dL_drot", "opacities": "dL_dopacity", "shs": "dL_dsh"}
    for k, gk in pairs.items():
        flat = base[k].reshape(case.P, -1)
        fd = np.zeros(tuple(flat.shape))
        for j in range(flat.shape[1]):
            d = []
            for s in (1.0, -1.0):
                t = flat.clone()
                t[:, j] += s * h
                d.append(loss_rows(dict(base, **{k: t.reshape(base[k].shape)})))
            fd[:, j] = (d[0] - d[1]) / (2 * h)
        got = f64[gk].reshape(case.P, -1)
        scale = np.maximum(np.abs(fd).max(1, keepdims=True), 1e-30)
        err = np.abs(got - fd)[vis] / scale[vis]
        print("%s: worst |f64 - fd| / row max = %.2e" % (gk, err.max()))
        assert err.max() <= 1e-4, (gk, float(err.max()))
