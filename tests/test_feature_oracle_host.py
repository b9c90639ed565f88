"""CPU: the numpy restatement of the feature blend (tests/feature_oracle.py) against the port oracle's own colour path, which is a
3-channel feature blend with a background behind it -- so that the GPU test's expected values rest on the oracle:

* backward with C = 3 and g = the upstream colour gradient is the oracle's dL_dcolor (backward.cu:1076: dL_dcolor[g][ch] +=
  alpha T dL_dpixel[ch]), within the project's gradient bar;
* forward with F = the oracle's per-Gaussian colours, plus bg * out_T, is the oracle's out_color.  The oracle accumulates a pixel in
  float32: every contribution rounds its product and the running sum once (2^-24 relative each, of values <= max |colour|), the
  background term once more: (max_contrib + 1) * 2^-23 * max(1, max |colour|), the bar test_contribution_oracle_host.py puts on 1 - T;
* forward with F = ones is the walk's own sum of w."""
import numpy as np
import pytest
import torch

from util import GRAD_TOL, pyoracle, synth

import contribution_cases as cases
import feature_oracle as fo


@pytest.mark.parametrize("name", ["a", "c"])
def test_feature_restatement_is_the_oracles_colour_path(name):
    scene, ref, wk, excl = cases.oracle(name)
    P, W, H = int(scene["means3D"].shape[0]), int(scene["W"]), int(scene["H"])
    # backward: the oracle's colour gradient of a random upstream colour gradient, every other upstream gradient zero
    up = synth.make_upstream_grads(W, H, seed=5, scale=1.0)
    o = pyoracle.Oracle(scene, kind="port")
    o.forward()
    z = torch.zeros
    g = o.backward(up["grad_color"], z(1, H, W), z(1, H, W), z(2, H, W))
    want = g["dL_dcolor"].astype(np.float64)
    o.close()
    got = fo.backward(wk, up["grad_color"].numpy(), P)
    assert got.shape == (P, 3)
    scale = max(1.0, float(np.abs(want).max()))
    err_b = float(np.abs(got - want).max())
    assert err_b <= GRAD_TOL * scale, (err_b, scale)
    assert float(np.abs(want).max()) > 0.0
    # forward: the oracle's image
    rgb = ref["rgb"].astype(np.float64)
    bg = scene["bg"].numpy().astype(np.float64)
    img = fo.forward(wk, rgb) + bg[:, None, None] * ref["out_T"].astype(np.float64)[None]
    tol = (wk["max_contrib"] + 1) * 2.0 ** -23 * max(1.0, float(np.abs(rgb).max()))
    err_f = float(np.abs(img - ref["out_color"]).max())
    print(name, "backward err %.3g (bar %.3g)  forward err %.3g (bar %.3g)" % (err_b, GRAD_TOL * scale, err_f, tol))
    assert err_f <= tol, (err_f, tol)
    # ones: the sum of the weights; a [P] vector is one channel
    ones = fo.forward(wk, np.ones(P))
    assert ones.shape == (1, H, W)
    np.testing.assert_allclose(ones[0], wk["sum_w"], rtol=1e-12, atol=0.0)
    # the two functions are adjoint to each other
    rng = np.random.default_rng(3)
    F, G = rng.standard_normal((P, 5)), rng.standard_normal((5, H, W))
    lhs, rhs = float((fo.forward(wk, F) * G).sum()), float((F * fo.backward(wk, G, P)).sum())
    assert abs(lhs - rhs) <= 1e-9 * max(1.0, abs(lhs))
