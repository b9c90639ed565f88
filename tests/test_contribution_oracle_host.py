"""CPU: the numpy restatement of the contribution statistics (tests/contribution_oracle.py) against the reference's own arithmetic,
as the port oracle restates it -- so that the GPU test's expected values rest on the oracle and not on a second opinion.

* weight_sum is the oracle's dL_dcolor[:, 0] of a backward with grad_color = 1 and every other upstream gradient zero
  (backward.cu:1076: dL_dcolor[g][ch] += alpha T dL_dpixel[ch]), within the project's gradient bar;
* the per-pixel sum of w is 1 - out_T (T telescopes: w_k = T_k - T_k (1 - alpha_k));
* the last contributor's list position is the oracle's n_contrib, on every pixel."""
import numpy as np
import pytest
import torch

from util import GRAD_TOL, pyoracle

import contribution_cases as cases
import contribution_oracle as co


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "opaque", "1x1", "8x8", "17x9"])
def test_restatement_is_the_oracles_forward_and_backward(name):
    scene, ref, wk, excl = cases.oracle(name)
    P, W, H = int(scene["means3D"].shape[0]), int(scene["W"]), int(scene["H"])
    out = co.reduce(wk, P)
    # decisions: the same last contributor on EVERY pixel, cliff pixels included (the same float32 arithmetic, libm's expf)
    np.testing.assert_array_equal(wk["last_pos"], ref["n_contrib"])
    # sum of w against 1 - T: every step of the oracle's float32 T recurrence rounds once (2^-24 relative, T <= 1)
    tol = (wk["max_contrib"] + 1) * 2.0 ** -23
    err_T = float(np.abs(wk["sum_w"] - (1.0 - ref["out_T"].astype(np.float64))).max())
    assert err_T <= tol, (err_T, tol)
    # weight_sum against the reference's colour gradient
    o = pyoracle.Oracle(scene, kind="port")
    o.forward()
    z = torch.zeros
    g = o.backward(torch.ones(3, H, W), z(1, H, W), z(1, H, W), z(2, H, W))
    want = g["dL_dcolor"][:, 0].astype(np.float64)
    o.close()
    scale = max(1.0, float(np.abs(want).max()))
    err = float(np.abs(out["weight_sum"] - want).max())
    print(name, "weight_sum err %.3g (scale %.3g)  sum_w - (1 - T) %.3g (tol %.3g)  excluded %.2e" % (err, scale, err_T, tol, excl.mean()))
    assert err <= GRAD_TOL * scale, (err, scale)
    # the other outputs are consistent with the walk
    assert out["hits"].sum() == wk["pix"].size and out["dominant"].sum() == int((wk["dominant_id"] >= 0).sum())
    assert (out["weight_max"] <= 0.99 + 1e-12).all() and ((out["hits"] > 0) == (out["weight_max"] > 0)).all()
    assert float(excl.mean()) <= 0.01


def test_pixel_weights_skip_pixels_and_scale_the_sum():
    scene, ref, wk, _ = cases.oracle("a")
    P, W, H = int(scene["means3D"].shape[0]), int(scene["W"]), int(scene["H"])
    pw = cases.random_weights(H, W, 3)
    full, part = co.reduce(wk, P), co.reduce(wk, P, pw)
    assert 0.2 < (pw == 0).mean() < 0.4
    assert (part["dominant_id"][pw == 0] == -1).all() and np.array_equal(part["dominant_id"][pw > 0], full["dominant_id"][pw > 0])
    assert (part["hits"] <= full["hits"]).all() and part["hits"].sum() < full["hits"].sum()
    assert (part["weight_max"] <= full["weight_max"]).all()
    two = co.reduce(wk, P, 2.0 * (pw > 0))
    np.testing.assert_allclose(two["weight_sum"], 2.0 * co.reduce(wk, P, 1.0 * (pw > 0))["weight_sum"], rtol=1e-12)
    np.testing.assert_array_equal(two["hits"], part["hits"])
    assert co.contribution_oracle(ref, P, W, H)["near_tie"].shape == (H, W)
