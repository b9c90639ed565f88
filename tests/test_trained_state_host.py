"""CPU: the recorded trained states (tests/golden/trained_*.npz, tests/golden/make_golden_trained.py) -- that each fixture holds what it
was recorded for, that the port oracle reproduces the reference's stored outputs on it, and that the reference itself is well
conditioned on it (so that the GPU tests of tests/test_gpu_trained_state.py can hold the kernels to the plain bars)."""
import os

import numpy as np
import pytest

import golden_util
from test_oracle_golden import assert_port_matches_reference
from util import ill_conditioned_count, pyoracle, synth

TRAINED = golden_util.TRAINED
END = tuple(n for n in TRAINED if n.endswith("_end"))


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x.astype(np.float64)))


def active_coeffs(meta):
    return synth.active_sh_coeffs(int(meta["active_sh_degree"]), int(meta["active_sh_degree_t"]), bool(meta["force_sh_3d"]), int(meta["gaussian_dim"]))


@pytest.mark.parametrize("name", TRAINED)
def test_fixture_is_a_densified_trained_state(name):
    f = golden_util.load_trained(name)
    raw, meta, stats = f["raw"], f["meta"], f["stats"]
    P = raw["_xyz"].shape[0]
    assert P == meta["P"] > meta["P0"]
    assert meta["cloned"] > 0 and meta["split"] > 0 and meta["pruned"] > 0, meta
    # raw quaternions are not unit
    for n in ("_rotation",) + (("_rotation_r",) if meta["rot_4d"] else ()):
        off = np.abs(np.linalg.norm(raw[n].astype(np.float64), axis=1) - 1.0) > 1e-3
        assert off.mean() >= 0.5, "%s %s: | |q| - 1 | > 1e-3 on %.1f %% of the rows only" % (name, n, 100 * off.mean())
    # the coefficients beyond the active degrees were never touched
    assert float(np.abs(raw["_features"][:, active_coeffs(meta):]).max(initial=0.0)) == 0.0
    assert (raw["_features"][:, active_coeffs(meta) - 1] != 0).any(), "the last active coefficient was never trained"
    # statistics of real steps, with Gaussians no view of the interval saw: the NaN -> 0 branch of densify_classify
    assert (stats["denom"] == 0).any()
    assert (stats["denom"] > 0).any() and (stats["xyz_gradient_accum"] > 0).any()
    assert stats["denom"].shape == (P, 1) and stats["max_radii2D"].shape == (P,)
    assert len(f["views"]) == 2


def test_a_fixture_is_part_way_up_the_sh_ramp():
    below = [n for n in TRAINED if active_coeffs(golden_util.load_trained(n)["meta"]) < golden_util.load_trained(n)["raw"]["_features"].shape[1]]
    assert below, "every fixture has all of its allocated coefficients active"
    m = golden_util.load_trained("rot4d_end")["meta"]
    assert (m["active_sh_degree"], m["active_sh_degree_t"]) < (m["max_sh_degree"], m["max_sh_degree_t"])


def test_after_reset_opacities_are_pinned():
    """A reset gives at most 0.01; two Adam steps at lr 0.05 move the raw value by at most 0.1: sigmoid(logit(0.01) + 0.1) = 0.011."""
    raw = golden_util.load_trained("rot4d_reset")["raw"]
    assert float(_sigmoid(raw["_opacity"]).max()) <= 0.02


@pytest.mark.parametrize("name", END)
def test_end_state_has_clamped_colours(name):
    f = golden_util.load_trained(name)
    for v, (scene, up, fw, bw) in enumerate(f["views"]):
        vis = fw["radii"] > 0
        assert fw["clamped"][vis].any(), "%s view %d: no visible Gaussian has a colour channel clamped at 0" % (name, v)


@pytest.mark.parametrize("name", TRAINED)
def test_port_oracle_matches_reference_on_trained_state(name):
    for v, (scene, up, fw, bw) in enumerate(golden_util.load_trained(name)["views"]):
        assert_port_matches_reference("%s view %d" % (name, v), scene, up, fw, bw)


@pytest.mark.parametrize("name", TRAINED)
def test_reference_is_well_conditioned_on_trained_state(name):
    """util.ill_conditioned_count on the port oracle (pinned to the reference's stored outputs by the test above; the accumulation modes
    exist only there): the visible Gaussians on which it differs from ITSELF -- atomics in the opposite order (mode 1), per-Gaussian sums
    accumulated in double (mode 2), against mode 0 -- by more than 1e-4 * scale on a tensor behind the covariance chain.  At most 2 % in
    every view, and the count the generator stored."""
    f = golden_util.load_trained(name)
    for v, (scene, up, fw, bw) in enumerate(f["views"]):
        o = pyoracle.Oracle(scene, kind="port")
        vis = o.forward()["radii"] > 0
        count = ill_conditioned_count(o, up, vis)
        o.close()
        print("%s view %d: the port oracle differs from itself beyond 1e-4 on %d of %d visible Gaussians" % (name, v, count, int(vis.sum())))
        assert int(vis.sum()) == f["meta"]["visible"][v]
        assert count == f["meta"]["ill_conditioned"][v]
        assert count <= 0.02 * int(vis.sum())


@pytest.mark.parametrize("name", TRAINED)
def test_fixture_file_is_small_enough_to_commit(name):
    assert os.path.getsize(os.path.join(golden_util.HERE, "golden", "trained_%s.npz" % name)) <= 1 << 20
