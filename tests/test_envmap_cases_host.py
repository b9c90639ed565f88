"""CPU: the cases, bars and float32 emulation of the environment-map edge tests (tests/envmap_cases.py, tests/envmap_oracle.py)
before any of it is held against csrc/envmap.hip: every population a case is tagged with is there, the two window-boundary tiles
exist, no pixel sits on the seam itself, delta stands on a measured float64 difference, the emulation stays within every bar in both
summation orders, and each of the six mutants exceeds a bar somewhere."""
import numpy as np
import pytest
import torch

import envmap_cases as ec
import envmap_oracle as eo

NAMES = [c["name"] for c in ec.CASES]
ALL_TAGS = ("x0=-1", "x0=ew-1", "seam_tile", "y0=-1", "y0=eh-1", "in1", "in2", "sub_tile", "ragged", "multi_tile", "window", "direct",
            "win3072", "win4096", "signed", "T0", "g0tile", "n0")
WORST = {}


def _ratios(got, d, acc=False):
    """max error / bar of (out, d / d alpha, d / d env) against the case's float64 reference; 0 / 0 counts as 0."""
    out, ga, ge = (np.asarray(a, np.float64) for a in got)
    pairs = ((out, d["out"], d["bar_out"]), (ga, d["ga_acc" if acc else "ga"], d["bar_ga"]),
             (ge, d["ge_acc" if acc else "ge"], d["bar_ge_acc" if acc else "bar_ge"]))
    res = []
    for a, want, bar in pairs:
        err = np.abs(a - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, 0.0, err / bar)
        res.append(float(r.max()))
    return res


@pytest.mark.parametrize("name", NAMES)
def test_every_tagged_population_is_present(name):
    d = ec.build(name)
    case = d["case"]
    pop = ec.populations(d["taps"], d["tiles"], case["up"], case["env"])
    assert set(case["tags"]) <= set(ALL_TAGS)
    missing = [t for t in case["tags"] if pop[t] == 0]
    assert not missing, (name, missing, pop)
    assert pop["none"] == 0, "a tile with no contributing pixel cannot occur (envmap_cases docstring)"
    assert case["W"] <= 80 and case["H"] <= 64 and case["eh"] * case["ew"] <= 2 ** 19
    if case["up"] == "T0":
        assert (d["T"] == 0).sum() >= 16 and (d["T"] != 0).any()
    if case["up"] == "g0tile":
        assert not d["g"][:, :16, :16].any() and len(d["tiles"]["path"]) > 1
        assert d["n"][d["tiles"]["box"][0][2], d["tiles"]["box"][0][0]] > 0          # the tile does touch texels; its terms are all zero


def test_populations_shapes_and_maps_are_covered():
    tagged = {t for c in ec.CASES for t in c["tags"]}
    assert tagged == set(ALL_TAGS), set(ALL_TAGS) - tagged
    for pose in ("rig2", "seam"):
        assert {(c["W"], c["H"]) for c in ec.CASES if c["pose"] == pose} >= set(ec.SHAPES)
    forms = {}
    for c in ec.CASES:
        forms.setdefault((c["eh"], c["ew"]), set()).add(c["env"])
    for m in ((1, 1), (1, 7), (7, 1), (2, 3), (40, 72), (64, 64)):
        assert forms[m] == {"noise", "signed"}, (m, forms[m])
    paths = [p for n in NAMES for p in ec.build(n)["tiles"]["path"]]
    assert "window" in paths and "direct" in paths and "none" not in paths
    # each pole from both poses that face it, the seam tile on small and on full-width boxes
    for tag in ("y0=-1", "y0=eh-1", "seam_tile"):
        assert sum(tag in c["tags"] for c in ec.CASES) >= 2, tag


def test_window_boundary_tiles_exist():
    """ew = 1024 with the pole and the seam inside tile 0: a box of exactly ENV_WIN = 3072 texels on the window path, one of 4096
    on the direct path; the recorded eh are what the search finds; the wide map sends a 32 x 32 image down the direct path."""
    assert eo.ENV_WIN == 3072
    assert ec.search_boundary_eh(3072) == ec.EH_3072 and ec.search_boundary_eh(4096) == ec.EH_4096
    a = ec.build("polar-32x32-map%dx1024-win3072" % ec.EH_3072)["tiles"]
    assert a["area"][0] == 3072 and a["path"][0] == "window" and tuple(a["box"][0]) == (0, 1023, 0, 2)
    b = ec.build("polar-32x32-map%dx1024-win4096" % ec.EH_4096)["tiles"]
    assert b["area"][0] == 4096 and b["path"][0] == "direct" and tuple(b["box"][0]) == (0, 1023, 0, 3)
    w = ec.build("polar-32x32-map8x4096-wide")["tiles"]
    assert "direct" in w["path"] and "window" in w["path"]


def test_no_pixel_is_exempt():
    """A pixel is exempt only on the seam itself (X < 0, |Y| < delta R); no case has one, with room to spare: 1e4 delta."""
    for n in NAMES:
        d = ec.build(n)
        assert not eo.exempt(d["taps"], ec.DELTA, ec.R).any(), n
        assert not eo.exempt(d["taps"], 1e4 * ec.DELTA, ec.R).any(), n


def test_delta_stands_on_the_measured_difference():
    """The kernel's float64 formulation (cofactor inverse, u * ew - 0.5) against the oracle's (linalg.inv, grid_sample's expression):
    the largest coordinate difference over all cases is what envmap_cases records, and DELTA is 10 x that rounded up to a power of ten."""
    dx = dy = 0.0
    for n in NAMES:
        d = ec.build(n)
        c = d["case"]
        kx, ky = eo.kernel_texel_coords(d["cam"], c["H"], c["W"], c["eh"], c["ew"], ec.R)
        dx, dy = max(dx, float(np.abs(kx - d["taps"]["ix"]).max())), max(dy, float(np.abs(ky - d["taps"]["iy"]).max()))
    print("largest float64 difference: ix %.3e, iy %.3e texels; DELTA %.0e" % (dx, dy, ec.DELTA))
    # (the last bits of the difference depend on the linear-algebra library: recorded to within a factor of two)
    assert 0.5 * ec.MEASURED_F64_DIFF[0] <= dx <= 2 * ec.MEASURED_F64_DIFF[0] and 0.5 * ec.MEASURED_F64_DIFF[1] <= dy <= 2 * ec.MEASURED_F64_DIFF[1]
    assert ec.DELTA == 10.0 ** np.ceil(np.log10(10 * max(ec.MEASURED_F64_DIFF)))
    assert 10 * max(dx, dy) <= ec.DELTA


def test_atan2_and_acos_forms_agree_away_from_the_pole():
    """v = atan2(rho, z) / pi against acos(z / R) / pi: 1e-12 where rho >= 0.05 R (u is the same expression in both)."""
    seen = 0
    for n in NAMES:
        d = ec.build(n)
        X = torch.from_numpy(d["taps"]["X"])
        far = torch.sqrt(X[..., 0] ** 2 + X[..., 1] ** 2) >= 0.05 * ec.R
        (u1, v1), (u2, v2) = eo.texcoord(X, ec.R), eo.texcoord_atan2(X, ec.R)
        assert torch.equal(u1, u2)
        if far.any():
            assert float((v1 - v2).abs()[far].max()) <= 1e-12, n
            seen += int(far.sum())
    assert seen > 1000


@pytest.mark.parametrize("name", ["rig2-33x31-map40x72-signed", "seam-17x19-map2x3-noise", "seam-50x36-map40x72-noise"])
def test_reference_is_the_autograd_statement(name):
    """envmap_oracle.reference (taps written out, atan2 form) against composite / composite_grads (acos form, autograd) on cases
    away from the poles: 1e-9 of the tensors' scale (the acos form's own float64 loss is below that there)."""
    d = ec.build(name)
    H, W = d["case"]["H"], d["case"]["W"]
    cam = eo.abi_camera(d["cam"])
    colour, alpha, env, g = (torch.from_numpy(np.asarray(a, np.float64)) for a in (d["colour"], 1 - d["T"].astype(np.float64), d["env"], d["g"]))
    want, _ = eo.composite(colour, alpha, env, cam, ec.R)
    ga, ge = eo.composite_grads(colour, alpha, env, cam, g, ec.R)
    assert np.abs(d["out"] - want.numpy()).max() <= 1e-9
    assert np.abs(d["ga"] - ga.numpy().reshape(H, W)).max() <= 1e-9 * max(1.0, float(ga.abs().max()))
    assert np.abs(d["ge"] - ge.numpy()).max() <= 1e-9 * max(1.0, float(ge.abs().max()))


@pytest.mark.parametrize("name", NAMES)
def test_emulation_stays_within_every_bar(name):
    """The float32 emulation in both summation orders, without and with accumulate: every element within its bar (the bars are
    derivations: beyond one, the derivation is wrong, not the factor); untouched texels exact."""
    d = ec.build(name)
    for order in ("row", "tile"):
        for acc in (False, True):
            pa, pe = (d["prior_alpha"], d["prior_env"]) if acc else (None, None)
            got = eo.emulate_f32(d["taps"], d["colour"], d["T"], d["env"], d["g"], order, pa, pe)
            r = _ratios(got, d, acc)
            if acc:
                # d / d alpha under accumulate is fl32(prior + ga), one more rounding of a value the bar does not know: held bit
                # for bit to that sum (as on the GPU), not to the bar
                assert np.array_equal(got[1], d["prior_alpha"].reshape(got[1].shape) + plain_ga)
                r[1] = 0.0
            else:
                plain_ga = got[1]
            for k, v in zip(("forward", "d_alpha", "d_env"), r):
                WORST[k] = max(WORST.get(k, 0.0), v)
            assert max(r) <= 1.0, (name, order, acc, r)
            zero = d["n"] == 0
            want = d["prior_env"][:, zero] if acc else np.zeros((3, int(zero.sum())), np.float32)
            assert np.array_equal(got[2][:, zero].view(np.int32), want.view(np.int32))
    print("%-40s worst ratios: forward %.3f  d_alpha %.3f  d_env %.3f" % ((name,) + tuple(r)))


@pytest.mark.parametrize("mutant", eo.MUTANTS)
def test_every_mutant_exceeds_a_bar(mutant):
    """One defect each: (a) the seam wraps, (b) the pole rows clamp, (c) align_corners = True, (d) the weights of corners 1 and 2
    swapped, (e) round instead of floor, (f) the scatter drops the pixels a corner of which was clamped into the box.  Each must
    exceed a bar on at least one case -- a mutant that passes everywhere means a case is missing."""
    caught = []
    for n in NAMES:
        d = ec.build(n)
        c = d["case"]
        got = eo.mutants(d["cam"], c["H"], c["W"], c["eh"], c["ew"], d["colour"], d["T"], d["env"], d["g"], ec.R, names=(mutant,))[mutant]
        r = _ratios(got, d)
        if max(r) > 1.0:
            caught.append((n, r))
    assert caught, "no case catches the mutant %s" % mutant
    n, r = max(caught, key=lambda x: max(x[1]))
    print("mutant %-14s caught by %d of %d cases; first %s; worst %s (ratios forward %.3g, d_alpha %.3g, d_env %.3g)" % (
        (mutant, len(caught), len(NAMES), caught[0][0], n) + tuple(r)))
    if mutant == "drop_clamped":
        assert all(x[1][0] <= 1.0 and x[1][1] <= 1.0 for x in caught)       # a scatter defect: only d / d env sees it


def test_worst_ratios_are_reported():
    """Not a check of its own: prints the emulation's worst error / bar ratio per output over all cases."""
    for k, v in sorted(WORST.items()):
        print("emulation worst ratio %-8s %.3f" % (k, v))
