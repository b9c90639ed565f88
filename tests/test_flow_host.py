"""CPU: the PyTorch statement of the per-Gaussian flow (tests/flow_oracle.py) against the C oracle's screen positions, the argument
checks of fdgs_gaussian_flow_forward / fdgs_gaussian_flow_backward (no GPU is touched) and the signatures of render / render_raw."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import flow_cases as fc
import chain_oracle as co
import flow_oracle as fo
import util

# worst |oracle(float32) - (means2D_to - means2D_from)| measured over ORACLE_CASES, in units of 2^-23 * max(1, |pix_0|, |pix_1|)
MEASURED_UNITS = 2.40
ORACLE_CASES = [(True, ("rig0", "rig1")), (True, ("rig1", "rig1")), (False, ("rig0", "rig1")), (False, ("rig1", "rig0"))]


def _oracle_units(rot_4d, poses, P=1000):
    s0, s1 = fc.pair(P, rot_4d, poses)
    r0, _ = util.run_oracle(s0)
    r1, _ = util.run_oracle(s1)
    both = (r0["radii"] > 0) & (r1["radii"] > 0)
    assert both.mean() >= 0.5, "the scene should keep at least half of its Gaussians in both views"
    par = fc.params_of(s0, raw=False)
    flow, p0, p1, ok = fo.gaussian_flow(*fc.cam_args(s0, s1), *[par[n] for n in fo.NAMES], rot_4d=rot_4d, raw=False, dtype=torch.float32,
                                        details=True)
    assert flow.dtype == torch.float32 and bool(ok[torch.from_numpy(both)].all())
    want = r1["means2D"][both] - r0["means2D"][both]          # float32 - float32
    assert want.dtype == np.float32
    unit = 2.0 ** -23 * np.maximum(1.0, np.maximum(np.abs(p0.numpy()[both]).max(1), np.abs(p1.numpy()[both]).max(1)))
    dev = np.abs(flow.numpy()[both].astype(np.float64) - want.astype(np.float64)).max(1) / unit
    return float(dev.max()), float(np.abs(want).max())


def test_oracle_in_float32_is_the_c_oracles_screen_motion():
    """flow_oracle in float32 == means2D(forward at the target) - means2D(forward at the source) of the C oracle, for every Gaussian with
    radii > 0 in both views (rot_4d and plain 4D, two rig poses, one and two cameras).  The two differ by rounding only: the oracle's
    float32 matrix products and its float32 ndc2Pix against the C oracle's fixed evaluation order and double-promoted ndc2Pix.
    Measured worst deviation over the four cases: 2.40 units of 2^-23 * max(1, |pix_0|, |pix_1|) (2.14, 2.40, 2.13, 2.13 in the order
    of ORACLE_CASES); the assertion is 2 x that, 4.8 units.  Beyond 64 units the oracle would be wrong, not rounded differently."""
    worst = 0.0
    for rot_4d, poses in ORACLE_CASES:
        units, span = _oracle_units(rot_4d, poses)
        print("flow oracle float32 vs C oracle, rot_4d=%s poses=%s: %.2f units (max |flow| %.1f px)" % (rot_4d, poses, units, span))
        if poses[0] != poses[1] or rot_4d:
            assert span > 1.0, "the case should have motion to compare"
        worst = max(worst, units)
    assert worst <= 64.0, "the oracle is wrong: %.1f units" % worst
    assert worst <= 2.0 * MEASURED_UNITS, "worst deviation %.2f units, measured %.2f when the test was written" % (worst, MEASURED_UNITS)


def test_oracle_zero_cases_and_raw_mode():
    """One camera and equal timestamps: exactly 0; plain 4D with one camera: exactly 0; raw parameters give the activated ones' flow."""
    s0, s1 = fc.pair(257, True, ("rig0", "rig0"), t1=fc.T0)
    par = fc.params_of(s0, raw=False)
    assert not fo.gaussian_flow(*fc.cam_args(s0, s1), *[par[n] for n in fo.NAMES], rot_4d=True, raw=False).any()
    s0, s1 = fc.pair(257, False, ("rig0", "rig0"))
    assert not fo.gaussian_flow(*fc.cam_args(s0, s1), *[par[n] for n in fo.NAMES], rot_4d=False, raw=False).any()
    s0, s1 = fc.pair(257, True, ("rig0", "rig1"))
    act, raw = fc.params_of(s0, raw=False), fc.params_of(s0, raw=True)
    a = fo.gaussian_flow(*fc.cam_args(s0, s1), *[act[n] for n in fo.NAMES], rot_4d=True, raw=False, scaling_modifier=0.7)
    b = fo.gaussian_flow(*fc.cam_args(s0, s1), *[raw[n] for n in fo.NAMES], rot_4d=True, raw=True, scaling_modifier=0.7)
    assert float((a - b).abs().max()) <= 1e-4 and float(a.abs().max()) > 1.0     # (log / exp of float32 scales in between)
    # a Gaussian behind the target camera: flow 0 and no gradient
    behind = act["means3D"].clone()
    behind[0] = torch.tensor([0.0, 0.0, -50.0])
    leaves = {n: act[n].double().requires_grad_(True) for n in fo.NAMES}
    leaves["means3D"] = behind.double().requires_grad_(True)
    f = fo.gaussian_flow(*fc.cam_args(s0, s1), *[leaves[n] for n in fo.NAMES], rot_4d=True, raw=False)
    f.sum().backward()
    assert not f[0].any() and all(not leaves[n].grad[0].any() for n in fo.NAMES) and bool(leaves["means3D"].grad[1].any())


def test_c_entries_check_their_arguments_without_touching_the_gpu():
    from fdgs import _capi
    lib = _capi.lib
    assert {"fdgs_gaussian_flow_forward", "fdgs_gaussian_flow_backward"} <= set(_capi.EXPORTED)
    NOT_NULL = 256   # never dereferenced: every call below is turned away first

    def fresh(rot_4d=1):
        a = _capi.FdgsFlowIn()
        assert a.struct_size == C.sizeof(_capi.FdgsFlowIn)
        a.P, a.W, a.H, a.rot_4d, a.gaussian_dim, a.raw_params, a.scale_modifier = 10, 64, 48, rot_4d, 4, 1, 1.0
        for f in ("means3D", "ts", "scales", "scales_t", "rotations", "rotations_r", "viewmatrix", "projmatrix"):
            setattr(a, f, NOT_NULL)
        return a

    grads = _capi.FdgsFlowGrads()
    assert grads.struct_size == C.sizeof(_capi.FdgsFlowGrads)

    def both(a, what):
        rc = lib.fdgs_gaussian_flow_forward(C.byref(a), NOT_NULL, None)
        assert rc == 1 and "fdgs_gaussian_flow_forward" in _capi.last_error() and what in _capi.last_error(), _capi.last_error()
        rc = lib.fdgs_gaussian_flow_backward(C.byref(a), NOT_NULL, 1.0, C.byref(grads), None)
        assert rc == 1 and "fdgs_gaussian_flow_backward" in _capi.last_error() and what in _capi.last_error(), _capi.last_error()

    assert lib.fdgs_gaussian_flow_forward(None, NOT_NULL, None) == 1 and "NULL" in _capi.last_error()
    assert lib.fdgs_gaussian_flow_backward(None, NOT_NULL, 1.0, C.byref(grads), None) == 1 and "NULL" in _capi.last_error()
    a = fresh()
    a.struct_size -= 4
    both(a, "struct_size")
    a = fresh()
    a.P = -1
    both(a, "P must not be negative")
    for w, h in ((0, 48), (64, 0), (-3, 48)):
        a = fresh()
        a.W, a.H = w, h
        both(a, "W and H")
    for f in ("means3D", "viewmatrix", "projmatrix"):
        a = fresh()
        setattr(a, f, None)
        both(a, f)
    for f in ("ts", "scales", "scales_t", "rotations", "rotations_r"):   # rot_4d without the 4D tensors
        a = fresh()
        setattr(a, f, None)
        both(a, "rot_4d needs")
    a = fresh()
    a.viewmatrix_to = NOT_NULL        # only one of the target matrices
    both(a, "come together")
    a = fresh()
    a.gaussian_dim = 3                # rot_4d on a 3D model
    both(a, "gaussian_dim")
    a = fresh()
    assert lib.fdgs_gaussian_flow_forward(C.byref(a), None, None) == 1 and "flows" in _capi.last_error()
    assert lib.fdgs_gaussian_flow_backward(C.byref(a), None, 1.0, C.byref(grads), None) == 1 and "dL_dflows" in _capi.last_error()
    assert lib.fdgs_gaussian_flow_backward(C.byref(a), NOT_NULL, 1.0, None, None) == 1 and "out" in _capi.last_error()
    grads.struct_size += 8
    assert lib.fdgs_gaussian_flow_backward(C.byref(a), NOT_NULL, 1.0, C.byref(grads), None) == 1 and "fdgs_flow_grads" in _capi.last_error()
    grads.struct_size -= 8
    # no Gaussians: nothing to do, whatever the pointers; a backward with no output asked for: nothing to do either
    a = fresh()
    a.P = 0
    a.means3D = None
    assert lib.fdgs_gaussian_flow_forward(C.byref(a), None, None) == 0
    assert lib.fdgs_gaussian_flow_backward(C.byref(a), None, 1.0, C.byref(grads), None) == 0
    a = fresh()
    assert lib.fdgs_gaussian_flow_backward(C.byref(a), NOT_NULL, 1.0, C.byref(grads), None) == 0   # every output NULL
    assert lib.fdgs_version() == _capi.FDGS_VERSION == 502


def test_flow_to_is_keyword_only_and_defaults_to_none():
    from fdgs.flow import gaussian_flow
    from fdgs.fused import render_raw
    from fdgs.gaussian_renderer import render
    for fn in (render, render_raw):
        p = inspect.signature(fn).parameters["flow_to"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    sig = inspect.signature(gaussian_flow).parameters
    assert list(sig)[:8] == ["cam", "cam_to", "means3D", "ts", "scales", "scales_t", "rotations", "rotations_r"]
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("rot_4d", "gaussian_dim", "raw", "scaling_modifier"))
    assert sig["scaling_modifier"].default == 1.0


def test_python_argument_errors():
    from fdgs.flow import gaussian_flow
    s0, s1 = fc.pair(8, True, ("rig0", "rig1"))
    par = fc.params_of(s0, raw=False)
    cam, cam_to = fc.Cam(s0), fc.Cam(s1)
    with pytest.raises(RuntimeError, match="GPU"):
        gaussian_flow(cam, cam_to, *[par[n] for n in fo.NAMES], rot_4d=True, gaussian_dim=4, raw=False)
    empty = gaussian_flow(cam, cam_to, par["means3D"][:0], None, None, None, None, None, rot_4d=False, gaussian_dim=3, raw=False)
    assert empty.shape == (0, 2)


# ---- the analytic float64 statement, the per-element bar and its K (tests/flow_oracle.py, tests/flow_cases.py) ----

def _autograd(case):
    b = fc.build(case)
    scale = float(np.float32(fc.SCALE))
    flow, g = fo.flow_with_grads(*b["cam"], b["par"], b["dL"].double() * scale, **fc.settings(case))
    return dict({n: g[n].numpy() for n in fo.NAMES}, flows=flow.numpy())


@pytest.mark.parametrize("case", fc.CASES, ids=lambda c: c.name)
def test_analytic_statement_is_float64_autograd(case):
    """Without a plant the hand-written backward is float64 autograd of the forward statement, element by element, to 1e-11 relative.
    Relative to what the element is made of: max(|element|, 2^23 sens_e), the size of its first-order terms in the inputs.  Two float64
    evaluations of a sum agree to 2^-53 of its TERMS, not of the sum: over the cases' 10^5 elements some are small against their terms
    by chance or by construction (one camera: g_0 + g_1), and relative to the element alone the two statements differ by up to 4e-8
    (hard_act_p1000 scales_t, temporal scale 60; 1.2e-10 on the generic two-camera cases) whichever is called the reference.  The
    temporal scale of 60 cancels by structure (w does not depend on it to 1e-7), which no first-order term in the inputs sees: for
    scales_t the size is also at least that of the two routes it is the difference of (flow_oracle.analytic's "scales_t_terms")."""
    f64, sens = fc.oracle(case)
    ref = _autograd(case)
    worst_lit, worst = 0.0, 0.0
    for k in fo.OUTPUTS:
        a, r = f64[k].reshape(case.P, -1), ref[k].reshape(case.P, -1)
        d = np.abs(a - r)
        size = np.maximum(np.maximum(np.abs(a), np.abs(r)), 2.0 ** 23 * sens[k].reshape(case.P, -1))
        if k == "scales_t" and case.rot_4d:
            size = np.maximum(size, f64["scales_t_terms"].reshape(case.P, 1))
        assert (size[d > 0] > 0).all(), k
        with np.errstate(all="ignore"):
            lit = np.where(d > 0, d / np.maximum(np.abs(a), np.abs(r)), 0.0)
            rel = np.where(d > 0, d / size, 0.0)
        worst_lit, worst = max(worst_lit, float(lit.max())), max(worst, float(rel.max()))
        assert rel.max() <= 1e-11, "%s %s: element %s differs by %.3g of its terms" % (case.name, k, np.unravel_index(rel.argmax(), rel.shape), rel.max())
    print("%s: analytic vs autograd, worst %.3g of the terms, %.3g of the element itself" % (case.name, worst, worst_lit))


@pytest.mark.parametrize("case", [c for c in fc.CASES if c.family == "hard"], ids=lambda c: c.name)
def test_every_population_is_present(case):
    f64, _ = fc.oracle(case)
    got = fc.assert_populations(case, f64)
    print(case.name, got)
    placed = fc.build(case)["placed"]
    assert set(fc.need(case)) - {"dl_zero", "dl_one", "dl_big"} == set(placed)
    for c in fc.CASES:
        assert c.P <= 1000 and (c.family == "hard") == bool(fc.need(c))


@pytest.fixture(scope="module")
def r32():
    """{family: {tensor: (r32, case, element)}}: the float32 statement's worst ratio over the family's cases."""
    worst = {}
    for case in fc.CASES:
        f64, sens = fc.oracle(case)
        f32 = fc.float32_statement(case)
        assert np.array_equal(f32["ok"], f64["ok"]), case.name
        for k, (r, at) in fc.ratios(f32, f64, sens).items():
            w = worst.setdefault(case.family, {})
            if r > w.get(k, (-1.0,))[0]:
                w[k] = (r, case.name, tuple(int(i) for i in at))
    return worst


def test_float32_statement_pins_K(r32):
    """K = 4 * r32 per output tensor and family, from the float32 statement on the CPU alone."""
    assert set(r32) == set(fc.K) == {"generic", "hard"}
    for fam in sorted(r32):
        assert set(r32[fam]) == set(fc.K[fam]) == set(fo.OUTPUTS)
        for k in fo.OUTPUTS:
            r, name, at = r32[fam][k]
            print("r32 %-8s %-12s %12.4g  (%s, element %s)   K = %g" % (fam, k, r, name, at, fc.K[fam][k]))
            assert np.isfinite(r) and r > 0.0
            assert abs(fc.K[fam][k] - 4.0 * r) <= fc.K_TOLERANCE * fc.K[fam][k], \
                "flow_cases.K[%r][%r] = %g drifted from 4 * r32 = %g" % (fam, k, fc.K[fam][k], 4.0 * r)


def _flags(case, plant):
    """{tensor: number of elements beyond K times their bar} of the float64 statement with ``plant``, rounded to float32."""
    f64, sens = fc.oracle(case)
    b = fc.build(case)
    bad = fo.analytic(*b["cam"], b["par"], b["dL"], scale=fc.SCALE, plant=plant, **fc.settings(case))
    hits = {}
    for k in fo.OUTPUTS:
        n = len(co.flagged(bad[k].astype(np.float32), f64[k], sens[k], fc.K[case.family][k]))
        if n:
            hits[k] = n
    return hits


def _old_bar_passes(case, plant):
    """Does ``plant`` pass the bar the gradients had before, 1e-4 * max(1, max|ref|) on the maximum over a tensor's elements?"""
    f64, _ = fc.oracle(case)
    b = fc.build(case)
    bad = fo.analytic(*b["cam"], b["par"], b["dL"], scale=fc.SCALE, plant=plant, **fc.settings(case))
    return all(np.abs(bad[n].astype(np.float32) - f64[n]).max() <= 1e-4 * max(1.0, np.abs(f64[n]).max()) for n in fo.NAMES)


PLANT_GENERIC = "raw_p1000_two_mod0.7"
PLANT_HARD = "hard_raw_p257"


def test_the_projection_term_of_the_normalisation_backward_is_zero_here():
    """Why "no_proj" cannot be flagged: w is homogeneous of degree 0 in either quaternion, so q . g = 0 and the term q (q . g) that
    act_normalize_bwd subtracts is rounding.  With and without it the float64 statement is the same to 1e-11 of the element's terms."""
    for name in (PLANT_GENERIC, PLANT_HARD):
        case = fc.BY_NAME[name]
        f64, sens = fc.oracle(case)
        b = fc.build(case)
        bad = fo.analytic(*b["cam"], b["par"], b["dL"], scale=fc.SCALE, plant="no_proj", **fc.settings(case))
        for k in fo.OUTPUTS:
            size = np.maximum(np.abs(f64[k]), 2.0 ** 23 * sens[k])
            d = np.abs(bad[k] - f64[k])
            assert (d <= 1e-11 * size).all(), (name, k, float((d / np.maximum(size, 1e-300)).max()))


@pytest.mark.parametrize("plant", [p for p in fo.PLANTS if p not in fo.UNOBSERVABLE_PLANTS])
def test_planted_errors(plant):
    """The float64 statement with one wrong term stands in for a kernel with that bug: at the bar the GPU tests use it is flagged on a
    generic case, and a plant in a raw-only or 4D-only term on the hard case too; the unplanted statement, rounded to float32, never."""
    cases = [fc.BY_NAME[PLANT_GENERIC]] + ([fc.BY_NAME[PLANT_HARD]] if plant in fo.RAW_PLANTS + fo.ROT4D_PLANTS else [])
    for case in cases:
        assert case.raw and case.rot_4d and case.mod != 1.0
        assert not _flags(case, None), case.name
        hits = _flags(case, plant)
        print("%s on %s: flagged %r; the old max-norm bar %s" % (plant, case.name, hits, "passes it" if _old_bar_passes(case, plant) else "catches it"))
        assert hits, "%s: the planted error passes the bar on every tensor of %s" % (plant, case.name)
