"""GPU: blend_fwd_kernel<FLOW> and blend_bwd_kernel<AUX> (blend_fwd.hip, blend_bwd.hip, blend_common.h) against the float64 oracle of
tests/blend_oracle.py, element by element, on the cases of tests/blend_cases.py (its CASES table says which path each exists for).

Per case and forward mode (default lists, tile_cull, sparse_lists):  1. the HIP forward;  2. the float64 forward on the records and lists
of THIS forward;  3. the cliff flags;  4. per upstream variant, ``backward_begin`` (stage_mask 5: the blend backward alone) on a zeroed
(P, 16) ``grad_accum`` with the upstream images zeroed on the flagged pixels;  5. a synchronize and a read of the records.

Forward: n_contrib equal on every unflagged pixel; final_T and out_T the same bits; colour, depth, flow, T within K * unit; finite; the
flagged share within the cap.  Backward: every one of the 12 words of every Gaussian within K_word * unit, no element exempt; words 12..15
exact zero bits; the whole record exact zero bits for a Gaussian in no list or accepted by no unflagged pixel; colour-only: words 3-5 exact
zero bits; two runs on one forward agree within twice the summation part of the unit; the case's populations are present."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blend_cases as bc  # noqa: E402
import blend_oracle as bo  # noqa: E402
from util import collect_forward, native_args_fwd, scene_to_device  # noqa: E402

pytestmark = pytest.mark.gpu

FWD = [(c.name, m) for c in bc.CASES for m in c.modes]
BWD = [(c.name, m, v) for c in bc.CASES for m in c.modes for v in (bc.VARIANTS if m == "default" else ("colour", "all"))]


@pytest.fixture(scope="module")
def forwards(gpu_device):
    """{(case, mode): the HIP forward (native result, device scene, collected arrays), the float64 forward on it, its populations}:
    computed once, shared by the forward and the backward tests, left unchanged."""
    from fdgs import _capi
    from fdgs.gaussian_renderer.diff_gaussian_rasterization import _C
    cache = {}

    def get(name, mode):
        if (name, mode) in cache:
            return cache[name, mode]
        case = bc.BY_NAME[name]
        sc = scene_to_device(bc.build(case), gpu_device)
        opt = bc.MODES[mode]
        if opt["sparse"]:
            _capi.forward_lazy_status(gpu_device, wait=True)
            _C.rasterize_gaussians(*native_args_fwd(sc), tile_cull=opt["tile_cull"])      # leaves the run-ahead sizes behind
            s0 = _capi.sparse_lists_stats()
            res = _C.rasterize_gaussians(*native_args_fwd(sc), tile_cull=opt["tile_cull"], lazy=True, sparse_lists=True)
            _pend, failed, _rep = _capi.forward_lazy_status(gpu_device, wait=True)
            assert res[0] == -1 and failed == 0 and _capi.sparse_lists_stats()[0] - s0[0] == 1, "the forward did not take sparse lists"
        else:
            res = _C.rasterize_gaussians(*native_args_fwd(sc), tile_cull=opt["tile_cull"])
        fwd = collect_forward(res, sc["P"], case.W, case.H)
        f64 = bo.forward(fwd, fwd["point_list"], fwd["ranges"], case.bg, case.W, case.H)
        cache[name, mode] = {"case": case, "sc": sc, "res": res, "fwd": fwd, "f64": f64, "pops": bc.populations(case, fwd, f64)}
        return cache[name, mode]
    return get


@pytest.fixture(scope="module")
def ratios():
    """HIP's worst |hip - f64| / unit per class over the tests that ran: printed (BASELINE.md section 8 records it)."""
    rep = {}
    yield rep
    print("\nHIP worst ratio per class: " + json.dumps({k: float("%.4g" % v) for k, v in sorted(rep.items())}))


def _hold(rep, label, cls, got, want, unit, keep=None):
    assert np.isfinite(got).all(), "%s: %s has non-finite elements" % (label, cls)
    r = bo.ratio(got, want, unit)
    if keep is not None:
        r = np.where(keep, r, 0.0)
    at = np.unravel_index(int(np.argmax(r)), r.shape) if r.size else ()
    worst = float(r[at]) if r.size else 0.0
    rep[cls] = max(rep.get(cls, 0.0), worst)
    assert worst <= bc.K[cls], "%s: %s element %s: |hip - f64| = %.3g units of %g; K = %g (hip %r, f64 %r)" % (
        label, cls, at, worst, float(unit[at]), bc.K[cls], np.asarray(got).reshape(want.shape)[at], want[at])


@pytest.mark.parametrize("name,mode", FWD)
def test_blend_forward_vs_f64(name, mode, forwards, ratios):
    e = forwards(name, mode)
    case, fwd, f64 = e["case"], e["fwd"], e["f64"]
    label = "%s [%s]" % (name, mode)
    share = bc.assert_flag_cap(case, f64["flagged"])
    ok = ~f64["flagged"]
    bad = int((fwd["n_contrib"].astype(np.int64)[ok] != f64["n_contrib"][ok]).sum())
    assert bad == 0, "%s: n_contrib differs on %d unflagged pixels" % (label, bad)
    assert fwd["final_T"].tobytes() == fwd["out_T"].tobytes(), label + ": final_T and out_T differ"
    _hold(ratios, label, "colour", fwd["out_color"], f64["out_color"], f64["u_color"], ok[None])
    _hold(ratios, label, "depth", fwd["out_depth"], f64["out_depth"], f64["u_depth"], ok)
    _hold(ratios, label, "T", fwd["out_T"], f64["out_T"], f64["u_T"], ok)
    if case.flow:
        _hold(ratios, label, "flow", fwd["out_flow"], f64["out_flow"], f64["u_flow"], ok[None])
    else:
        assert not fwd["out_flow"].view(np.uint32).any(), label + ": FLOW = false: the flow planes are not exact zero bits"
    bc.assert_populations(case, mode, e["pops"])
    print(label, "flagged %.3f %%" % (100 * share), {k: v for k, v in e["pops"].items() if v and not k.startswith(("deep_", "drain_"))})


def _hip_backward(e, up, dev):
    """The blend backward alone on a zeroed accumulator: -> [P,16] float32."""
    from fdgs.gaussian_renderer.diff_gaussian_rasterization import _C
    sc = e["sc"]
    (R, _c, _f, _d, _T, radii, geom, binb, img, _cov, om) = e["res"]
    P = sc["P"]
    z = torch.Tensor([])
    g = lambda k: sc[k] if sc.get(k) is not None else z  # noqa: E731
    d = lambda t: None if t is None else t.to(dev).contiguous()  # noqa: E731
    gacc = torch.zeros((P, 16), dtype=torch.float32, device=dev)
    stage = torch.zeros((P, 8), dtype=torch.float32, device=dev)
    _C.backward_begin(sc["bg"], sc["means3D"], om, radii, g("colors_precomp"), g("flow_2d"), sc["opacities"], z, z, z, z, z, sc["scale_modifier"],
                      g("cov3D_precomp"), sc["prefilter_var"], sc["world_view_transform"], sc["full_proj_transform"], sc["tanfovx"], sc["tanfovy"],
                      d(up["grad_color"]), d(up["grad_depth"]), d(up["grad_alpha"]), d(up["grad_flow"]), z, sc["sh_degree"], sc["sh_degree_t"],
                      sc["camera_center"], sc["timestamp"], sc["time_duration"], sc["rot_4d"], sc["gaussian_dim"], sc["force_sh_3d"], geom, R, binb,
                      img, False, grad_accum=gacc, sh_stage=stage)
    torch.cuda.synchronize()
    return gacc.cpu().numpy()


@pytest.mark.parametrize("name,mode,variant", BWD)
def test_blend_backward_vs_f64(name, mode, variant, forwards, ratios, gpu_device):
    e = forwards(name, mode)
    case, fwd, f64 = e["case"], e["fwd"], e["f64"]
    label = "%s [%s, %s]" % (name, mode, variant)
    bc.assert_flag_cap(case, f64["flagged"])
    bc.assert_populations(case, mode, e["pops"])
    up = bc.mask_upstream(bc.upstream(case, variant), f64["flagged"])
    n = lambda t: None if t is None else t.numpy()  # noqa: E731
    want = bo.backward(fwd, fwd["point_list"], fwd["ranges"], case.bg, case.W, case.H, fwd["n_contrib"], fwd["final_T"], n(up["grad_color"]),
                       n(up["grad_depth"]), n(up["grad_alpha"]), n(up["grad_flow"]), ignore=f64["flagged"])
    runs = [_hip_backward(e, up, gpu_device) for _ in range(2)]
    cls = np.asarray(bo.WORD_CLASS)
    for got in runs:
        assert not got[:, 12:16].view(np.uint32).any(), label + ": words 12..15 are not exact zero bits"
        dead = ~want["accepted"]
        nz = np.nonzero(dead & got.view(np.uint32).any(1))[0]
        assert nz.size == 0, "%s: the records of Gaussians no unflagged pixel accepts are not exact zero bits: %r" % (label, nz[:8].tolist())
        if variant == "colour":
            assert not got[:, 3:6].view(np.uint32).any(), label + ": colour-only: words 3-5 are not exact zero bits"
        for c in sorted(set(bo.WORD_CLASS)):
            w = np.nonzero(cls == c)[0]
            _hold(ratios, label, c, got[:, w], want["words"][:, w], want["unit"][:, w])
    d = np.abs(runs[0][:, 0:12].astype(np.float64) - runs[1][:, 0:12])
    over = d > 2.0 * want["usum"]
    assert not over.any(), "%s: two runs on one forward differ by more than twice the summation unit at %r" % (label, np.argwhere(over)[:4].tolist())
