"""GPU: the per-Gaussian backward kernels -- preprocess_bwd_kernel(_w4) (preprocess_bwd.hip), sh_bwd_batch_kernel and sh_flush_kernel<0>
(sh_bwd.hip, sh_eval.h) -- against the float64 oracle of tests/chain_oracle.py, element by element, on accumulator records the test
writes itself (no blend atomics between the inputs and the kernels under test).  Per case of tests/chain_cases.py (its CASES table
says which path each exists for) and per view:

  1. the HIP forward;  2. ``backward_begin`` (stage_mask 5) with a small real upstream gradient;  3. the view's ``grad_accum`` is
  overwritten with the case's records (words 12..15 zero);  4. ``sh_backward_batch`` -- words 12..15 and the stage records are read;
  5. ``backward_finish`` (stage_mask 2), and ``sh_flush`` over the staged views.

Asserted: every element |hip - f64| <= K_tensor * (4 ulp32 of |f64_e| + sens_e) with chain_cases.K (no element exempt; with several
views or a prefill the fp32 additions join the bar, chain_cases.expected); the chain outputs of culled Gaussians, and the dL_dsh rows,
stage records and hand-over words of SH-dead ones, are exact zeros; ``grad_accum`` is all zero bits on exit; the populations of the
case are there, counted from THIS forward's radii and records.  The pass-through outputs of a culled Gaussian whose record is not zero
(dL_dcolor, dL_dflows, dL_dmean2D.z, dL_dopacity: the blend backward's own sums, which the reference hands through as well) equal the
record -- the oracle says so, at K = 0 for the copies.

The dense ``sh_bwd_kernel`` cannot take hand-written records (stage 1 runs the blend backward first);
tests/test_gpu_api.py::test_sh_backward_paths_bitwise ties it bit for bit to the batch-plus-flush path checked here.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_cases as cc  # noqa: E402
import chain_oracle as co  # noqa: E402
from util import collect_forward, native_args_fwd, scene_to_device  # noqa: E402

pytestmark = pytest.mark.gpu

SINK = {"dL_dopacity": "dL_dopacity", "dL_dmeans3D": "dL_dmean3D", "dL_dts": "dL_dts", "dL_dscales": "dL_dscale",
        "dL_dscales_t": "dL_dscale_t", "dL_drotations": "dL_drot", "dL_drotations_r": "dL_drot_r"}
PER_VIEW = {"dL_dmeans2D": "dL_dmean2D", "dL_dcolors": "dL_dcolor", "dL_dcov3D": "dL_dcov3D", "dL_dflows": "dL_dflows"}
NAMES = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dflows", "dL_dts", "dL_dscales",
         "dL_dscales_t", "dL_drotations", "dL_drotations_r")
CHAIN_OUT = ("dL_dcov3D", "dL_dmean3D", "dL_dts", "dL_dscale", "dL_dscale_t", "dL_drot", "dL_drot_r")


def run_hip_case(built, dev):
    """-> (forwards per view, hip outputs by oracle name, words / stage per view, grad_accum after the last call)."""
    from fdgs import _capi
    from fdgs.gaussian_renderer import diff_gaussian_rasterization as dgr
    _C = dgr._C
    c = built["case"]
    P, W, H, V = c.P, c.W, c.H, c.views
    e = torch.Tensor([])
    fo = dict(dtype=torch.float32, device=dev)
    shapes = {"dL_dopacity": (P, 1), "dL_dmeans3D": (P, 3), "dL_dts": (P, 1), "dL_dscales": (P, 3), "dL_dscales_t": (P, 1),
              "dL_drotations": (P, 4), "dL_drotations_r": (P, 4)}
    sink = {}
    for k, s in shapes.items():
        if built["prefill"] is not None:
            sink[k] = torch.from_numpy(built["prefill"][SINK[k]].reshape(s)).to(dev).contiguous()
        else:
            sink[k] = torch.full(s, float("nan"), **fo)    # every element must be written
    gacc, stage = torch.zeros((V, P, 16), **fo), torch.zeros((V, P, 8), **fo)
    gen = torch.Generator().manual_seed(5)
    up = (1e-2 * torch.randn(3, H, W, generator=gen)).to(dev)
    dgr.set_analytic_sh_gradients(bool(c.analytic))
    try:
        fwds, pends = [], []
        sc0 = scene_to_device(built["scene"], dev)   # the views of a batch share the parameter tensors
        for v in range(V):
            sc = dict(sc0, **built["views"][v])
            g = lambda k: sc[k] if sc.get(k) is not None else e  # noqa: E731
            res = _C.rasterize_gaussians(*native_args_fwd(sc), raw_params=c.raw)
            (R, _c, _f, _d, _T, radii, geom, binb, img, _cov, out_means3D) = res
            fwds.append(collect_forward(res, P, W, H))
            pends.append(_C.backward_begin(
                sc["bg"], sc["means3D"], out_means3D, radii, g("colors_precomp"), g("flow_2d"), sc["opacities"], g("ts"), g("scales"),
                g("scales_t"), g("rotations"), g("rotations_r"), sc["scale_modifier"], g("cov3D_precomp"), sc["prefilter_var"],
                sc["world_view_transform"], sc["full_proj_transform"], sc["tanfovx"], sc["tanfovy"], up, None, None, None, g("shs"),
                sc["sh_degree"], sc["sh_degree_t"], sc["camera_center"], sc["timestamp"], sc["time_duration"], sc["rot_4d"],
                sc["gaussian_dim"], sc["force_sh_3d"], geom, R, binb, img, False, raw_params=c.raw, grad_out=sink,
                accumulate=(v > 0 or c.mode == "accumulate"), grad_accum=gacc[v], sh_stage=stage[v],
                per_view_outputs=(c.mode != "noperview")))
            torch.cuda.synchronize()
            gacc[v].zero_()
            gacc[v][:, 0:12] = torch.from_numpy(built["acc"][v]).to(dev)
        stage.zero_()
        if c.M > 0:
            _C.sh_backward_batch(pends)
        torch.cuda.synchronize()
        words = [gacc[v][:, 12:16].cpu().numpy() for v in range(V)]
        stages = [stage[v].cpu().numpy() for v in range(V)]
        grads = None
        for v in range(V):
            grads = _C.backward_finish(pends[v])
        torch.cuda.synchronize()
        hip = {}
        for n, t in zip(NAMES, grads):
            key = SINK.get(n) or PER_VIEW.get(n)
            if key is not None:
                hip[key] = None if t is None else t.cpu().numpy()
        if c.M > 0:
            dsh = torch.full((P, c.M, 3), float("nan"), **fo)
            _capi.sh_flush(stage.contiguous(), dsh, c.D, c.D_t, c.dim, c.force_sh_3d, bool(c.analytic))
            torch.cuda.synchronize()
            hip["dL_dsh"] = dsh.cpu().numpy()
        return fwds, hip, words, stages, gacc.cpu().numpy()
    finally:
        dgr.set_analytic_sh_gradients(False)


def check_case(case, dev, report):
    built = cc.build(case)
    fwds, hip, words, stages, gacc = run_hip_case(built, dev)
    if case.period:
        # Gaussian i is Gaussian i % period: the forward's records repeat bit for bit, so one period of the oracle covers every element
        for k in ("radii", "out_means3D", "cov3D", "conic_opacity", "clamped"):
            a = np.asarray(fwds[0][k])
            assert a.tobytes() == cc.tile(a[:case.period], case.P, case.period).tobytes(), k
    exp, core, per_view, pops = cc.oracle_case(built, fwds)
    assert not gacc.view(np.uint32).any(), "%s: grad_accum is not all zero bits on exit" % case.name

    def hold(name, got, want, bar, where=""):
        assert np.isfinite(got).all(), "%s: %s%s has non-finite elements" % (case.name, name, where)
        r, at = cc.worst(got, want, bar)
        report[name] = max(report.get(name, 0.0), r)
        K = cc.K[name]
        assert r <= K or (K == 0.0 and r == 0.0), "%s: %s%s element %s: |hip - f64| = %.3g of (4 ulp32 + sens) = %g; K = %g (hip %r, f64 %r)" % (
            case.name, name, where, at, r, float(bar[at]), K, np.asarray(got).reshape(want.shape)[at], want[at])

    for v in range(case.views):
        f64, sens = per_view[v]
        vis = fwds[v]["radii"] > 0
        if case.M > 0:
            live = vis & (np.where(fwds[v]["clamped"] != 0, 0.0, built["acc"][v][:, 0:3]) != 0).any(1)
            hold("sh_words", words[v], f64["sh_words"], co.core_bar(f64["sh_words"], sens["sh_words"]), " (view %d)" % v)
            st = np.where(live[:, None], stages[v], np.concatenate([stages[v][:, 0:4], np.zeros((case.P, 4), np.float32)], axis=1))
            hold("stage", st, f64["stage"], co.core_bar(f64["stage"], sens["stage"]), " (view %d)" % v)
            assert not words[v][~live].any() and not stages[v][~live][:, 0:4].any(), "%s: an SH-dead Gaussian has non-zero hand-over words / stage record" % case.name
        else:
            assert not words[v].any()
    for k in exp:
        if k in ("sh_words", "stage", "dL_dconic") or (k == "dL_dsh" and case.M == 0):
            continue
        if hip.get(k) is None:
            assert case.mode == "noperview" and k in PER_VIEW.values(), (case.name, k)
            continue
        hold(k, hip[k], exp[k], core[k])
    # exact zeros: the chain outputs of a Gaussian culled in every view (no prefill), the dL_dsh row of one SH-dead in every view
    if built["prefill"] is None:
        gone = np.ones(case.P, bool)
        for v in range(case.views):
            gone &= ~(fwds[v]["radii"] > 0)
        assert gone.sum() >= (4 if "culled" in case.need else 0)
        for k in CHAIN_OUT:
            if hip.get(k) is not None:
                assert not hip[k].reshape(case.P, -1)[gone].any(), "%s: %s of a culled Gaussian is not exactly zero" % (case.name, k)
    if case.M > 0:
        dead = np.ones(case.P, bool)
        for v in range(case.views):
            dead &= ~((fwds[v]["radii"] > 0) & (np.where(fwds[v]["clamped"] != 0, 0.0, built["acc"][v][:, 0:3]) != 0).any(1))
        assert not hip["dL_dsh"][dead].any(), "%s: the dL_dsh row of an SH-dead Gaussian is not exactly zero" % case.name
    if case.mode == "noperview":
        assert all(hip[k] is None for k in ("dL_dcolor", "dL_dcov3D", "dL_dflows"))
    return pops


@pytest.fixture(scope="module")
def ratios():
    """HIP's worst |hip - f64| / (4 ulp32 + sens) per tensor over the cases that ran: printed (BASELINE.md records it)."""
    rep = {}
    yield rep
    print("\nHIP worst ratio per tensor: " + json.dumps({k: float("%.4g" % v) for k, v in sorted(rep.items())}))


@pytest.mark.parametrize("name", [c.name for c in cc.CASES])
def test_gaussian_backward_vs_f64(name, gpu_device, ratios):
    pops = check_case(cc.BY_NAME[name], gpu_device, ratios)
    print(name, {k: v for k, v in pops[0].items() if v})


def test_gaussian_backward_w4_variant(gpu_device, ratios):
    """P = 2^20 + 3: launch_preprocess_bwd selects preprocess_bwd_kernel_w4 (the 128-VGPR build of the same body).  rot_4d raw, D = 0,
    512 x 512; one period of 4099 Gaussians repeated, so every one of the 2^20 + 3 Gaussians' elements is compared."""
    check_case(cc.LARGE, gpu_device, ratios)
