"""GPU: the forward preprocess -- preprocess_fwd_kernel<0/1/2>, colour_batch_kernel, reachable_rect (preprocess_fwd.hip) and
gaussian_at_time (fdgs_math.h) -- against the float64 oracle of tests/preprocess_oracle.py, Gaussian by Gaussian, on the directed
cases of tests/preprocess_cases.py (its docstring lists the populations; tests/test_preprocess_oracle_host.py pins the oracle, the
flags and the constants K on the CPU, from the port alone).

  test_forward_vs_f64   per case and view.  Decisions (alive, radius, tile count, rectangle read off the tile lists, clamp bits) equal
                        float64's for every Gaussian none of whose thresholded quantities is flagged; a flagged one equals the port
                        oracle bit for bit (radius, tile count, clamp bits, depth and position bits), the contract of the file's header.
                        Floats: every element |hip - f64| <= K_tensor * (4 ulp32 |f64_e| + sens_e), no element exempt.  Culled
                        Gaussians: exact zeros, and every output of the geometry buffer is written (the scratch is pre-filled with a
                        pattern the kernels cannot produce).
  test_paths_tied       one launch (PART 0) against the split forward (PART 1 + PART 2) and against colour_batch_kernel over 1, 2, 8
                        and 9 views (crosses COLOUR_BATCH_MAX), bit for bit; tile_cull on against off for everything but the lists.
  test_reachable_rect   every (Gaussian, tile) instance tile_cull drops stays below the blend's alpha threshold on every pixel centre
                        of the tile in float64, with the conic as stored; a Gaussian at or above 1/255 keeps the tile of its mean.
  test_alignment        P in {61, 62, 63, 257}: the same scene from separately allocated tensors and from slices of one flat buffer
                        laid out as layout.SEGMENTS (rotations / rotations_r 4, 8, 12 bytes off 16, flow_2d 4 off 8): forward,
                        backward_finish on hand-written accumulator records (into an unaligned sink, overwrite and accumulate) and
                        camera_backward are bit-identical.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_oracle as co  # noqa: E402
import preprocess_cases as pc  # noqa: E402
import preprocess_oracle as po  # noqa: E402
from util import collect_forward, native_args_fwd, run_oracle, scene_to_device  # noqa: E402

pytestmark = pytest.mark.gpu
PATTERN = 0xAB
BIT_KEYS = ("radii", "tiles_touched", "depths", "cov3D", "out_means3D", "covs_com", "means2D", "conic_opacity", "rgb", "rec_depth", "rec_flow",
            "clamped_bits")


def device_scene(built, v, dev):
    """The view's scene on the device; ``sh_off``: the coefficient tensor that many floats off its 16-byte alignment."""
    sc = scene_to_device(pc.view_scene(built, v), dev)
    off = built["case"].sh_off
    if off and sc.get("shs") is not None:
        buf = torch.zeros(sc["shs"].numel() + 4, dtype=torch.float32, device=dev)
        sh = buf[off:off + sc["shs"].numel()].view(sc["shs"].shape)
        sh.copy_(sc["shs"])
        assert sh.data_ptr() % 16 == 4 * off and sh.is_contiguous()
        sc["shs"] = sh
    return sc


def forward(sc, case, patterned=False, **kw):
    from fdgs import _capi
    from fdgs.gaussian_renderer.diff_gaussian_rasterization import _C
    keep = _capi.scratch
    if patterned:   # the binding's scratch allocator, pre-filled: what the kernels leave of the pattern was never written
        _capi.scratch = lambda nbytes, dev, floor=0: torch.full((max(int(nbytes), floor),), PATTERN, dtype=torch.uint8, device=dev)
    try:
        res = _C.rasterize_gaussians(*native_args_fwd(sc), raw_params=case.raw, **kw)
    finally:
        _capi.scratch = keep
    torch.cuda.synchronize()
    return collect_forward(res, case.P, case.W, case.H)


def lists_of(hip, P, W):
    """(tile x, tile y) of every listed instance per Gaussian -> (count [P], rect [P,4] of the listed tiles, zeros where none)."""
    gx = (W + 15) // 16
    g, t = hip["point_list"].astype(np.int64), hip["tile_keys"].astype(np.int64)
    cnt = np.bincount(g, minlength=P)
    rect = np.zeros((P, 4), np.int64)
    big = 1 << 30
    for col, val, red in ((0, t % gx, np.minimum), (1, t // gx, np.minimum), (2, t % gx + 1, np.maximum), (3, t // gx + 1, np.maximum)):
        acc = np.full(P, big if red is np.minimum else -big)
        red.at(acc, g, val)
        rect[:, col] = np.where(cnt > 0, acc, 0)
    return cnt, rect


def port_of(built, v, dev):
    """The port's forward; a raw case gets the kernels' OWN activations (fdgs_debug_activations), so that a flagged decision is compared
    on the same fp32 inputs."""
    from fdgs import _capi
    scene = pc.view_scene(built, v)
    act = None
    if scene.get("raw"):
        g = lambda k: None if scene.get(k) is None else scene[k].to(dev)   # noqa: E731
        outs = _capi.debug_activations(g("opacities"), g("scales"), g("scales_t"), g("rotations"), g("rotations_r"))
        torch.cuda.synchronize()
        act = [None if t is None else t.cpu().numpy() for t in outs]
    ref, _ = run_oracle(pc.activated(scene, act), None, kind="port")
    return ref


@pytest.fixture(scope="module")
def ratios():
    rep = {}
    yield rep
    print("\nHIP worst ratio per tensor: " + json.dumps({k: float("%.4g" % v) for k, v in sorted(rep.items())}))


@pytest.mark.parametrize("name", [c.name for c in pc.CASES])
def test_forward_vs_f64(name, gpu_device, ratios):
    case = pc.BY_NAME[name]
    built = pc.build(case)
    P, W, H = case.P, case.W, case.H
    for v in range(len(case.poses)):
        sc = device_scene(built, v, gpu_device)
        hip = forward(sc, case, patterned=True)
        inp = pc.oracle_inputs(pc.view_scene(built, v))
        base, sens = po.sensitivity(inp, seed=v)
        fl = po.flags(inp, base, sens)
        if v == 0:
            print(name, {k: n for k, n in pc.assert_populations(case, inp, base, fl, built["planted"]).items() if n})
        where = "%s view %d" % (name, v)
        alive = hip["radii"] > 0
        # ---- every output of the geometry buffer was written ----
        for k in ("depths", "cov3D", "tiles_touched", "clamped_bits", "means2D", "conic_opacity", "rgb", "rec_depth", "rec_flow"):
            raw = np.ascontiguousarray(hip[k]).view(np.uint8)
            word = raw.reshape(-1, hip[k].dtype.itemsize)
            assert not (word == PATTERN).all(1).any(), "%s: %s has elements the kernel never wrote" % (where, k)
        # ---- decisions ----
        cnt, lrect = lists_of(hip, P, W)
        ok = ~fl["geo"]
        for what, got, want in (("alive", alive, base["alive"]), ("radius", hip["radii"], base["radius"]),
                                ("tile count", hip["tiles_touched"].astype(np.int64), base["tiles"]), ("listed instances", cnt, base["tiles"])):
            bad = np.nonzero(ok & (np.asarray(got) != want))[0]
            assert not len(bad), "%s: %s differs from float64 on unflagged Gaussians %r (hip %r, f64 %r)" % (where, what, bad[:8], np.asarray(got)[bad[:8]], want[bad[:8]])
        bad = np.nonzero(ok & (lrect != base["rect"]).any(1))[0]
        assert not len(bad), "%s: rectangle differs from float64 on unflagged Gaussians %r (hip %r, f64 %r)" % (where, bad[:8], lrect[bad[:8]], base["rect"][bad[:8]])
        assert np.array_equal(cnt, hip["tiles_touched"].astype(np.int64)), where + ": listed instances != tiles_touched"
        both = alive & base["alive"]
        if case.M > 0:
            m = both[:, None] & ~fl["rgb"]
            bad = np.nonzero((m & (hip["clamped"].astype(bool) != base["clamped"])).any(1))[0]
            assert not len(bad), "%s: clamp bits differ from float64 on unflagged Gaussians %r" % (where, bad[:8])
        # ---- flagged: the port oracle, bit for bit ----
        flagged = fl["geo"] | fl["rgb"].any(1)
        if flagged.any():
            ref = port_of(built, v, gpu_device)
            f = flagged
            assert np.array_equal(hip["radii"][f], ref["radii"][f]), "%s: radius of a flagged Gaussian differs from the port's: %r vs %r" % (where, hip["radii"][f], ref["radii"][f])
            assert np.array_equal(hip["tiles_touched"][f], ref["tiles_touched"][f]), where + ": tile count of a flagged Gaussian differs from the port's"
            fa = f & (ref["radii"] > 0)
            assert np.array_equal(hip["depths"][fa].view(np.uint32), ref["depths"][fa].view(np.uint32)), where + ": depth bits of a flagged Gaussian"
            assert np.array_equal(hip["means2D"][fa].view(np.uint32), ref["means2D"][fa].view(np.uint32)), where + ": position bits of a flagged Gaussian"
            if case.M > 0:
                assert np.array_equal(hip["clamped"][fa], ref["clamped"][fa]), where + ": clamp bits of a flagged Gaussian differ from the port's"
        # ---- floats, element by element ----
        got = {"out_means3D": hip["out_means3D"], "cov3D": hip["cov3D"], "pix": hip["means2D"], "conic": hip["conic_opacity"][:, 0:3],
               "opacity": hip["conic_opacity"][:, 3], "depth": hip["depths"], "rgb": hip["rgb"]}
        for k in po.FLOATS:
            # out_means3D and cov3D are written for culled Gaussians too (gaussian_at_time's values): compared wherever the temporal
            # cull agrees; the others where the Gaussian is alive on both sides (a disagreement is a flagged decision, held above)
            sel = both if k not in ("out_means3D", "cov3D") else ~fl["marg"]
            if not sel.any():
                continue
            assert np.isfinite(got[k][sel]).all(), "%s: %s has non-finite elements" % (where, k)
            r, at = pc.worst(got[k][sel], base[k][sel], co.core_bar(base[k][sel], sens[k][sel]))
            ratios[k] = max(ratios.get(k, 0.0), r)
            gi = int(np.nonzero(sel)[0][at[0]])
            assert r <= pc.K[k], "%s: %s of Gaussian %d element %s: |hip - f64| = %.3g of (4 ulp32 + sens); K = %g (hip %r, f64 %r)" % (
                where, k, gi, at[1:], r, pc.K[k], got[k][gi], base[k][gi])
        assert np.array_equal(hip["rec_depth"].view(np.uint32), hip["depths"].view(np.uint32)), where + ": the record's depth word"
        assert np.array_equal(hip["covs_com"].view(np.uint32), hip["cov3D"].view(np.uint32)), where + ": covs_com"
        assert np.array_equal(hip["rec_flow"].view(np.uint32), pc.view_scene(built, v)["flow_2d"].numpy().view(np.uint32)), where + ": the record's flow words"
        # ---- culled Gaussians: exact zeros ----
        dead = ~alive
        for k in ("radii", "tiles_touched", "depths", "means2D", "conic_opacity", "rgb", "clamped_bits"):
            assert not np.ascontiguousarray(hip[k][dead]).view(np.uint8).any(), "%s: %s of a culled Gaussian is not exactly zero" % (where, k)
        assert not cnt[dead].any() and not lrect[dead].any(), where + ": a culled Gaussian is listed"


def _same_bits(a, b, what, keys=BIT_KEYS):
    for k in keys:
        assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), "%s: %s differs" % (what, k)


@pytest.mark.parametrize("name", pc.TIED_CASES)
def test_paths_tied(name, gpu_device):
    from fdgs.gaussian_renderer.diff_gaussian_rasterization import _C
    case = pc.BY_NAME[name]
    built = pc.build(case)
    sc0 = device_scene(built, 0, gpu_device)
    # nine views of the same Gaussians: the case's poses in turn, own timestamps
    views = []
    for v in range(9):
        cam = {k: (t.to(gpu_device) if isinstance(t, torch.Tensor) else t) for k, t in built["views"][v % len(built["views"])].items()}
        views.append(dict(sc0, **dict(cam, timestamp=pc.TIMESTAMP + 0.07 * v)))
    one = [forward(sc, case) for sc in views]
    assert sum(int((o["radii"] > 0).sum()) for o in one) > 0
    lists = ("point_list", "tile_keys", "ranges")
    split = forward(views[0], case, split_colour=True)
    _same_bits(one[0], split, name + ": split forward (PART 1 + PART 2) against one launch", BIT_KEYS + lists)
    for nv in (1, 2, 8, 9):
        hs = _C.preprocess_batch([native_args_fwd(sc) for sc in views[:nv]], raw_params=case.raw)
        for v in range(nv):
            res = _C.rasterize_gaussians(*native_args_fwd(views[v]), raw_params=case.raw, preprocessed=hs[v])
            torch.cuda.synchronize()
            got = collect_forward(res, case.P, case.W, case.H)
            _same_bits(one[v], got, "%s: colour_batch_kernel over %d views, view %d, against one launch" % (name, nv, v), BIT_KEYS + lists)
    cull = forward(views[0], case, tile_cull=True)
    _same_bits(one[0], cull, name + ": tile_cull on against off")


@pytest.mark.parametrize("name", pc.REACH_CASES)
def test_reachable_rect(name, gpu_device):
    """The bar is tests/test_gpu_block_cull.py's float64 bar with its margin of 1e-4 on the safe side: a dropped instance must stay
    BELOW (1/255)(1 - 1e-4) on every pixel centre of its tile.  A Gaussian whose effective opacity is itself below 1/255 is listed
    nowhere because alpha <= opacity < 1/255 on every pixel (the blend's own test, forward.cu:590); for those the statement checked is
    that one, in exact arithmetic on the stored fp32 opacity, since an opacity one fp32 step below 1/255 is within 1e-4 of it."""
    case = pc.BY_NAME[name]
    built = pc.build(case)
    W, H, P = case.W, case.H, case.P
    gx = (W + 15) // 16
    total = 0
    for v in range(len(case.poses)):
        sc = device_scene(built, v, gpu_device)
        off, on = forward(sc, case), forward(sc, case, tile_cull=True)
        inp = pc.oracle_inputs(pc.view_scene(built, v))
        base, sens = po.sensitivity(inp, seed=v)
        fl = po.flags(inp, base, sens)
        key = lambda h: set(zip(h["point_list"].astype(np.int64).tolist(), h["tile_keys"].astype(np.int64).tolist()))   # noqa: E731
        k_off, k_on = key(off), key(on)
        assert k_on <= k_off, name + ": tile_cull lists an instance the reference's rectangle does not hold"
        drop = np.array(sorted(k_off - k_on), np.int64).reshape(-1, 2)
        total += len(drop)
        rec = on["conic_opacity"].astype(np.float64)
        pix = on["means2D"].astype(np.float64)
        third = np.float64(np.float32(1.0) / np.float32(255.0))
        if len(drop):
            g, t = drop[:, 0], drop[:, 1]
            best = np.zeros(len(drop))
            for j in range(16):
                for i in range(16):
                    px, py = (t % gx) * 16 + i, (t // gx) * 16 + j
                    inside = (px < W) & (py < H)
                    dx, dy = pix[g, 0] - px, pix[g, 1] - py
                    power = -0.5 * (rec[g, 0] * dx * dx + rec[g, 2] * dy * dy) - rec[g, 1] * dx * dy
                    alpha = np.where(power > 0, 0.0, np.minimum(0.99, rec[g, 3] * np.exp(np.minimum(power, 0.0))))
                    best = np.maximum(best, np.where(inside, alpha, 0.0))
            faint = rec[g, 3] < third
            bad = np.nonzero(~faint & ~(best < (1.0 / 255.0) * (1.0 - 1e-4)))[0]
            assert not len(bad), "%s view %d: dropped instance (Gaussian %d, tile %d) reaches alpha %g" % (name, v, g[bad[0]], t[bad[0]], best[bad[0]])
            assert (best[faint] < 1.0 / 255.0).all()
        # opacity clearly below 1/255: listed nowhere; at or above, mean on screen: the tile of the mean is kept
        alive = on["radii"] > 0
        cnt = np.bincount(on["point_list"].astype(np.int64), minlength=P)
        below, above = alive & ~fl["opa"] & ~fl["geo"] & (base["opa255"] < 0), alive & ~fl["opa"] & ~fl["geo"] & (base["opa255"] > 0)
        assert not cnt[below].any(), name + ": a Gaussian below 1/255 is listed"
        onscreen = above & (pix[:, 0] >= 0) & (pix[:, 0] <= W - 1) & (pix[:, 1] >= 0) & (pix[:, 1] <= H - 1)
        mt = (np.floor(pix[:, 1] + 0.5).astype(np.int64) // 16) * gx + np.floor(pix[:, 0] + 0.5).astype(np.int64) // 16
        missing = [int(i) for i in np.nonzero(onscreen)[0] if (int(i), int(mt[i])) not in k_on]
        assert not missing, "%s view %d: Gaussians %r lost the tile of their mean" % (name, v, missing[:8])
        assert below.sum() >= 2 and onscreen.sum() >= 8
    assert total > 0, name + ": tile_cull dropped nothing"


def _flat_scene(sc, dev):
    """The scene's parameter tensors as slices of ONE flat buffer laid out as layout.SEGMENTS; flow_2d 4 bytes off 8."""
    from fdgs import layout
    P, M = int(sc["means3D"].shape[0]), int(sc["M"])
    rows = layout.row_floats(M)
    flat = torch.zeros(P * sum(rows), dtype=torch.float32, device=dev)
    assert flat.data_ptr() % 16 == 0
    out, at = dict(sc), 0
    for seg, n in zip(layout.SEGMENTS, rows):
        view = flat[at:at + P * n].view((P,) + layout.tail(seg, M))
        view.copy_(sc[seg.kernel].reshape(view.shape))
        out[seg.kernel] = view
        at += P * n
    fb = torch.zeros(2 * P + 1, dtype=torch.float32, device=dev)
    out["flow_2d"] = fb[1:].view(P, 2)
    out["flow_2d"].copy_(sc["flow_2d"])
    assert out["flow_2d"].data_ptr() % 8 == 4
    assert out["rotations"].data_ptr() % 16 == (28 * P) % 16 and out["rotations_r"].data_ptr() % 16 == (52 * P) % 16
    return out


def _backward(sc, case, fwd_res, acc, dev, unaligned, accumulate):
    """backward_begin, the accumulator overwritten with ``acc``, camera_backward, backward_finish -> (grads by name, camera grads,
    guard words around the rotation sinks)."""
    from fdgs.gaussian_renderer import diff_gaussian_rasterization as dgr
    _C = dgr._C
    P, W, H = case.P, case.W, case.H
    e = torch.Tensor([])
    g = lambda k: sc[k] if sc.get(k) is not None else e  # noqa: E731
    (R, _c, _f, _d, _T, radii, geom, binb, img, _cov, out_means3D) = fwd_res
    shapes = {"dL_dopacity": (P, 1), "dL_dmeans3D": (P, 3), "dL_dts": (P, 1), "dL_dscales": (P, 3), "dL_dscales_t": (P, 1),
              "dL_drotations": (P, 4), "dL_drotations_r": (P, 4)}
    gen = torch.Generator().manual_seed(9)
    sink, bufs = {}, {}
    for k, s in shapes.items():
        n = P * s[1]
        lead = (4 + (7 * P if k == "dL_drotations" else 13 * P) % 4) if (unaligned and k.startswith("dL_drot")) else 4
        # (the prefill of the slice is the same whatever its offset: drawn on its own, between two constant guards)
        body = torch.randn(n, generator=torch.Generator().manual_seed(100 + len(bufs)))
        buf = torch.cat([torch.full((lead,), 7.0), body, torch.full((4,), 7.0)]).to(dev)
        bufs[k] = (buf, lead, n, buf.clone())
        sink[k] = buf[lead:lead + n].view(s)
    if unaligned:
        assert sink["dL_drotations"].data_ptr() % 16 == (28 * P) % 16 and sink["dL_drotations_r"].data_ptr() % 16 == (52 * P) % 16
    gacc, stage = torch.zeros((P, 16), device=dev), torch.zeros((P, 8), device=dev)
    up = (1e-2 * torch.randn(3, H, W, generator=gen)).to(dev)
    pend = _C.backward_begin(
        sc["bg"], sc["means3D"], out_means3D, radii, g("colors_precomp"), g("flow_2d"), sc["opacities"], g("ts"), g("scales"), g("scales_t"),
        g("rotations"), g("rotations_r"), sc["scale_modifier"], g("cov3D_precomp"), sc["prefilter_var"], sc["world_view_transform"],
        sc["full_proj_transform"], sc["tanfovx"], sc["tanfovy"], up, None, None, None, g("shs"), sc["sh_degree"], sc["sh_degree_t"],
        sc["camera_center"], sc["timestamp"], sc["time_duration"], sc["rot_4d"], sc["gaussian_dim"], sc["force_sh_3d"], geom, R, binb, img,
        False, raw_params=case.raw, grad_out=sink, accumulate=accumulate, grad_accum=gacc, sh_stage=stage)
    torch.cuda.synchronize()
    gacc.zero_()
    gacc[:, 0:12] = torch.from_numpy(acc).to(dev)
    _C.sh_backward_batch([pend])
    cam = _C.camera_backward(pend)
    grads = _C.backward_finish(pend)
    torch.cuda.synchronize()
    # (dL_dsh is deferred with sh_stage: these calls leave it untouched, the stage records stand for it)
    out = {n: (None if t is None else t.cpu().numpy().copy()) for n, t in zip(dgr._GRADS, grads) if n != "dL_dsh"}
    out["sh_stage"] = stage.cpu().numpy().copy()
    for k, (buf, lead, n, before) in bufs.items():
        assert torch.equal(buf[:lead], before[:lead]) and torch.equal(buf[lead + n:], before[lead + n:]), "the elements around the %s sink were written" % k
    return out, {k: t.cpu().numpy().copy() for k, t in cam.items()}


@pytest.mark.parametrize("P", [61, 62, 63, 257])
def test_alignment(P, gpu_device):
    from fdgs.gaussian_renderer.diff_gaussian_rasterization import _C
    case = pc.Case("align", P, 4, True, 3, 2, 48, ("marg", "near"), raw=True, seed=40 + P)
    built = pc.build(case)
    apart = scene_to_device(pc.view_scene(built, 0), gpu_device)
    flat = _flat_scene(apart, gpu_device)
    rng = np.random.default_rng(P)
    acc = rng.standard_normal((P, 12)).astype(np.float32)
    results = []
    for sc, un in ((apart, False), (flat, True)):
        res = _C.rasterize_gaussians(*native_args_fwd(sc), raw_params=True)
        torch.cuda.synchronize()
        fwd = collect_forward(res, P, case.W, case.H)
        per_mode = []
        for accumulate in (False, True):
            per_mode.append(_backward(sc, case, res, acc, gpu_device, un, accumulate))
        results.append((fwd, per_mode))
    (f0, b0), (f1, b1) = results
    assert (f0["radii"] > 0).sum() >= P // 2
    _same_bits(f0, f1, "P = %d: forward from the flat bucket against separately allocated tensors" % P,
               BIT_KEYS + ("point_list", "tile_keys", "ranges"))
    for mode, ((g0, c0), (g1, c1)) in zip(("overwrite", "accumulate"), zip(b0, b1)):
        for k in g0:
            if g0[k] is not None:
                assert g0[k].tobytes() == g1[k].tobytes(), "P = %d, %s: %s differs between the aligned and the unaligned run" % (P, mode, k)
        assert np.abs(g0["dL_drotations"]).sum() > 0 and np.abs(g0["dL_drotations_r"]).sum() > 0
        for k in c0:
            assert c0[k].tobytes() == c1[k].tobytes(), "P = %d, %s: camera gradient %s differs" % (P, mode, k)
