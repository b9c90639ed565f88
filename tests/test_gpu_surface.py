"""GPU: fdgs.surface (csrc/tsdf.hip) -- TSDF integration and surface nets against the numpy statement tests/surface_oracle.py.

The bars are those of tests/test_gpu_depth.py (tests/loss_cases.py: MARGIN, VALUE_FLOOR): per element, 4 x the float32 statement's own
distance from the float64 truth, floored at 2e-6; weights, counts and faces are exact.  Voxels the truth flags as sitting on a decision
threshold (at most 2 % of a case, checked on the host) are left out of the integration's comparison.  A bar never looks at a kernel's
output; every test prints its worst ratio error / bar (DESIGN.md records them).  Every output array sits between guard bands."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import surface_cases as sc
import surface_oracle as so
from loss_cases import MARGIN, VALUE_FLOOR

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 64, 12345.0


def _ratio(tag, got, r64, r32, sel=None):
    """The worst |got - truth| / bar over the selected elements, bar = max(VALUE_FLOOR, MARGIN |float32 statement - truth|)."""
    err = np.abs(got.astype(np.float64) - r64)
    ratio = err / np.maximum(VALUE_FLOOR, MARGIN * np.abs(r32.astype(np.float64) - r64))
    if sel is not None:
        ratio = ratio[..., sel]
    return float(ratio.max()) if ratio.size else 0.0


def _guarded(shape, dev, dtype=torch.float32):
    """(the tensor, the buffer it sits in with GUARD sentinels before and after it)."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev).to(dtype)
    body = whole[GUARD:GUARD + n]
    return body.view(shape), whole


def _guards_intact(whole):
    want = torch.tensor(SENTINEL).to(whole.dtype).item()
    return bool((whole[:GUARD] == want).all()) and bool((whole[-GUARD:] == want).all())


def _gpu_volume(vol, dev, fill=True):
    """A TSDFVolume holding ``vol``'s arrays, every array between guard bands; returns (volume, [buffers])."""
    from fdgs import surface
    v = surface.TSDFVolume(vol["origin"], vol["s"], vol["dims"], trunc=vol["trunc"], color=vol["color"] is not None, device=dev)
    wholes = []
    for k in ("tsdf", "weight", "color", "cweight"):
        if vol[k] is None:
            continue
        t, whole = _guarded(vol[k].shape, dev)
        t.copy_(torch.from_numpy(vol[k]))
        setattr(v, k, t)
        wholes.append(whole)
    return v, wholes


def _gpu_views(views, dev):
    t = lambda a, lead: None if a is None else torch.from_numpy(a).to(dev).view((lead,) + a.shape[-2:])  # noqa: E731
    return [{"depth": t(v["depth"], 1), "alpha": t(v["alpha"], 1), "mask": t(v["mask"], 1), "image": t(v["image"], 3), "camera": v["camera"],
             "weight": v["weight"], "alpha_min": v["alpha_min"]} for v in views]


def _arrays(volume):
    return {k: (None if t is None else t.cpu().numpy()) for k, t in volume.arrays().items()}


# ---- 1. integration ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sc.INTEGRATE_CASES))
def test_integrate_against_the_statement(name, gpu_device):
    from fdgs import surface
    vol, views = sc.integrate_case(name)
    r64, r32 = sc.integrate_refs(name)
    volume, wholes = _gpu_volume(vol, gpu_device)
    surface.integrate(volume, _gpu_views(views, gpu_device))
    torch.cuda.synchronize()
    got = _arrays(volume)
    assert all(_guards_intact(w) for w in wholes), "integrate wrote outside an array"
    ok = ~r64["flag"]
    assert 1.0 - ok.mean() <= 0.02
    assert np.array_equal(got["weight"][ok], r64["weight"][ok].astype(np.float32)), "weight differs"
    rt = _ratio("tsdf", got["tsdf"], r64["tsdf"], r32["tsdf"], ok)
    line = "%-7s %d views: tsdf ratio %.3f" % (name, len(views), rt)
    untouched = ok & (r64["weight"] == 0)
    assert not got["tsdf"][untouched].view(np.int32).any() and not got["weight"][untouched].view(np.int32).any()
    if vol["color"] is not None:
        assert np.array_equal(got["cweight"][ok], r64["cweight"][ok].astype(np.float32)), "cweight differs"
        rc = _ratio("color", got["color"], r64["color"], r32["color"], ok)
        line += ", color ratio %.3f" % rc
        none = ok & (r64["cweight"] == 0)
        assert not got["color"][:, none].view(np.int32).any() and not got["cweight"][none].view(np.int32).any()
        assert rc <= 1.0, line
    print(line)
    assert np.isfinite(got["tsdf"]).all() and rt <= 1.0, line


@pytest.mark.parametrize("name", ["full", "chunk"])
def test_one_call_is_bit_identical_to_one_call_per_view_and_to_a_second_run(name, gpu_device):
    from fdgs import surface
    vol, views = sc.integrate_case(name)
    gviews = _gpu_views(views, gpu_device)
    runs = []
    for mode in ("one", "one", "each"):
        volume, _ = _gpu_volume(vol, gpu_device)
        if mode == "one":
            surface.integrate(volume, gviews)
        else:
            for v in gviews:
                surface.integrate(volume, [v])
        torch.cuda.synchronize()
        runs.append(_arrays(volume))
    for k in ("tsdf", "weight", "color", "cweight"):
        assert np.array_equal(runs[0][k].view(np.int32), runs[1][k].view(np.int32)), "second run differs in " + k
        assert np.array_equal(runs[0][k].view(np.int32), runs[2][k].view(np.int32)), "one call per view differs in " + k
    assert (runs[0]["weight"] > 0).any()


# ---- 2. extraction -------------------------------------------------------------------------------------------------------------
def _extract_guarded(volume, min_weight, vcap, fcap, dev, with_arrays=True):
    from fdgs import _capi, surface
    counts = torch.full((2,), -7, dtype=torch.int32, device=dev)
    scratch = torch.empty(max(int(_capi.lib.fdgs_surface_extract_scratch_bytes(*volume.dims)), 256), dtype=torch.uint8, device=dev)
    out = {}
    if with_arrays:
        for k in ("vertices", "normals", "colors"):
            out[k] = _guarded((vcap, 3), dev)
        out["faces"] = _guarded((fcap, 3), dev, torch.int32)
    surface._extract_call(volume, min_weight, counts, scratch, vcap, fcap, **{k: v[0] for k, v in out.items()})
    torch.cuda.synchronize()
    return [int(c) for c in counts.cpu()], out


@pytest.mark.parametrize("dims", sc.EXTRACT_SHAPES, ids=["%dx%dx%d" % d for d in sc.EXTRACT_SHAPES])
@pytest.mark.parametrize("kind", sc.EXTRACT_KINDS)
def test_extract_against_the_statement(kind, dims, gpu_device):
    _check_extract(kind, dims, gpu_device)


@pytest.mark.parametrize("kind", sc.CHUNK_KINDS)
def test_extract_past_a_scan_chunk(kind, gpu_device):
    """266 240 voxels = 1040 workgroup counts per scan, 16 of them behind the first chunk of 1024.  The sphere sits in the middle of
    the volume: its counts reach the totals through the carry.  "random" has vertices and quads in every workgroup: the ranks of
    the last z slice are the carry plus their own."""
    _check_extract(kind, sc.CHUNK_SHAPE, gpu_device)


def _check_extract(kind, dims, gpu_device):
    from fdgs import surface
    vol, mw = sc.extract_case(kind, dims)
    m64, m32 = sc.extract_refs(kind, dims)
    V, F = len(m64["vertices"]), len(m64["faces"])
    volume, wholes = _gpu_volume(vol, gpu_device)
    before = _arrays(volume)
    (nv, nf), _ = _extract_guarded(volume, mw, 0, 0, gpu_device, with_arrays=False)        # count only
    assert (nv, nf) == (V, F)
    (nv, nf), out = _extract_guarded(volume, mw, V, F, gpu_device)
    assert (nv, nf) == (V, F)
    assert all(_guards_intact(w) for _, w in out.values()), "extract wrote outside an output array"
    assert all(_guards_intact(w) for w in wholes) and all(np.array_equal(before[k], v) for k, v in _arrays(volume).items())
    assert np.array_equal(out["faces"][0].cpu().numpy(), m32["faces"]) and np.array_equal(m32["faces"], m64["faces"])
    line = "%-10s %-9s V %d F %d:" % (kind, "%dx%dx%d" % dims, V, F)
    for k in ("vertices", "normals", "colors"):
        got = out[k][0].cpu().numpy()
        r = _ratio(k, got, m64[k], m32[k])
        line += " %s ratio %.3f" % (k, r)
        assert np.isfinite(got).all() and r <= 1.0, line
    print(line)
    mesh = surface.extract(volume, mw)                                                     # the public call: exact allocation
    assert tuple(mesh.vertices.shape) == (V, 3) and tuple(mesh.faces.shape) == (F, 3)
    for k in ("vertices", "normals", "colors", "faces"):
        assert torch.equal(getattr(mesh, k), out[k][0]), k
    if kind == "sphere" and dims == (17, 9, 33):
        r = so.mesh_report(mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy(), sc.sphere_centre(vol))
        assert r["edge_uses"] == {2} and r["euler"] == 2 and r["min_outward"] > 0 and r["used"], r
    if min(dims) < 2 or dims == (2, 2, 2):
        assert F == 0


@pytest.mark.parametrize("kind", ["sphere", "random"])
def test_capacities_below_the_counts(kind, gpu_device):
    """The full counts are still reported, the rows below the capacities are those of the full mesh, nothing is written beyond."""
    vol, mw = sc.extract_case(kind, (17, 9, 33))
    m64, _ = sc.extract_refs(kind, (17, 9, 33))
    V, F = len(m64["vertices"]), len(m64["faces"])
    volume, _ = _gpu_volume(vol, gpu_device)
    _, full = _extract_guarded(volume, mw, V, F, gpu_device)
    for vcap, fcap in ((V // 2, F // 3), (0, 5), (3, 0), (V, F - 1)):
        (nv, nf), out = _extract_guarded(volume, mw, vcap, fcap, gpu_device)
        assert (nv, nf) == (V, F)
        assert all(_guards_intact(w) for _, w in out.values()), (vcap, fcap)
        for k, cap in (("vertices", vcap), ("normals", vcap), ("colors", vcap), ("faces", fcap)):
            assert torch.equal(out[k][0], full[k][0][:cap]), (k, vcap, fcap)


def test_volumes_without_a_cell_give_an_empty_mesh(gpu_device):
    from fdgs import surface
    for dims in ((1, 5, 3), (4, 4, 1), (0, 3, 3)):
        volume = surface.TSDFVolume((0, 0, 0), 0.1, dims, device=gpu_device)
        volume.weight.fill_(1.0)
        mesh = surface.extract(volume)
        assert mesh.vertices.shape == (0, 3) and mesh.faces.shape == (0, 3)


# ---- 3. end to end -------------------------------------------------------------------------------------------------------------
def _example():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "extract_surface.py")
    spec = importlib.util.spec_from_file_location("extract_surface", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plane_mesh_on_the_gpu_meets_the_voxel_diagonal_bound(gpu_device):
    from fdgs import surface
    vol, views = sc.plane_case()
    volume, _ = _gpu_volume(vol, gpu_device)
    surface.integrate(volume, _gpu_views(views, gpu_device))
    mesh = surface.extract(volume)
    v = mesh.vertices.cpu().numpy()
    assert len(v) >= 50 and mesh.faces.shape[0] >= 50
    assert np.abs(v[:, 2] - sc.PLANE_Z).max() <= math.sqrt(3.0) * vol["s"]
    assert float((mesh.normals[:, 2] + 1.0).abs().max()) <= 1e-4


def test_fuse_and_extract_a_moving_scene_and_the_example_writes_plys(gpu_device, tmp_path):
    """examples/extract_surface.py at tiny size, in this process: two timestamps of a fdgs.synth scene."""
    from fdgs import surface, synth, train_host
    mod = _example()
    kw = dict(W=64, H=48, P=400, s0=0.2, dims=24, extent=1.4, seed=9)
    meshes = mod.run(gpu_device, frames=2, out=str(tmp_path / "surf"), log=print, **kw)
    assert len(meshes) == 2
    for k, (t, mesh) in enumerate(meshes):
        V, F = mesh.vertices.shape[0], mesh.faces.shape[0]
        assert F > 0 and V > 0
        assert int(mesh.faces.min()) >= 0 and int(mesh.faces.max()) < V
        assert float(mesh.vertices.min()) >= -1.4 and float(mesh.vertices.max()) <= 1.4
        assert torch.isfinite(mesh.vertices).all() and torch.isfinite(mesh.normals).all() and torch.isfinite(mesh.colors).all()
        back = surface.load_mesh_ply(str(tmp_path / ("surf_%04d.ply" % k)), gpu_device)
        assert torch.equal(back.vertices, mesh.vertices) and torch.equal(back.faces, mesh.faces)
    (t0, m0), (t1, m1) = meshes
    assert m0.vertices.shape != m1.vertices.shape or not torch.equal(m0.vertices, m1.vertices)
    # fuse_sequence (inside the example) against fuse + extract on a volume of one's own, bit for bit
    scene = synth.make_scene(synth.SceneConfig("surface", kw["P"], kw["W"], kw["H"], 1, 0, kw["s0"], 1.0, True, 4, True), seed=kw["seed"])
    model, pipe, bg = train_host.GaussianParams(scene, gpu_device), train_host.PipelineFlags(), scene["bg"].to(gpu_device)
    from fdgs.playback import with_timestamp
    volume = surface.TSDFVolume((-1.4, -1.4, -1.4), 2.8 / 24, (24, 24, 24), device=gpu_device)
    for t, seq in meshes:
        volume.reset()
        surface.fuse(model, [with_timestamp(c, t) for c in mod.cameras_for(scene, gpu_device)], pipe, bg, volume)
        mine = surface.extract(volume)
        for k in ("vertices", "normals", "colors", "faces"):
            assert torch.equal(getattr(mine, k), getattr(seq, k)), (t, k)


def test_default_device_volume_and_prepared_views(gpu_device):
    """A volume built with the default device ("cuda", no index) takes views that live on cuda:0; views prepared once give the bits of
    unprepared ones, also when integrated twice."""
    from fdgs import surface
    vol, views = sc.integrate_case("full")
    r64, _ = sc.integrate_refs("full")
    gviews = _gpu_views(views, gpu_device)
    with torch.cuda.device(gpu_device):
        default = surface.TSDFVolume(vol["origin"], vol["s"], vol["dims"], trunc=vol["trunc"])
    assert default.device == gpu_device and default.tsdf.device == gpu_device
    surface.integrate(default, gviews[:1])
    surface.integrate(default, gviews[1:])
    explicit = surface.TSDFVolume(vol["origin"], vol["s"], vol["dims"], trunc=vol["trunc"], device=gpu_device)
    prepared = surface.prepare_views([dict(v, intrinsics=views[n]["intr"]) for n, v in enumerate(gviews)], gpu_device)
    assert len(prepared) == len(views)
    surface.integrate(explicit, prepared)
    torch.cuda.synchronize()
    ok = ~r64["flag"]
    assert np.array_equal(default.weight.cpu().numpy()[ok], r64["weight"][ok].astype(np.float32))
    for k in ("tsdf", "weight", "color", "cweight"):
        assert torch.equal(getattr(default, k), getattr(explicit, k)), k
    surface.integrate(explicit, prepared)
    assert torch.equal(explicit.weight, 2 * default.weight)
    empty = surface.TSDFVolume((0, 0, 0), 0.1, (0, 4, 4), device=gpu_device)
    surface.integrate(empty, gviews)                       # nothing to do, nothing is called
    assert surface.extract(empty).faces.shape == (0, 3)


@pytest.mark.parametrize("extra", [[], ["--workload", "C1"]], ids=["default", "workload"])
def test_example_main_writes_a_ply(extra, gpu_device, tmp_path, capsys):
    """examples/extract_surface.py through its command line: one timestamp, a 16^3 volume."""
    from fdgs import surface
    out = str(tmp_path / "m")
    _example().main(["--frames", "1", "--dims", "16", "--out", out] + extra)
    mesh = surface.load_mesh_ply(out + "_0000.ply", gpu_device)
    assert mesh.faces.shape[0] > 0 and int(mesh.faces.max()) < mesh.vertices.shape[0]
    assert "%d vertices, %d faces" % (mesh.vertices.shape[0], mesh.faces.shape[0]) in capsys.readouterr().out
