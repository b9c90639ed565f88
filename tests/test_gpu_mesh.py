"""GPU: the mesh calls of fdgs.surface (csrc/mesh.hip) -- connected components, component filtering with compaction, Taubin smoothing
-- against the numpy statement tests/mesh_oracle.py on the shared inputs of tests/mesh_cases.py.

Integer outputs (component ids, counts, faces, boundary flags) are compared by array equality, vertex rows after ``clean`` by array
equality against a gather of the input.  Smoothed positions and normals are held to the bar of tests/test_gpu_surface.py: per element
4 x the float32 statement's own distance from the float64 truth, floored at 2e-6 (tests/loss_cases.py: MARGIN, VALUE_FLOOR); only
vertices whose normal the truth flags as a near-cancelling sum (at most 2 % of a case, checked on the host) are left out of the normals'
comparison.  A bar never looks at a kernel's output; every smoothing test prints its worst error / bar.  Every output array of the
low-level calls sits between guard bands."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import mesh_cases as mc
import mesh_oracle as mo
from loss_cases import MARGIN, VALUE_FLOOR

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 64, 12345


def _guarded(shape, dev, dtype):
    """(the tensor, the buffer it sits in with GUARD sentinels before and after it)."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), SENTINEL % 251 if dtype == torch.uint8 else SENTINEL, dtype=dtype, device=dev)
    return whole[GUARD:GUARD + n].view(shape), whole


def _guards_intact(whole):
    want = SENTINEL % 251 if whole.dtype == torch.uint8 else SENTINEL
    return bool((whole[:GUARD] == want).all()) and bool((whole[-GUARD:] == want).all())


def _gpu_mesh(m, dev):
    from fdgs import surface
    return surface.Mesh(*[torch.from_numpy(np.ascontiguousarray(m[k])).to(dev) for k in ("vertices", "normals", "colors", "faces")])


def _np(mesh):
    return {k: getattr(mesh, k).cpu().numpy() for k in ("vertices", "normals", "colors", "faces")}


def _components_guarded(mesh, cap, dev):
    """fdgs_mesh_components with every output between guard bands: ({name: array}, n, rounds)."""
    from fdgs import surface
    struct, _, _held = surface._mesh_struct(mesh)
    out = {"vertex_component": _guarded((struct.V,), dev, torch.int32), "counter": _guarded((1,), dev, torch.int32),
           "vertex_counts": _guarded((cap,), dev, torch.int32), "face_counts": _guarded((cap,), dev, torch.int32)}
    rounds = surface._components_call(struct, dev, cap, out["vertex_component"][0], out["counter"][0], out["vertex_counts"][0], out["face_counts"][0])
    torch.cuda.synchronize()
    assert all(_guards_intact(w) for _, w in out.values()), "fdgs_mesh_components wrote outside an output array"
    return {k: v[0].cpu().numpy() for k, v in out.items()}, int(out["counter"][0].item()), rounds


def _compact_guarded(mesh, vc, keep, vcap, fcap, dev, with_arrays=True):
    from fdgs import surface
    struct, _, _held = surface._mesh_struct(mesh)
    counts = torch.full((2,), -7, dtype=torch.int32, device=dev)
    out = {}
    if with_arrays:
        for k in ("vertices", "normals", "colors"):
            out[k] = _guarded((vcap, 3), dev, torch.float32)
        out["faces"] = _guarded((fcap, 3), dev, torch.int32)
    surface._compact_call(struct, dev, vc, keep, counts, vcap, fcap, **{k: v[0] for k, v in out.items()})
    torch.cuda.synchronize()
    assert all(_guards_intact(w) for _, w in out.values()), "fdgs_mesh_compact wrote outside an output array"
    return [int(c) for c in counts.cpu()], {k: v[0] for k, v in out.items()}


# ---- 1. components and clean ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.TOPOLOGY_CASES + mc.CHUNK_CASES)
def test_components_and_clean_against_the_statement(name, gpu_device):
    from fdgs import surface
    m, ref = mc.topology_case(name), mc.topology_refs(name)
    mesh = _gpu_mesh(m, gpu_device)
    before = _np(mesh)
    runs = []
    for _ in range(2):                                                       # the second run: bit-identical
        got, n, rounds = _components_guarded(mesh, ref["n"], gpu_device)
        assert n == ref["n"] and 0 <= rounds <= 32
        for k in ("vertex_component", "vertex_counts", "face_counts"):
            assert np.array_equal(got[k], ref[k]), k
        runs.append(rounds)
    print("%-15s V %d F %d: %d components, %s hook passes" % (name, len(m["vertices"]), len(m["faces"]), ref["n"], runs))
    comp = surface.components(mesh)                                          # the public call: exact allocation
    assert comp.n == ref["n"] and tuple(comp.vertex_counts.shape) == (ref["n"],) and tuple(comp.face_counts.shape) == (ref["n"],)
    for k in ("vertex_component", "vertex_counts", "face_counts"):
        assert np.array_equal(getattr(comp, k).cpu().numpy(), ref[k]), k
    for choice in mc.CLEAN_CHOICES:
        want, vmap = mo.compact(m, ref["vertex_component"], mo.keep_mask(ref["face_counts"], **choice))
        outs = [_np(surface.clean(mesh, **choice)) for _ in range(2)]
        for k in ("vertices", "normals", "colors", "faces"):
            assert outs[0][k].shape == want[k].shape and np.array_equal(outs[0][k].view(np.int32), want[k].view(np.int32)), (choice, k)
            assert np.array_equal(outs[0][k].view(np.int32), outs[1][k].view(np.int32)), (choice, k)
        assert np.array_equal(outs[0]["vertices"].view(np.int32), m["vertices"][vmap >= 0].view(np.int32))      # a gather of the input
        if len(want["faces"]):
            assert want["faces"].min() >= 0 and outs[0]["faces"].max() < len(want["vertices"])
    assert all(np.array_equal(before[k], v) for k, v in _np(mesh).items()), "the input mesh was modified"


@pytest.mark.parametrize("name,base", [("absent", None), ("absent_random", "random")])
def test_absent_faces_change_nothing(name, base, gpu_device):
    """Faces with indices -1, V and 2^30 mixed in: every result equals that of the same mesh without them."""
    from fdgs import surface
    dirty = _gpu_mesh(mc.topology_case(name), gpu_device)
    clean = _gpu_mesh(mc.blocks(257, seed=258) if base is None else mc.extracted(base), gpu_device)
    a, b = surface.components(dirty), surface.components(clean)
    assert a.n == b.n
    for k in ("vertex_component", "vertex_counts", "face_counts"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    for choice in mc.CLEAN_CHOICES:
        x, y = surface.clean(dirty, **choice), surface.clean(clean, **choice)
        for k in ("vertices", "normals", "colors", "faces"):
            assert torch.equal(getattr(x, k), getattr(y, k)), (choice, k)
    for pin in (True, False):
        x, y = surface.smooth(dirty, 2, pin_boundary=pin), surface.smooth(clean, 2, pin_boundary=pin)
        assert torch.equal(x.vertices, y.vertices) and torch.equal(x.normals, y.normals)
        assert torch.equal(x.faces, dirty.faces) and torch.equal(x.colors, dirty.colors)


def test_two_components_with_equal_face_counts_under_keep_largest_one(gpu_device):
    from fdgs import surface
    m = mc.topology_case("equal_pair")
    out = surface.clean(_gpu_mesh(m, gpu_device), keep_largest=1)
    assert np.array_equal(out.vertices.cpu().numpy(), m["vertices"][:7]) and np.array_equal(out.faces.cpu().numpy(), m["faces"][:5])


@pytest.mark.parametrize("name", ["random", "v1025"] + list(mc.CHUNK_CASES))
def test_capacities_below_the_counts_and_count_only_calls(name, gpu_device):
    """The full counts are still reported, the rows below the capacities are those of the full result, nothing is written beyond.
    "v262145" is past a scan chunk in its vertices and not in its faces: the two scans of fdgs_mesh_compact's one launch run over
    1025 and 2 workgroup counts, and every other component with a face is kept, so kept vertices lie on both sides of the chunk."""
    m, ref = mc.topology_case(name), mc.topology_refs(name)
    mesh = _gpu_mesh(m, gpu_device)
    for cap in (0, 1, ref["n"] // 2, ref["n"] - 1):
        got, n, _ = _components_guarded(mesh, cap, gpu_device)
        assert n == ref["n"] and np.array_equal(got["vertex_component"], ref["vertex_component"])
        assert np.array_equal(got["vertex_counts"], ref["vertex_counts"][:cap]) and np.array_equal(got["face_counts"], ref["face_counts"][:cap]), cap
    vc = torch.from_numpy(ref["vertex_component"]).to(gpu_device)
    keep_np = (ref["face_counts"] > 0) & (np.arange(ref["n"]) % 2 == 0)             # every other component that has a face
    keep = torch.from_numpy(keep_np.astype(np.uint8)).to(gpu_device)
    want, _ = mo.compact(m, ref["vertex_component"], keep_np)
    V, F = len(want["vertices"]), len(want["faces"])
    assert 0 < V < len(m["vertices"]) and 0 < F < len(m["faces"])
    (nv, nf), _ = _compact_guarded(mesh, vc, keep, 0, 0, gpu_device, with_arrays=False)             # count only
    assert (nv, nf) == (V, F)
    _, full = _compact_guarded(mesh, vc, keep, V, F, gpu_device)
    for k in want:
        assert np.array_equal(full[k].cpu().numpy().view(np.int32), want[k].view(np.int32)), k
    for vcap, fcap in ((V // 2, F // 3), (0, 5), (3, 0), (V, F - 1)):
        (nv, nf), out = _compact_guarded(mesh, vc, keep, vcap, fcap, gpu_device)
        assert (nv, nf) == (V, F)
        for k, cap in (("vertices", vcap), ("normals", vcap), ("colors", vcap), ("faces", fcap)):
            assert torch.equal(out[k], full[k][:cap]), (k, vcap, fcap)
    # ids outside [0, C) are kept nowhere, whatever they are
    bad = vc.clone()
    rows = torch.arange(0, len(bad), 3, device=gpu_device)
    bad[rows] = torch.tensor([-1, ref["n"], 2 ** 30], dtype=torch.int32, device=gpu_device)[torch.arange(len(rows), device=gpu_device) % 3]
    (nv, nf), out = _compact_guarded(mesh, bad, keep, len(m["vertices"]), len(m["faces"]), gpu_device)
    want_bad, _ = mo.compact(m, bad.cpu().numpy(), keep_np)
    assert (nv, nf) == (len(want_bad["vertices"]), len(want_bad["faces"]))
    assert np.array_equal(out["faces"][:nf].cpu().numpy(), want_bad["faces"])


# ---- 2. smoothing --------------------------------------------------------------------------------------------------------------
def _ratio(got, r64, r32, rows=None):
    """The worst |got - truth| / bar over the selected rows, bar = max(VALUE_FLOOR, MARGIN |float32 statement - truth|)."""
    err = np.abs(got.astype(np.float64) - r64)
    ratio = err / np.maximum(VALUE_FLOOR, MARGIN * np.abs(r32.astype(np.float64) - r64))
    if rows is not None:
        ratio = ratio[rows]
    return float(ratio.max()) if ratio.size else 0.0


@pytest.mark.parametrize("iterations,pin", mc.SMOOTH_RUNS, ids=["it%d_pin%d" % (i, p) for i, p in mc.SMOOTH_RUNS])
@pytest.mark.parametrize("name", mc.SMOOTH_CASES)
def test_smooth_against_the_statement(name, iterations, pin, gpu_device):
    from fdgs import surface
    m = mc.smooth_case(name)
    r64, r32 = mc.smooth_refs(name, iterations, pin)
    mesh = _gpu_mesh(m, gpu_device)
    before = _np(mesh)
    struct, _, _held = surface._mesh_struct(mesh)
    V = struct.V
    runs = []
    for _ in range(2):
        pos, normals, flags = _guarded((V, 3), gpu_device, torch.float32), _guarded((V, 3), gpu_device, torch.float32), _guarded((V,), gpu_device, torch.uint8)
        surface._smooth_call(struct, gpu_device, iterations, mc.LAMBDA, mc.MU, pin, pos[0], normals[0], flags[0])
        torch.cuda.synchronize()
        assert _guards_intact(pos[1]) and _guards_intact(normals[1]) and _guards_intact(flags[1]), "fdgs_mesh_smooth wrote outside an output array"
        runs.append((pos[0].cpu().numpy(), normals[0].cpu().numpy(), flags[0].cpu().numpy()))
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "the second run differs"
    got_p, got_n, got_b = runs[0]
    assert np.array_equal(got_b, r64["boundary"]), "boundary flags differ"
    assert r64["flag"].mean() <= 0.02
    rp, rn = _ratio(got_p, r64["vertices"], r32["vertices"]), _ratio(got_n, r64["normals"], r32["normals"], ~r64["flag"])
    line = "%-7s it %2d pin %d V %d: vertices ratio %.3f, normals ratio %.3f" % (name, iterations, pin, V, rp, rn)
    print(line)
    assert np.isfinite(got_p).all() and np.isfinite(got_n).all() and rp <= 1.0 and rn <= 1.0, line
    if iterations == 0:
        assert np.array_equal(got_p.view(np.int32), m["vertices"].view(np.int32))
    if pin:
        fixed = r64["boundary"] > 0
        assert np.array_equal(got_p[fixed].view(np.int32), m["vertices"][fixed].view(np.int32))
    out = surface.smooth(mesh, iterations, pin_boundary=pin)                 # the public call: the same bits, in a new mesh
    assert np.array_equal(out.vertices.cpu().numpy().view(np.int32), got_p.view(np.int32))
    assert np.array_equal(out.normals.cpu().numpy().view(np.int32), got_n.view(np.int32))
    assert torch.equal(out.colors, mesh.colors) and torch.equal(out.faces, mesh.faces)
    kept = surface.smooth(mesh, iterations, pin_boundary=pin, recompute_normals=False)
    assert torch.equal(kept.normals, mesh.normals) and torch.equal(kept.vertices, out.vertices)
    assert all(np.array_equal(before[k], v) for k, v in _np(mesh).items()), "the input mesh was modified"


def test_empty_meshes_smooth_to_themselves(gpu_device):
    from fdgs import surface
    for name in ("empty", "no_faces"):
        mesh = _gpu_mesh(mc.topology_case(name), gpu_device)
        out = surface.smooth(mesh)
        assert torch.equal(out.vertices, mesh.vertices) and out.faces.shape == (0, 3)
        assert not out.normals.any()


# ---- 3. end to end -------------------------------------------------------------------------------------------------------------
def test_fuse_extract_clean_smooth(gpu_device):
    """A small synthetic model, fused and extracted as tests/test_gpu_surface.py does, then cleaned to its largest component and smoothed."""
    from fdgs import surface
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "extract_surface.py")
    spec = importlib.util.spec_from_file_location("extract_surface", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    (_t, raw), = mod.run(gpu_device, frames=1, out=None, log=None, W=64, H=48, P=400, s0=0.2, dims=24, extent=1.4, seed=9)
    parts = surface.components(raw)
    cleaned = surface.clean(raw, keep_largest=1)
    mesh = surface.smooth(cleaned)
    print("raw %d vertices / %d faces in %d components -> %d / %d" % (raw.vertices.shape[0], raw.faces.shape[0], parts.n, mesh.vertices.shape[0],
                                                                    mesh.faces.shape[0]))
    V, F = mesh.vertices.shape[0], mesh.faces.shape[0]
    assert parts.n >= 1 and F == int(parts.face_counts.max()) and 0 < V <= raw.vertices.shape[0]
    assert surface.components(mesh).n == 1
    assert int(mesh.faces.min()) >= 0 and int(mesh.faces.max()) < V
    for k in ("vertices", "normals", "colors"):
        assert torch.isfinite(getattr(mesh, k)).all(), k
    assert torch.equal(mesh.faces, cleaned.faces) and torch.equal(mesh.colors, cleaned.colors)
    lengths = mesh.normals.norm(dim=1)
    assert bool(((lengths - 1).abs() < 1e-5).logical_or(lengths == 0).all())
