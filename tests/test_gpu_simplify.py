"""GPU: fdgs.surface.simplify and fdgs_mesh_simplify (csrc/mesh_simplify.hip) against the numpy statement tests/simplify_oracle.py on
the shared inputs of tests/simplify_cases.py.

``vertex_map``, both counts and the faces are compared by array equality.  Positions, colours and normals are held to the bar of
tests/test_gpu_mesh.py: per element 4 x the float32 statement's own distance from the float64 truth, floored at 2e-6
(tests/loss_cases.py: MARGIN, VALUE_FLOOR); only clusters whose normal the truth flags as a near-cancelling sum (at most 2 % of a case,
checked on the host) are left out of the normals' comparison, nothing is left out of the others.  A bar never looks at the kernel's
output; every test prints its worst error / bar.  Every output array of the low-level call sits between guard bands."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import simplify_cases as sc
import simplify_oracle as so
from loss_cases import MARGIN, VALUE_FLOOR
from test_gpu_mesh import _gpu_mesh, _guarded, _guards_intact, _np, _ratio

pytestmark = pytest.mark.gpu


def _simplify_guarded(mesh, origin, h, dims, placement, stabilise, vcap, fcap, dev, with_arrays=True, with_map=True):
    """fdgs_mesh_simplify with every output between guard bands: ([n_vertices, n_faces], {name: tensor})."""
    from fdgs import surface
    struct, _, _held = surface._mesh_struct(mesh)
    counts = _guarded((2,), dev, torch.int32)
    out = {}
    if with_arrays:
        for k in ("vertices", "normals", "colors"):
            out[k] = _guarded((vcap, 3), dev, torch.float32)
        out["faces"] = _guarded((fcap, 3), dev, torch.int32)
    vmap = _guarded((struct.V,), dev, torch.int32) if with_map else None
    surface._simplify_call(struct, dev, origin, h, dims, placement, stabilise, counts[0], None, vcap, fcap,
                           vertex_map=None if vmap is None else vmap[0], **{k: v[0] for k, v in out.items()})
    torch.cuda.synchronize()
    assert all(_guards_intact(w) for _, w in list(out.values()) + [counts] + ([vmap] if with_map else [])), "fdgs_mesh_simplify wrote outside an output array"
    res = {k: v[0] for k, v in out.items()}
    if with_map:
        res["vertex_map"] = vmap[0]
    return [int(c) for c in counts[0].cpu()], res


@pytest.mark.parametrize("name,placement,stabilise", sc.RUNS + sc.CHUNK_RUNS, ids=sc.RUN_IDS + sc.CHUNK_RUN_IDS)
def test_simplify_against_the_statement(name, placement, stabilise, gpu_device):
    from fdgs import surface
    m, origin, h, dims = sc.case(name)
    r64, r32 = sc.refs(name, placement, stabilise)
    nv, nf = len(r32["vertices"]), len(r32["faces"])
    mesh = _gpu_mesh(m, gpu_device)
    before = _np(mesh)
    runs = []
    for _ in range(2):                                                       # the second run: bit-identical
        counts, out = _simplify_guarded(mesh, origin, h, dims, placement, stabilise, nv, nf, gpu_device)
        assert counts == [nv, nf]
        runs.append({k: v.cpu().numpy() for k, v in out.items()})
    for k in runs[0]:
        assert np.array_equal(runs[0][k].view(np.uint8), runs[1][k].view(np.uint8)), "the second run differs in %s" % k
    got = runs[0]
    assert np.array_equal(got["vertex_map"], r32["vertex_map"]), "vertex_map differs"
    assert np.array_equal(got["faces"], r32["faces"]), "faces differ"
    assert r64["flag"].mean() <= 0.02 if nv else True
    ratios = {k: _ratio(got[k], r64[k], r32[k], ~r64["flag"] if k == "normals" else None) for k in ("vertices", "colors", "normals")}
    line = "%-16s %s s %g: %d / %d -> %d / %d, worst error / bar: vertices %.3f, colours %.3f, normals %.3f" % (
        name, "quadric" if placement else "mean", stabilise, len(m["vertices"]), len(m["faces"]), nv, nf, ratios["vertices"], ratios["colors"], ratios["normals"])
    print(line)
    assert all(np.isfinite(got[k]).all() for k in ratios) and max(ratios.values()) <= 1.0, line
    assert all(np.array_equal(before[k], v, equal_nan=k == "vertices") for k, v in _np(mesh).items()), "the input mesh was modified"
    # the public call, where the grid it chooses is the case's: the same bits, in a mesh of exactly the counted size
    own = None if name in AUTO else origin
    if surface._grid_for(surface._bounds(mesh.vertices), h, own)[1] == tuple(dims):
        pub, vmap = surface.simplify(mesh, h, origin=own, placement="quadric" if placement else "mean", stabilise=stabilise, return_map=True)
        for k in ("vertices", "normals", "colors", "faces"):
            assert getattr(pub, k).shape == got[k].shape and np.array_equal(getattr(pub, k).cpu().numpy().view(np.uint8), got[k].view(np.uint8)), k
        assert np.array_equal(vmap.cpu().numpy(), got["vertex_map"])
    else:
        assert name not in AUTO


# the cases whose grid is the one simplify() chooses by itself
AUTO = ("no_faces", "strip257", "strip1025", "sphere_fine", "sphere_coarse", "two_sheets", "duplicates", "unusable", "fan", "zero_area",
        "grid_chunk")


@pytest.mark.parametrize("name,placement", [("sphere_fine", so.QUADRIC), ("strip_permuted", so.MEAN), ("unusable", so.QUADRIC)])
def test_capacities_below_the_counts_and_count_only_calls(name, placement, gpu_device):
    """The full counts are still reported, the rows below the capacities are those of the full result, nothing is written beyond."""
    m, origin, h, dims = sc.case(name)
    r32 = sc.refs(name, placement, sc.STABILISE)[1]
    V, F = len(r32["vertices"]), len(r32["faces"])
    assert V > 8 and F > 8
    mesh = _gpu_mesh(m, gpu_device)
    args = (mesh, origin, h, dims, placement, sc.STABILISE)
    for with_map in (False, True):
        counts, out = _simplify_guarded(*args, 0, 0, gpu_device, with_arrays=False, with_map=with_map)      # count only
        assert counts == [V, F]
        if with_map:
            assert np.array_equal(out["vertex_map"].cpu().numpy(), r32["vertex_map"])
    _, full = _simplify_guarded(*args, V, F, gpu_device)
    for vcap, fcap in ((V // 2, F // 3), (0, 5), (3, 0), (V, F - 1), (V + 7, F + 7)):
        counts, out = _simplify_guarded(*args, vcap, fcap, gpu_device)
        assert counts == [V, F]
        for k, cap, n in (("vertices", vcap, V), ("normals", vcap, V), ("colors", vcap, V), ("faces", fcap, F)):
            assert torch.equal(out[k][:min(cap, n)], full[k][:min(cap, n)]), (k, vcap, fcap)
            sentinel = 12345
            assert bool((out[k][n:] == sentinel).all()), "rows beyond the count were written: %s" % k


def test_cell_for_target_stays_below_the_target_and_is_reproducible(gpu_device):
    from fdgs import surface
    mesh = _gpu_mesh(sc.case("sphere_fine")[0], gpu_device)
    F = mesh.faces.shape[0]
    for target in (F, 400, 100, 3, 0):
        cell = surface.cell_for_target(mesh, target)
        assert cell == surface.cell_for_target(mesh, target) and cell > 0
        n = surface.simplify(mesh, cell).faces.shape[0]
        print("target %4d faces: cell %.5f gives %d" % (target, cell, n))
        assert n <= target
    assert surface.simplify(mesh, surface.cell_for_target(mesh, 400)).faces.shape[0] > 100      # the best probe, not just any
    empty = _gpu_mesh(sc.case("empty")[0], gpu_device)
    assert surface.cell_for_target(empty, 10) == 1.0 and surface.simplify(empty, 1.0).vertices.shape == (0, 3)


def test_fuse_extract_clean_smooth_simplify_save_load(gpu_device, tmp_path):
    """The small volume of tests/test_gpu_mesh.py through the whole chain, and through a PLY."""
    from fdgs import surface
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "extract_surface.py")
    spec = importlib.util.spec_from_file_location("extract_surface", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    (_t, raw), = mod.run(gpu_device, frames=1, out=None, log=None, W=64, H=48, P=400, s0=0.2, dims=24, extent=1.4, seed=9)
    smoothed = surface.smooth(surface.clean(raw, keep_largest=1))
    voxel = 2.0 * 1.4 / 24
    mesh, vmap = surface.simplify(smoothed, 2 * voxel, return_map=True)
    V, F = mesh.vertices.shape[0], mesh.faces.shape[0]
    print("smoothed %d vertices / %d faces -> %d / %d at a cell of 2 voxels" % (smoothed.vertices.shape[0], smoothed.faces.shape[0], V, F))
    assert 0 < V < smoothed.vertices.shape[0] // 2 and 0 < F < smoothed.faces.shape[0] // 2
    assert int(mesh.faces.min()) >= 0 and int(mesh.faces.max()) < V and int(vmap.min()) >= 0 and int(vmap.max()) == V - 1
    for k in ("vertices", "normals", "colors"):
        assert torch.isfinite(getattr(mesh, k)).all(), k
    lengths = mesh.normals.norm(dim=1)
    assert bool(((lengths - 1).abs() < 1e-5).logical_or(lengths == 0).all())
    moved = (mesh.vertices[vmap.long()] - smoothed.vertices).norm(dim=1)
    assert float(moved.max()) <= np.sqrt(3) * 2 * voxel * (1 + 1e-5)         # a vertex stays inside its members' cell
    target = surface.simplify(smoothed, surface.cell_for_target(smoothed, F // 2))
    assert 0 < target.faces.shape[0] <= F // 2
    ply = str(tmp_path / "simplified.ply")
    surface.save_mesh_ply(ply, mesh)
    back = surface.load_mesh_ply(ply, gpu_device)
    assert torch.equal(back.vertices, mesh.vertices) and torch.equal(back.normals, mesh.normals) and torch.equal(back.faces, mesh.faces)
    assert float((back.colors - mesh.colors.clamp(0, 1)).abs().max()) <= 0.5 / 255 + 1e-6
