"""Times fdgs.surface.simplify (csrc/mesh_simplify.hip) on the mesh the 256^3 extraction of DESIGN 4.17 yields (16 synthetic views of
1352 x 1014 fused into a 256^3 volume: examples/extract_surface.py's bench inputs) at cell sizes of 2 and 4 voxels: the count-only
call and the emitting call of fdgs_mesh_simplify as C calls alone on preallocated outputs (HIP events around one call, the median and
range of --reps calls after a warm-up call), the public simplify() as a whole (allocation, the bounds reduction, two host reads), and a
PyTorch formulation of the same result on the same GPU -- torch.unique for the clusters, index_add_ for the sums and the quadrics, a
batched float64 solve, a host-free duplicate removal by sorting packed triples -- which is what the call replaces.  Prints one JSON
line (times in ms).

    python tools/simplify_cost.py [--reps 20] [--dims 256]
    rocprofv3 --kernel-trace --stats -- python tools/simplify_cost.py --reps 5 --no-torch      kernel times, in a run of their own
"""
import argparse
import importlib.util
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools.mesh_cost import _timed  # noqa: E402


def torch_simplify(mesh, origin, h, dims, stabilise=1e-3):
    """The same result up to summation order, in PyTorch on the GPU: (vertices, normals, colors, faces)."""
    v, f = mesh.vertices, mesh.faces.long()
    dev = v.device
    o = torch.tensor(origin, dtype=torch.float32, device=dev)
    n = torch.tensor(dims, device=dev)
    h = torch.tensor(h, dtype=torch.float32, device=dev)      # a tensor: dividing by a Python number multiplies by its reciprocal
    ijk = torch.minimum(torch.clamp(torch.floor((v - o) / h), min=0).long(), n - 1)
    cell = (ijk[:, 2] * dims[1] + ijk[:, 1]) * dims[0] + ijk[:, 0]
    cells, vmap, count = torch.unique(cell, return_inverse=True, return_counts=True)
    C = cells.shape[0]
    cijk = torch.stack([cells % dims[0], (cells // dims[0]) % dims[1], cells // (dims[0] * dims[1])], 1)
    centre = o + (cijk.float() + 0.5) * h
    mean = torch.zeros((C, 3), dtype=torch.float32, device=dev).index_add_(0, vmap, (v - centre[vmap]) / h) / count[:, None]
    colors = torch.zeros((C, 3), dtype=torch.float32, device=dev).index_add_(0, vmap, mesh.colors) / count[:, None]
    normals = torch.nn.functional.normalize(torch.zeros((C, 3), dtype=torch.float32, device=dev).index_add_(0, vmap, mesh.normals), dim=1)
    # quadrics: every face once per corner, in the receiving cell's units
    key = vmap[f].reshape(-1)
    p = (v[f].repeat_interleave(3, 0) - centre[key][:, None, :]) / h                  # [3 F, 3 corners, 3]
    nr = torch.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], dim=1)
    ln = nr.norm(dim=1)
    d = -(nr * p[:, 0]).sum(1)
    w = torch.where(ln > 0, 1.0 / ln, torch.zeros_like(ln)).double()
    nd = nr.double()
    A = torch.zeros((C, 3, 3), dtype=torch.float64, device=dev).index_add_(0, key, nd[:, :, None] * nd[:, None, :] * w[:, None, None])
    b = torch.zeros((C, 3), dtype=torch.float64, device=dev).index_add_(0, key, nd * (d.double() * w)[:, None])
    lam = stabilise * A.diagonal(dim1=1, dim2=2).sum(1) / 3.0
    eye = torch.eye(3, dtype=torch.float64, device=dev)
    safe = lam > 0
    M = A + torch.where(safe, lam, torch.ones_like(lam))[:, None, None] * eye
    x = torch.linalg.solve(M, lam[:, None] * mean.double() - b)
    x = torch.where(safe[:, None], x, mean.double()).clamp(-0.5, 0.5).float()
    vertices = centre + h * x
    # faces: drop the collapsed ones, keep the first of every canonical triple, in input order -- no host read until the final mask
    t = vmap[f]
    ok = (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])
    shift = t.argmin(1)
    rows = torch.arange(t.shape[0], device=dev)
    canon = torch.stack([t[rows, (shift + k) % 3] for k in range(3)], 1)
    packed = (canon[:, 0] * C + canon[:, 1]) * C + canon[:, 2]                         # C < 2^21 here: fits int64
    packed = torch.where(ok, packed, torch.full_like(packed, -1))
    order = torch.sort(packed, stable=True).indices
    sp = packed[order]
    first = torch.ones_like(sp, dtype=torch.bool)
    first[1:] = sp[1:] != sp[:-1]
    keep = torch.zeros_like(ok)
    keep[order] = first & (sp >= 0)
    return vertices, normals, colors, t[keep].int()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--dims", type=int, default=256)
    ap.add_argument("--no-torch", action="store_true", help="leave the PyTorch formulation out (for a kernel trace of the library's kernels alone)")
    args = ap.parse_args()
    from fdgs import _capi, surface
    spec = importlib.util.spec_from_file_location("extract_surface", os.path.join(ROOT, "examples", "extract_surface.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    volume, views, _ = ex.bench_inputs(dev, args.dims)
    surface.integrate(volume, views)
    mesh = surface.extract(volume)
    del views
    V, F = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    out = {"voxels": args.dims ** 3, "vertices": V, "faces": F, "reps": args.reps,
           "scratch_MB": round(_capi.lib.fdgs_mesh_simplify_scratch_bytes(V, F) / 2 ** 20, 1)}
    struct, _, _held = surface._mesh_struct(mesh)
    scratch = _capi.scratch(_capi.lib.fdgs_mesh_simplify_scratch_bytes(V, F), dev, floor=256)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    for voxels in (2, 4):
        h = voxels * volume.voxel_size
        origin, dims = surface._grid_for(surface._bounds(mesh.vertices), h)
        r = {"cell": h, "grid": list(dims)}
        for name, placement in (("quadric", _capi.FDGS_SIMPLIFY_QUADRIC), ("mean", _capi.FDGS_SIMPLIFY_MEAN)):
            args_ = (struct, dev, origin, h, dims, placement, 1e-3, counts, scratch)
            surface._simplify_call(*args_)
            nv, nf = (int(c) for c in counts.cpu())
            r["vertices"], r["faces"] = nv, nf
            o = surface.Mesh(*[torch.empty((nv, 3), dtype=torch.float32, device=dev) for _ in range(3)], torch.empty((nf, 3), dtype=torch.int32, device=dev))
            if name == "quadric":
                r["count_call_ms"] = _timed(lambda: surface._simplify_call(*args_), args.reps, dev)
            r["emit_call_%s_ms" % name] = _timed(lambda: surface._simplify_call(*args_, nv, nf, o.vertices, o.normals, o.colors, o.faces), args.reps, dev)
        r["simplify_public_ms"] = _timed(lambda: surface.simplify(mesh, h), args.reps, dev)
        if not args.no_torch:
            mine = surface.simplify(mesh, h)
            tv, tn, tc, tf = torch_simplify(mesh, [float(x) for x in origin], h, dims)
            r["torch_same_faces"] = bool(tf.shape == mine.faces.shape and torch.equal(tf, mine.faces))
            r["torch_max_vertex_gap"] = float((tv - mine.vertices).abs().max()) if tv.shape == mine.vertices.shape else None
            r["torch_formulation_ms"] = _timed(lambda: torch_simplify(mesh, [float(x) for x in origin], h, dims), max(3, args.reps // 4), dev)
        out["cell_%d_voxels" % voxels] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
