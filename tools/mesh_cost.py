"""Times the three mesh calls of fdgs.surface (csrc/mesh.hip) on the mesh the 256^3 extraction of DESIGN 4.17 yields (16 synthetic
views of 1352 x 1014 fused into a 256^3 volume: examples/extract_surface.py's bench inputs): fdgs_mesh_components, fdgs_mesh_compact
(keeping the largest component) and fdgs_mesh_smooth with 10 iterations, each as the C call alone on preallocated outputs, HIP events
around one call, the median and range of --reps calls after a warm-up call; next to them the public functions (allocation, the host
reads) and the extraction they follow.  fdgs_mesh_components synchronises once per hook pass, so its figure is a stream time that
includes those round trips; the others are stream times of back-to-back launches.  Prints one JSON line (times in ms).

    python tools/mesh_cost.py [--reps 20] [--dims 256]
    rocprofv3 --kernel-trace --stats -- python tools/mesh_cost.py --reps 5      kernel times, in a run of their own
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


def _timed(fn, reps, dev):
    fn()
    torch.cuda.synchronize(dev)
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize(dev)
        ts.append(a.elapsed_time(b))
    ts.sort()
    return {"median": round(ts[len(ts) // 2], 4), "range": [round(ts[0], 4), round(ts[-1], 4)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--dims", type=int, default=256)
    args = ap.parse_args()
    from fdgs import surface
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
    out = {"voxels": args.dims ** 3, "vertices": V, "faces": F, "reps": args.reps}
    out["extract_ms"] = _timed(lambda: surface.extract(volume), args.reps, dev)

    comp = surface.components(mesh)
    out["components"], out["component_rounds"] = comp.n, comp.rounds
    out["largest_component_faces"] = int(comp.face_counts.max()) if comp.n else 0
    struct, _, _held = surface._mesh_struct(mesh)
    vc, counter = torch.empty(V, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    vcount, fcount = torch.empty(comp.n, dtype=torch.int32, device=dev), torch.empty(comp.n, dtype=torch.int32, device=dev)
    out["components_call_ms"] = _timed(lambda: surface._components_call(struct, dev, comp.n, vc, counter, vcount, fcount), args.reps, dev)
    out["components_counts_only_call_ms"] = _timed(lambda: surface._components_call(struct, dev, comp.n, vc, counter, vcount, fcount, labelled=True),
                                                   args.reps, dev)
    assert torch.equal(vc, comp.vertex_component) and torch.equal(fcount, comp.face_counts)

    keep = torch.zeros(comp.n, dtype=torch.uint8, device=dev)
    keep[int(comp.face_counts.argmax())] = 1
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    surface._compact_call(struct, dev, vc, keep, counts)
    Vk, Fk = (int(v) for v in counts.cpu())
    kept = surface.Mesh(*[torch.empty((Vk, 3), dtype=torch.float32, device=dev) for _ in range(3)], torch.empty((Fk, 3), dtype=torch.int32, device=dev))
    out["kept_vertices"], out["kept_faces"] = Vk, Fk
    out["compact_count_call_ms"] = _timed(lambda: surface._compact_call(struct, dev, vc, keep, counts), args.reps, dev)
    out["compact_emit_call_ms"] = _timed(lambda: surface._compact_call(struct, dev, vc, keep, counts, Vk, Fk, kept.vertices, kept.normals, kept.colors,
                                                                        kept.faces), args.reps, dev)

    pos, nrm = torch.empty_like(mesh.vertices), torch.empty_like(mesh.vertices)
    for its in (0, 1, 10):
        out["smooth_%d_iterations_call_ms" % its] = _timed(lambda: surface._smooth_call(struct, dev, its, 0.5, -0.53, True, pos, nrm), args.reps, dev)
    a, b = out["smooth_1_iterations_call_ms"]["median"], out["smooth_10_iterations_call_ms"]["median"]
    out["smooth_per_iteration_ms"] = round((b - a) / 9.0, 4)
    # what one pass moves at the least: 12 B of position in and out per vertex, 8 B of other-corner indices per incidence, 4 B of row start
    out["smooth_pass_min_bytes"] = 24 * V + 8 * 3 * F + 4 * V

    out["components_public_ms"] = _timed(lambda: surface.components(mesh), args.reps, dev)
    out["clean_public_ms"] = _timed(lambda: surface.clean(mesh, keep_largest=1), args.reps, dev)
    out["smooth_public_ms"] = _timed(lambda: surface.smooth(mesh), args.reps, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
