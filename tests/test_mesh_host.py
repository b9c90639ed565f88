"""CPU: the numpy statement of the mesh calls (tests/mesh_oracle.py) checked on its own -- a closed sphere through clean, floaters,
a flat grid, a noisy sphere under Taubin and Laplacian smoothing -- the shared inputs' share of near-cancelling normals, and the
host-side argument handling of the new C calls (nothing is launched)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import mesh_cases as mc
import mesh_oracle as mo
import surface_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("fdgs_mesh_components_scratch_bytes", "fdgs_mesh_components", "fdgs_mesh_compact_scratch_bytes", "fdgs_mesh_compact",
           "fdgs_mesh_smooth_scratch_bytes", "fdgs_mesh_smooth")


def test_the_sphere_is_one_component_and_stays_closed_through_clean():
    m = mc.extracted("sphere")
    c = mo.components(len(m["vertices"]), m["faces"])
    assert c["n"] == 1 and c["vertex_counts"].tolist() == [len(m["vertices"])] and c["face_counts"].tolist() == [len(m["faces"])]
    out = mo.clean(m, keep_largest=1)
    assert so.mesh_report(out["vertices"], out["faces"])["euler"] == 2
    assert all(np.array_equal(out[k], m[k]) for k in m)
    # with stray vertices and absent faces around it: the same sphere comes back
    dirty = mc.with_absent(mc.join(mc.make_mesh(np.ones((3, 3)), np.zeros((0, 3))), m))
    out = mo.clean(dirty)
    r = so.mesh_report(out["vertices"], out["faces"])
    assert r["euler"] == 2 and r["edge_uses"] == {2} and r["used"]
    assert np.array_equal(out["vertices"], m["vertices"]) and np.array_equal(out["faces"], m["faces"])


def test_keep_largest_and_min_faces_remove_exactly_the_floater():
    s = mc.extracted("sphere")
    far = dict(s, vertices=s["vertices"] + np.float32(1.0))
    both = mc.join(s, mc.floater(), far)
    c = mo.components(len(both["vertices"]), both["faces"])
    assert c["n"] == 3 and c["face_counts"].tolist() == [len(s["faces"]), 12, len(s["faces"])]
    want = mc.join(s, far)
    for choice in (dict(keep_largest=2), dict(min_faces=13)):
        out = mo.clean(both, **choice)
        assert all(np.array_equal(out[k], want[k]) for k in want), choice
    assert len(mo.clean(both, min_faces=12)["faces"]) == len(both["faces"])
    # ties in face count go to the smaller component id
    assert np.array_equal(mo.clean(both, keep_largest=1)["vertices"], s["vertices"])
    assert mo.keep_mask([4, 9, 9, 0, 9], keep_largest=2).tolist() == [False, True, True, False, False]
    assert mo.keep_mask([4, 9, 9, 0, 9], keep_largest=4, min_faces=5).tolist() == [False, True, True, False, True]
    assert mo.keep_mask([4, 0, 2]).tolist() == [True, False, True]


def test_component_ids_follow_the_smallest_vertex_index():
    faces = [[5, 6, 4], [0, 2, 2], [7, 7, 7], [9, 1, 3], [-1, 0, 5], [0, 10, 5]]       # the last two are absent (V = 10)
    c = mo.components(10, faces)
    assert c["vertex_component"].tolist() == [0, 1, 0, 1, 2, 2, 2, 3, 4, 1]
    assert c["vertex_counts"].tolist() == [2, 3, 3, 1, 1] and c["face_counts"].tolist() == [1, 1, 1, 1, 0]


def test_smoothing_a_flat_grid_with_pinned_boundary_moves_nothing():
    m = mc.smooth_case("grid")
    r = mo.smooth(m["vertices"], m["faces"], 10, mc.LAMBDA, mc.MU, True, np.float32)
    nx, ny = 9, 7
    j, i = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    edge = ((i == 0) | (i == nx - 1) | (j == 0) | (j == ny - 1)).ravel()
    assert np.array_equal(r["boundary"].astype(bool), edge)
    assert np.abs(r["vertices"] - m["vertices"]).max() <= 1e-6
    assert np.array_equal(r["vertices"][edge], m["vertices"][edge])
    assert np.abs(r["normals"] - np.array([0, 0, 1.0])).max() <= 1e-6
    free = mo.smooth(m["vertices"], m["faces"], 10, mc.LAMBDA, mc.MU, False, np.float64)
    assert np.abs(free["vertices"] - m["vertices"]).max() > 1e-3                  # unpinned, the rim does move


def test_taubin_reduces_the_noise_and_keeps_the_volume_better_than_laplacian():
    m, centre = mc.noisy_sphere()
    clean_sphere = mc.extracted("sphere")
    assert np.array_equal(mo.boundary(len(m["vertices"]), m["faces"]), np.zeros(len(m["vertices"]), np.uint8))

    def rms(v):
        r = np.linalg.norm(np.asarray(v, np.float64) - centre, axis=1)
        return float(np.sqrt(((r - r.mean()) ** 2).mean()))
    taubin = mo.smooth(m["vertices"], m["faces"], 10, mc.LAMBDA, mc.MU, True, np.float64)
    laplace = mo.smooth(m["vertices"], m["faces"], 10, mc.LAMBDA, 0.0, True, np.float64)
    print("radial rms: surface nets %.5f, noisy %.5f, taubin %.5f, laplacian %.5f" % (rms(clean_sphere["vertices"]), rms(m["vertices"]),
                                                                                     rms(taubin["vertices"]), rms(laplace["vertices"])))
    assert rms(taubin["vertices"]) < 0.75 * rms(m["vertices"])
    v0 = mo.volume(m["vertices"], m["faces"])
    dt, dl = abs(mo.volume(taubin["vertices"], m["faces"]) - v0), abs(mo.volume(laplace["vertices"], m["faces"]) - v0)
    print("volume %.6f: taubin changes it by %.2f %%, laplacian by %.2f %%" % (v0, 100 * dt / v0, 100 * dl / v0))
    assert v0 > 0 and dt < 0.25 * dl
    outward = (taubin["normals"] * (taubin["vertices"] - centre)).sum(1)
    assert outward.min() > 0


@pytest.mark.parametrize("name", mc.SMOOTH_CASES)
def test_shared_smoothing_inputs_keep_near_cancelling_normals_rare(name):
    """At most 2 % of a case's vertices have a normal whose sum nearly cancels; the cases reach the rows they are there for."""
    m = mc.smooth_case(name)
    V = len(m["vertices"])
    rs = mo.incidences(V, m["faces"])[0]
    deg = np.diff(rs)
    for iterations, pin in mc.SMOOTH_RUNS:
        r64, r32 = mc.smooth_refs(name, iterations, pin)
        share = float(r64["flag"].mean())
        print("%-7s it %2d pin %d: flagged %.2f %%, boundary %d of %d" % (name, iterations, pin, 100 * share, int(r64["boundary"].sum()), V))
        assert share <= 0.02
        assert np.array_equal(r64["boundary"], r32["boundary"]) and np.isfinite(r64["vertices"]).all() and np.isfinite(r32["normals"]).all()
        if iterations == 0:
            assert np.array_equal(r32["vertices"], m["vertices"])
    if name == "mixed":
        assert deg.max() == 80 and (deg == 1).sum() >= 5 and (deg == 0).sum() >= 2
        assert not mo.present(m["faces"], V).all()
        b = mc.smooth_refs(name, 1, True)[0]["boundary"]
        assert b[0] == 0 and b[1:81].all() and b[83] == 1       # the closed fan's centre is interior (its rim is not), the open fan's is not
    if name == "random":
        assert 0 < mc.smooth_refs(name, 1, True)[0]["boundary"].sum() < V


def test_topology_inputs_reach_what_they_are_there_for():
    refs = {n: mc.topology_refs(n) for n in mc.TOPOLOGY_CASES}
    assert refs["sphere"]["n"] == 1 and refs["random"]["n"] >= 10 and refs["empty"]["n"] == 0 and refs["no_faces"]["n"] == 300
    assert refs["triangle"]["n"] == 1 and refs["strip_permuted"]["n"] == 1 and refs["strip_natural"]["n"] == 1
    assert len(mc.topology_case("strip_permuted")["vertices"]) == 10002
    assert refs["v257"]["n"] >= 7 and refs["v1025"]["n"] >= 28 and (refs["v257"]["face_counts"] == 0).any()
    assert refs["equal_pair"]["face_counts"].tolist() == [5, 5]
    r = so.mesh_report(mc.topology_case("random")["vertices"], mc.topology_case("random")["faces"])
    assert max(r["edge_uses"]) >= 3                                       # non-manifold edges
    for name, base in (("absent", mc.blocks(257, seed=258)), ("absent_random", mc.extracted("random"))):
        m = mc.topology_case(name)
        bad = ~mo.present(m["faces"], len(m["vertices"]))
        assert bad.sum() >= 5 and {-1, len(m["vertices"]), 2 ** 30} <= set(m["faces"][bad].ravel().tolist())
        clean = mo.components(len(base["vertices"]), base["faces"])
        assert all(np.array_equal(refs[name][k], clean[k]) for k in ("vertex_component", "vertex_counts", "face_counts"))


def test_header_library_and_binding_list_carry_the_mesh_calls():
    from fdgs import _capi
    with open(os.path.join(ROOT, "include", "fdgs.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(fdgs_[a-z_0-9]+)\s*\(", text))
    for sym in SYMBOLS:
        assert sym in declared, "include/fdgs.h does not declare %s" % sym
        assert sym in _capi.EXPORTED and hasattr(_capi.lib, sym), sym
    for struct in ("fdgs_mesh_in", "fdgs_mesh_components_out", "fdgs_mesh_smooth_out"):
        assert re.search(r"typedef struct %s\s*\{\s*uint32_t struct_size;" % struct, text), struct
    assert _capi.lib.fdgs_version() == _capi.FDGS_VERSION == 502
    with open(os.path.join(ROOT, "4d-gaussian-splatting_amd", "csrc", "build.sh")) as f:
        sh = f.read()
    assert re.search(r"for src in [^;]*\bmesh\b[^;]*; do", sh) and re.search(r'\[mesh\]="[^"]*-ffp-contract=off', sh)
    lib = _capi.lib
    for name in ("components", "compact", "smooth"):
        fn = getattr(lib, "fdgs_mesh_%s_scratch_bytes" % name)
        assert fn(-1, 5) == 0 and fn(5, -1) == 0 and fn(2 ** 28, 5) == 0 and fn(5, 2 ** 28) == 0
        sizes = [fn(0, 0), fn(1, 1), fn(257, 300), fn(285325, 350838), fn(2 ** 28 - 1, 2 ** 28 - 1)]
        assert all(s % 256 == 0 for s in sizes) and sizes == sorted(sizes) and sizes[1] > 0, (name, sizes)
    assert 4 * 285325 <= lib.fdgs_mesh_components_scratch_bytes(285325, 350838) < 4.1 * 285325
    assert lib.fdgs_mesh_smooth_scratch_bytes(285325, 350838) >= (16 + 8) * 3 * 350838 + 12 * 285325


def test_struct_sizes_and_argument_errors_without_touching_the_gpu():
    """Every bad argument is FDGS_ERR_INVALID_ARG before anything is launched (the pointers here are not device memory)."""
    from fdgs import _capi
    lib = _capi.lib
    for cls, size in ((_capi.FdgsMeshIn, 48), (_capi.FdgsMeshComponentsOut, 56), (_capi.FdgsMeshSmoothOut, 48)):
        assert cls().struct_size == C.sizeof(cls) == size and cls._fields_[0][0] == "struct_size"
    nan = float("nan")

    def build(cls, base, kw):
        s = cls(*base)
        for k, x in kw.items():
            setattr(s, k, x)
        return s
    mesh = lambda **kw: build(_capi.FdgsMeshIn, (4, 2, 64, 64, 64, 64), kw)  # noqa: E731
    comp = lambda **kw: build(_capi.FdgsMeshComponentsOut, (2, 0, 64, 64, 64, 64, None), kw)  # noqa: E731
    surf = lambda **kw: build(_capi.FdgsSurfaceOut, (0, 0, None, None, None, None, 64, 64), kw)  # noqa: E731
    smo = lambda **kw: build(_capi.FdgsMeshSmoothOut, (1, 0.5, -0.53, 1, 64, 64, None), kw)  # noqa: E731
    calls = {
        "fdgs_mesh_components": lambda m, o=None, scratch=64: lib.fdgs_mesh_components(C.byref(m), C.byref(o if o is not None else comp()), scratch, None),
        "fdgs_mesh_compact": lambda m, o=None, scratch=64, vc=64, keep=64, n=3: lib.fdgs_mesh_compact(C.byref(m), vc, keep, n, C.byref(o if o is not None else surf()), scratch, None),
        "fdgs_mesh_smooth": lambda m, o=None, scratch=64: lib.fdgs_mesh_smooth(C.byref(m), C.byref(o if o is not None else smo()), scratch, None),
    }
    outs = {"fdgs_mesh_components": (comp, "fdgs_mesh_components_out"), "fdgs_mesh_compact": (surf, "fdgs_surface_out"),
            "fdgs_mesh_smooth": (smo, "fdgs_mesh_smooth_out")}
    for name, call in calls.items():
        for delta in (-4, 8):
            m = mesh()
            m.struct_size += delta
            assert call(m) == 1, name
            assert "struct_size" in _capi.last_error() and "fdgs_mesh_in" in _capi.last_error() and name in _capi.last_error()
            o = outs[name][0]()
            o.struct_size += delta
            assert call(mesh(), o) == 1 and outs[name][1] in _capi.last_error(), name
        for bad in (dict(V=-1), dict(F=-2), dict(V=2 ** 28), dict(F=2 ** 28), dict(faces=None)):
            assert call(mesh(**bad)) == 1, (name, bad)
            assert name in _capi.last_error()
        assert call(mesh(), scratch=None) == 1 and "scratch" in _capi.last_error(), name
    assert lib.fdgs_mesh_components(None, C.byref(comp()), 64, None) == 1 and lib.fdgs_mesh_components(C.byref(mesh()), None, 64, None) == 1
    assert lib.fdgs_mesh_compact(C.byref(mesh()), 64, 64, 3, None, 64, None) == 1 and lib.fdgs_mesh_smooth(C.byref(mesh()), None, 64, None) == 1
    components, compact, smooth = (calls[k] for k in ("fdgs_mesh_components", "fdgs_mesh_compact", "fdgs_mesh_smooth"))
    for bad in (dict(capacity=-1), dict(n_components=None), dict(vertex_component=None)):
        assert components(mesh(), comp(**bad)) == 1, bad
    for bad in (dict(n_vertices=None), dict(n_faces=None), dict(vertex_capacity=-1), dict(face_capacity=-1)):
        assert compact(mesh(), surf(**bad)) == 1, bad
    assert compact(mesh(), vc=None) == 1 and "vertex_component" in _capi.last_error()
    assert compact(mesh(), keep=None) == 1 and "keep" in _capi.last_error()
    assert compact(mesh(), n=-1) == 1 and "n_components" in _capi.last_error()
    assert compact(mesh(normals=None), surf(normals=64)) == 1 and "input array" in _capi.last_error()
    for bad in (dict(iterations=-1), dict(lam=nan), dict(mu=nan), dict(vertices=None)):
        assert smooth(mesh(), smo(**bad)) == 1, bad
    assert smooth(mesh(vertices=None)) == 1 and "vertices" in _capi.last_error()
    # nothing to do: no vertex, nothing is launched by the smoothing (the other two only clear their counters, on the GPU)
    assert smooth(mesh(V=0, F=0, vertices=None, faces=None), scratch=None) == 0


def test_cpu_tensors_are_refused():
    from fdgs import surface
    m = surface.Mesh(torch.zeros(3, 3), torch.zeros(3, 3), torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32))
    for fn in (surface.components, surface.clean, surface.smooth):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(m)
