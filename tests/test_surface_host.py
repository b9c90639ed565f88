"""CPU: the numpy statement of fdgs.surface (tests/surface_oracle.py) checked on its own -- an analytic plane, a closed sphere -- the
shared inputs' cliff share, the mesh PLY round trip and the host-side argument handling of the new C calls (nothing is launched)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import surface_cases as sc
import surface_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("fdgs_tsdf_integrate", "fdgs_surface_extract_scratch_bytes", "fdgs_surface_extract")


def test_plane_vertices_lie_within_a_voxel_diagonal_of_the_plane():
    """Three cameras in front of the plane z = PLANE_Z, constant depth maps: the projective distance is exact, the plane crosses
    every active cell, so every vertex is within sqrt(3) s of it.  Voxels beyond -trunc behind it stay unseen."""
    vol, views = sc.plane_case()
    fused = so.integrate(vol, views, np.float64)
    assert fused["weight"].max() == 3.0 and (fused["weight"] == 0).any()
    seen = fused["weight"] > 0
    z = vol["origin"][2] + (np.arange(vol["dims"][2]) + 0.5) * vol["s"]
    want = np.minimum(1.0, (sc.PLANE_Z - z) / vol["trunc"])[:, None, None] * np.ones_like(fused["tsdf"])
    assert np.abs(fused["tsdf"] - want)[seen].max() <= 1e-6
    assert not seen[z > sc.PLANE_Z + vol["trunc"] + 1e-6].any()
    mesh = so.extract(dict(vol, **{k: (None if fused[k] is None else fused[k].astype(np.float32)) for k in ("tsdf", "weight", "color", "cweight")}),
                      1.0, np.float64)
    assert len(mesh["vertices"]) >= 50 and len(mesh["faces"]) >= 50
    assert np.abs(mesh["vertices"][:, 2] - sc.PLANE_Z).max() <= math.sqrt(3.0) * vol["s"]
    assert np.abs(mesh["normals"][:, 2] + 1.0).max() <= 1e-5          # the distance grows towards the cameras, at -z
    assert mesh["colors"].min() >= 0.25 - 1e-6 and mesh["colors"].max() <= 0.75 + 1e-6


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_sphere_mesh_is_closed_manifold_and_wound_outwards(dtype):
    vol, mw = sc.extract_case("sphere", (17, 9, 33))
    mesh = so.extract(vol, mw, dtype)
    r = so.mesh_report(mesh["vertices"], mesh["faces"], sc.sphere_centre(vol))
    assert r["F"] >= 200 and r["used"]
    assert r["edge_uses"] == {2}, r                          # every undirected edge is in exactly two triangles
    assert r["euler"] == 2, r
    assert r["min_outward"] > 0, r
    c = np.asarray(sc.sphere_centre(vol))
    radial = (mesh["vertices"] - c) / np.linalg.norm(mesh["vertices"] - c, axis=1, keepdims=True)
    assert (mesh["normals"] * radial).sum(1).min() > 0.9
    assert np.abs(np.linalg.norm(mesh["vertices"] - c, axis=1) - sc.SPHERE_RADIUS * vol["s"]).max() <= 0.5 * vol["s"]


def test_extraction_edge_cases_of_the_statement():
    for dims in ((2, 2, 2), (5, 1, 4)):
        for kind in sc.EXTRACT_KINDS:
            vol, mw = sc.extract_case(kind, dims)
            mesh = so.extract(vol, mw, np.float64)
            assert len(mesh["faces"]) == 0                   # a quad needs four cells around an edge: at least 3 voxels across
            assert len(mesh["vertices"]) <= 1 and (min(dims) >= 2 or len(mesh["vertices"]) == 0)
    for kind in ("plane_slab", "random", "min_weight"):
        vol, mw = sc.extract_case(kind, (17, 9, 33))
        m64, m32 = sc.extract_refs(kind, (17, 9, 33))
        assert len(m64["faces"]) >= 100 and np.array_equal(m64["faces"], m32["faces"])
        assert m64["faces"].min() >= 0 and m64["faces"].max() < len(m64["vertices"])
        r = so.mesh_report(m64["vertices"], m64["faces"])
        assert r["edge_uses"] <= {1, 2, 3, 4}


@pytest.mark.parametrize("name", sorted(sc.INTEGRATE_CASES))
def test_shared_integration_inputs_keep_cliff_voxels_rare(name):
    """At most 2 % of a case's voxels sit on a decision threshold; the cases reach the branches they are there for."""
    vol, views = sc.integrate_case(name)
    r64, r32 = sc.integrate_refs(name)
    share = float(r64["flag"].mean())
    print("%-7s cliff voxels %.2f %%, seen %.0f %%" % (name, 100 * share, 100 * float((r64["weight"] > 0).mean())))
    assert share <= 0.02
    assert (r64["weight"] > 0).any()
    ok = ~r64["flag"]
    assert np.array_equal(r64["weight"][ok], r32["weight"][ok].astype(np.float64))
    if name in ("full", "chunk"):
        assert (r64["weight"] == 0).any() and len(np.unique(r64["weight"])) >= 4
        assert (r64["cweight"] < r64["weight"]).any()                                 # d = 1: distance without colour
    if name == "chunk":
        last = so.integrate(vol, views[:sc.CHUNK], np.float64)
        assert (last["weight"] != r64["weight"]).any()                                # the view beyond the chunk reaches the volume


def test_mesh_ply_round_trip_is_exact(tmp_path):
    from fdgs import surface
    g = torch.Generator().manual_seed(3)
    mesh = surface.Mesh(torch.randn(7, 3, generator=g), torch.nn.functional.normalize(torch.randn(7, 3, generator=g), dim=1),
                        torch.randint(0, 256, (7, 3), generator=g).float() / 255.0, torch.randint(0, 7, (5, 3), generator=g).int())
    path = str(tmp_path / "mesh.ply")
    surface.save_mesh_ply(path, mesh)
    with open(path, "rb") as f:
        head = f.read().split(b"end_header\n")[0].decode("ascii")
    assert head.startswith("ply\nformat binary_little_endian 1.0\nelement vertex 7\n")
    assert "property uchar red" in head and "element face 5\nproperty list uchar int vertex_indices" in head
    assert os.path.getsize(path) == len(head) + len("end_header\n") + 7 * 27 + 5 * 13
    back = surface.load_mesh_ply(path, "cpu")
    for k in ("vertices", "normals", "colors", "faces"):
        assert getattr(back, k).dtype == getattr(mesh, k).dtype and torch.equal(getattr(back, k), getattr(mesh, k)), k
    empty = surface.Mesh(torch.zeros(0, 3), torch.zeros(0, 3), torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32))
    surface.save_mesh_ply(path, empty)
    assert surface.load_mesh_ply(path, "cpu").faces.shape == (0, 3)


def test_header_library_and_binding_list_carry_the_surface_calls():
    from fdgs import _capi
    with open(os.path.join(ROOT, "include", "fdgs.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(fdgs_[a-z_0-9]+)\s*\(", text))
    for sym in SYMBOLS:
        assert sym in declared, "include/fdgs.h does not declare %s" % sym
        assert sym in _capi.EXPORTED and hasattr(_capi.lib, sym), sym
    for struct in ("fdgs_tsdf_volume", "fdgs_tsdf_view", "fdgs_surface_out"):
        assert re.search(r"typedef struct %s\s*\{\s*uint32_t struct_size;" % struct, text), struct
    assert _capi.lib.fdgs_version() == _capi.FDGS_VERSION == 502
    with open(os.path.join(ROOT, "4d-gaussian-splatting_amd", "csrc", "build.sh")) as f:
        sh = f.read()
    assert re.search(r"for src in [^;]*\btsdf\b[^;]*; do", sh) and re.search(r'\[tsdf\]="[^"]*-ffp-contract=off', sh)
    lib = _capi.lib
    assert lib.fdgs_surface_extract_scratch_bytes(1, 5, 3) == 0 and lib.fdgs_surface_extract_scratch_bytes(-1, 5, 3) == 0
    small, big = lib.fdgs_surface_extract_scratch_bytes(2, 2, 2), lib.fdgs_surface_extract_scratch_bytes(256, 256, 256)
    assert 0 < small < big and small % 256 == 0 and 4 * 256 ** 3 <= big < 4.1 * 256 ** 3


def test_struct_sizes_and_argument_errors_without_touching_the_gpu():
    """Every bad argument is FDGS_ERR_INVALID_ARG before anything is launched (the pointers here are not device memory)."""
    from fdgs import _capi
    lib = _capi.lib
    for cls, size in ((_capi.FdgsTsdfVolume, 72), (_capi.FdgsTsdfView, 80), (_capi.FdgsSurfaceOut, 64)):
        assert cls().struct_size == C.sizeof(cls) == size and cls._fields_[0][0] == "struct_size"

    def volume(**kw):
        v = _capi.FdgsTsdfVolume(4, 4, 4, 0.0, 0.0, 0.0, 0.1, 0.4, 64, 64, 64, 64)
        for k, x in kw.items():
            setattr(v, k, x)
        return v

    def view(**kw):
        v = _capi.FdgsTsdfView(4, 4, 64, 64, None, None, 64, 0.5, 10.0, 10.0, 2.0, 2.0, 1.0)
        for k, x in kw.items():
            setattr(v, k, x)
        return v

    def out(**kw):
        o = _capi.FdgsSurfaceOut(0, 0, None, None, None, None, 64, 64)
        for k, x in kw.items():
            setattr(o, k, x)
        return o
    integrate = lambda vol, v=None, n=1: lib.fdgs_tsdf_integrate(C.byref(vol), n, C.byref(v if v is not None else view()), None)  # noqa: E731
    extract = lambda vol, o=None, mw=1.0, scratch=64: lib.fdgs_surface_extract(C.byref(vol), mw, C.byref(o if o is not None else out()), scratch, None)  # noqa: E731
    inf, nan = float("inf"), float("nan")
    bad_volumes = (dict(tsdf=None), dict(weight=None), dict(trunc=0.0), dict(trunc=-1.0), dict(trunc=nan), dict(voxel_size=0.0),
                   dict(voxel_size=inf), dict(color=None), dict(cweight=None), dict(nx=-1), dict(nz=-3), dict(nx=1024, ny=1024, nz=256),
                   dict(nx=70000, ny=70000), dict(ox=nan))
    for name, call in (("fdgs_tsdf_integrate", integrate), ("fdgs_surface_extract", extract)):
        for delta in (-4, 8):
            v = volume()
            v.struct_size += delta
            assert call(v) == 1, name
            assert "struct_size" in _capi.last_error() and "fdgs_tsdf_volume" in _capi.last_error() and name in _capi.last_error()
        for bad in bad_volumes:
            assert call(volume(**bad)) == 1, (name, bad)
            assert name in _capi.last_error()
    assert lib.fdgs_tsdf_integrate(None, 0, None, None) == 1
    assert lib.fdgs_tsdf_integrate(C.byref(volume()), -1, None, None) == 1
    assert lib.fdgs_tsdf_integrate(C.byref(volume()), 1, None, None) == 1
    for delta in (-4, 8):
        v = view()
        v.struct_size += delta
        assert integrate(volume(), v) == 1 and "fdgs_tsdf_view" in _capi.last_error()
    for bad in (dict(depth=None), dict(viewmatrix=None), dict(H=0), dict(W=-2), dict(H=40000, W=40000), dict(alpha_min=0.0), dict(alpha_min=nan),
                dict(fl_x=0.0), dict(fl_y=inf), dict(cx=nan), dict(cy=inf), dict(view_weight=0.0), dict(view_weight=-1.0), dict(view_weight=nan)):
        assert integrate(volume(), view(**bad)) == 1, bad
    views = (_capi.FdgsTsdfView * 3)(view(), view(), view(depth=None))          # the bad view is the last one: all are checked first
    assert lib.fdgs_tsdf_integrate(C.byref(volume()), 3, views, None) == 1
    assert integrate(volume(), view(alpha=None, alpha_min=0.0), n=0) == 0       # no alpha: alpha_min is not looked at; nothing to do
    assert integrate(volume(nx=0), view()) == 0                                 # an empty volume: nothing is launched
    assert lib.fdgs_surface_extract(C.byref(volume()), 1.0, None, 64, None) == 1
    for delta in (-4, 8):
        o = out()
        o.struct_size += delta
        assert extract(volume(), o) == 1 and "fdgs_surface_out" in _capi.last_error()
    for bad in (dict(n_vertices=None), dict(n_faces=None), dict(vertex_capacity=-1), dict(face_capacity=-1)):
        assert extract(volume(), out(**bad)) == 1, bad
    assert extract(volume(), mw=nan) == 1 and "min_weight" in _capi.last_error()
    assert extract(volume(), scratch=None) == 1 and "scratch" in _capi.last_error()


def test_cpu_tensors_are_refused():
    from fdgs import surface, synth
    with pytest.raises(RuntimeError, match="no CPU path"):
        surface.TSDFVolume((0, 0, 0), 0.1, (4, 4, 4), device="cpu")
    vol = surface.TSDFVolume.__new__(surface.TSDFVolume)
    vol.device = torch.device("cuda", 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        surface.integrate(vol, [{"depth": torch.ones(1, 4, 4), "camera": synth.camera_for("axis", 4, 4)}])
