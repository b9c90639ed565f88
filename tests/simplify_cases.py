"""The inputs tests/test_simplify_host.py and tests/test_gpu_simplify.py share: seeded meshes with their grids, and their references
(tests/simplify_oracle.py).  A case is built once (lru_cache) and never modified.

The smallest shapes at which each pass of csrc/mesh_simplify.hip can go wrong: nothing, vertices without faces, a triangle inside one
cell and one across three, strips of 257 and 1025 vertices (one position past a workgroup, past four), the 5000-quad strip in natural
and permuted numbering on a grid of 92 160 cells (ten sort chunks, a third radix pass), a closed sphere at two cell sizes, a cube with
sharp edges, two coincident sheets of opposite winding, literal and rotated duplicate faces, absent faces with a NaN and an Inf vertex,
vertices exactly on cell boundaries, vertices outside the grid, a grid one cell thick, a fan of valence 80, faces of zero area.
None of these is past a scan chunk (1024 workgroup counts, 262 144 elements); "grid_chunk", a flat grid of 262 145 vertices, is.
"""
import functools

import numpy as np

import mesh_cases as mc
import simplify_oracle as so


def strip_v(V):
    """The first V vertices of a strip, with the faces that stay inside them."""
    m = mc.strip((V + 1) // 2)
    keep = (m["faces"] < V).all(1)
    return {"vertices": m["vertices"][:V], "normals": m["normals"][:V], "colors": m["colors"][:V], "faces": m["faces"][keep]}


def uv_sphere(n_lat=36, n_lon=36, r=1.0, seed=31):
    """A closed sphere of 2 n_lon (n_lat - 1) faces, outward wound, with its exact normals and seeded colours."""
    th = np.pi * np.arange(1, n_lat) / n_lat
    ph = 2 * np.pi * np.arange(n_lon) / n_lon
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(n_lon))], 2).reshape(-1, 3)
    verts = np.concatenate([[[0, 0, 1.0]], ring, [[0, 0, -1.0]]])
    idx = lambda i, j: 1 + i * n_lon + (j % n_lon)  # noqa: E731
    faces = [[0, idx(0, j), idx(0, j + 1)] for j in range(n_lon)]
    for i in range(n_lat - 2):
        for j in range(n_lon):
            faces += [[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], [idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)]]
    last = len(verts) - 1
    faces += [[last, idx(n_lat - 2, j + 1), idx(n_lat - 2, j)] for j in range(n_lon)]
    m = mc.make_mesh(r * verts, faces, seed=seed)
    m["normals"] = verts.astype(np.float32)
    return m


def cube(m=12, seed=41):
    """The surface of [0, 1]^3, every side m x m quads, the sides sharing their edge vertices; outward wound."""
    pos, faces = {}, []

    def vid(p):
        key = tuple(int(round(c * m)) for c in p)
        return pos.setdefault(key, len(pos))
    for axis in range(3):
        for side in (0, 1):
            u, w = [(1, 2), (2, 0), (0, 1)][axis]
            for i in range(m):
                for j in range(m):
                    q = []
                    for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = [0.0, 0.0, 0.0]
                        p[axis], p[u], p[w] = float(side), (i + di) / m, (j + dj) / m
                        q.append(vid(p))
                    if not side:
                        q = q[::-1]
                    faces += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    verts = np.array(sorted(pos, key=pos.get), np.float64) / m
    return mc.make_mesh(verts, faces, seed=seed)


CHUNK_GRID = (481, 545)               # 481 x 545 = 262 145 vertices = mc.SCAN_CHUNK + 1


def _duplicates():
    """A 4 x 4 grid whose faces 3, 8 and 11 come again: literally (at the end), rotated (at the end) and rotated BEFORE the original
    (inserted at the front) -- the survivor is the lowest index whichever form it has."""
    g = mc.grid(4, 4, s=0.25)
    f = g["faces"]
    extra_front = np.roll(f[11], 1)[None]
    faces = np.concatenate([extra_front, f, f[3][None], np.roll(f[8], -1)[None], f[3][None]])
    return dict(g, faces=faces.astype(np.int32))


def _zero_area():
    """A 5 x 5 grid with faces of zero area mixed in: repeated indices, and three different vertices on one line (dyadic coordinates:
    the cross product is exactly zero in float32 and in float64)."""
    g = mc.grid(5, 5, s=0.25)
    extra = np.array([[0, 0, 6], [7, 12, 7], [3, 3, 3], [0, 1, 2], [0, 6, 12], [5, 15, 10]], np.int32)
    return dict(g, faces=np.concatenate([g["faces"][:9], extra, g["faces"][9:]]).astype(np.int32))


def _unusable():
    """The sphere with absent faces mixed in, one vertex NaN and one with an Inf coordinate."""
    m = mc.with_absent(uv_sphere(12, 12, seed=32), every=9)
    v = m["vertices"].copy()
    v[5, 1] = np.nan
    v[40] = [0.5, np.inf, -0.25]
    return dict(m, vertices=v)


@functools.lru_cache(maxsize=None)
def case(name):
    """(mesh, origin [3] float32, h, dims)."""
    def auto(m, h):
        o, dims = so.default_grid(m["vertices"], h)
        return m, o, h, dims

    def fixed(m, origin, h, dims):
        return m, np.asarray(origin, np.float32), h, tuple(dims)
    if name == "empty":
        return fixed(mc.topology_case("empty"), (0, 0, 0), 1.0, (1, 1, 1))
    if name == "no_faces":
        return auto(mc.topology_case("no_faces"), 0.5)
    if name == "tri_one_cell":
        return fixed(mc.make_mesh([[0.25, 0.25, 0.5], [0.75, 0.25, 0.25], [0.25, 0.75, 0.75]], [[0, 1, 2]]), (0, 0, 0), 1.0, (2, 2, 1))
    if name == "tri_three_cells":
        return fixed(mc.make_mesh([[0.25, 0.25, 0.25], [1.25, 0.25, 0.25], [0.25, 1.25, 0.25]], [[0, 1, 2]]), (0, 0, 0), 1.0, (2, 2, 1))
    if name == "strip257":
        return auto(strip_v(257), 0.07)
    if name == "strip1025":
        return auto(strip_v(1025), 0.09)
    if name == "strip_natural":
        return fixed(mc.topology_case("strip_natural"), (-1, -1, -1), 0.35, (1440, 8, 8))
    if name == "strip_permuted":
        return fixed(mc.topology_case("strip_permuted"), (-1, -1, -1), 0.35, (1440, 8, 8))
    if name == "sphere_fine":
        return auto(uv_sphere(), 0.25)
    if name == "sphere_coarse":
        return auto(uv_sphere(), 0.6)
    if name == "cube":
        return fixed(cube(), (-0.125, -0.125, -0.125), 0.25, (5, 5, 5))
    if name == "two_sheets":
        g = mc.grid(9, 7)
        return auto(mc.join(g, dict(g, faces=g["faces"][:, ::-1])), 0.25)
    if name == "duplicates":
        return auto(_duplicates(), 0.125)
    if name == "unusable":
        return auto(_unusable(), 0.3)
    if name == "boundaries":
        return fixed(mc.grid(9, 7, s=0.125), (0, 0, 0), 0.25, (5, 4, 2))
    if name == "outside":
        return fixed(uv_sphere(16, 16, seed=33), (-0.5, -0.5, -0.5), 0.4, (3, 3, 3))
    if name == "one_thick":
        return fixed(uv_sphere(16, 16, seed=34), (-1.05, -1.05, -1.05), 0.4, (1, 6, 6))
    if name == "fan":
        return auto(mc.fan(80, True), 0.3)
    if name == "zero_area":
        return auto(_zero_area(), 0.5)
    if name == "grid_chunk":
        return auto(mc.grid(*CHUNK_GRID), 0.25)
    raise KeyError(name)


CASES = ("empty", "no_faces", "tri_one_cell", "tri_three_cells", "strip257", "strip1025", "strip_natural", "strip_permuted", "sphere_fine",
         "sphere_coarse", "cube", "two_sheets", "duplicates", "unusable", "boundaries", "outside", "one_thick", "fan", "zero_area")
STABILISE = 1e-3
# (case, placement, stabilise): every case under both placements, and stabilise = 0 where every cluster's A has full rank
RUNS = tuple((n, p, STABILISE) for n in CASES for p in (so.MEAN, so.QUADRIC)) + (("sphere_coarse", so.QUADRIC, 0.0),)
RUN_IDS = ["%s-%s-s%g" % (n, "quadric" if p else "mean", s) for n, p, s in RUNS]
# past a scan chunk (1024 workgroup counts = 262 144 elements; GPU tests only): the head pass runs over the V = 262 145 sorted
# positions (1025 counts), the face pass over F = 522 240 faces (2040 counts); about 42 000 clusters, fewer than a chunk of heads
CHUNK_RUNS = (("grid_chunk", so.QUADRIC, STABILISE),)
CHUNK_RUN_IDS = ["%s-%s-s%g" % (n, "quadric" if p else "mean", s) for n, p, s in CHUNK_RUNS]


@functools.lru_cache(maxsize=None)
def refs(name, placement, stabilise):
    """The float64 truth and the float32 statement; computed once, shared, read-only."""
    m, origin, h, dims = case(name)
    return (so.simplify(m, origin, h, dims, placement, stabilise, np.float64), so.simplify(m, origin, h, dims, placement, stabilise, np.float32))
