"""The inputs tests/test_mesh_host.py and tests/test_gpu_mesh.py share: seeded meshes (dicts of numpy arrays, tests/mesh_oracle.py) and
their references.  A case is built once (lru_cache) and never modified.

The smallest shapes at which the kernels can go wrong: nothing at all, vertices without faces, one triangle, one vertex past a
workgroup (257) and past four (1025), a long chain in permuted and in natural numbering (the union-find's worst and best
case), equal components, absent faces, a fan of valence 80 (a row longer than a wave), a vertex of valence 1 and one in no face.
One case is past a scan chunk: a chunk is 1024 workgroup counts, 262 144 elements, and "v262145" has one vertex more.
"""
import functools

import numpy as np

import mesh_oracle as mo
import surface_cases as sc

EXTRACT_DIMS = (17, 9, 33)
ABSENT = (-1, None, 2 ** 30)         # indices an absent face carries (None: V itself)


def make_mesh(vertices, faces, seed=0):
    """A mesh dict around ``vertices`` / ``faces`` with seeded unit normals and colours (what compaction has to carry along)."""
    rng = np.random.default_rng(seed)
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    n = rng.standard_normal(v.shape)
    n = (n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-9)).astype(np.float32)
    return {"vertices": v, "normals": n, "colors": rng.uniform(0, 1, v.shape).astype(np.float32),
            "faces": np.asarray(faces, np.int32).reshape(-1, 3)}


def strip(quads, permute_seed=None):
    """A strip of ``quads`` quads (two triangles each) over 2 (quads + 1) vertices; with a seed the vertices are renumbered at random."""
    i = np.arange(quads)
    top, bot = 2 * i, 2 * i + 1
    faces = np.stack([np.stack([top, bot, top + 2], 1), np.stack([bot, bot + 2, top + 2], 1)], 1).reshape(-1, 3)
    V = 2 * (quads + 1)
    x = np.arange(V) // 2
    verts = np.stack([0.1 * x, 0.1 * (np.arange(V) % 2), 0.01 * np.sin(0.7 * x)], 1)
    if permute_seed is not None:
        perm = np.random.default_rng(permute_seed).permutation(V)          # old -> new
        faces = perm[faces]
        verts = verts[np.argsort(perm)]
    return make_mesh(verts, faces, seed=quads)


def blocks(V, seed, block=37, per_block=30):
    """V vertices in blocks of ``block``; the faces of a block pick their corners inside it (some twice: repeated indices), so there
    are about V / block components plus the vertices no face picked."""
    rng = np.random.default_rng(seed)
    faces = []
    for lo in range(0, V, block):
        hi = min(V, lo + block)
        faces.append(rng.integers(lo, hi, (per_block, 3)))
    faces = rng.permutation(np.concatenate(faces))
    return make_mesh(rng.uniform(-1, 1, (V, 3)), faces, seed=seed)


SCAN_CHUNK = 1024 * 256              # elements whose workgroup counts fill one chunk of the scan: one more needs its carry


def islands(V, seed, groups=96, block=12, per_group=4):
    """V vertices, nearly all in no face; ``groups`` windows of ``block`` consecutive vertices spread evenly over [0, V), the last one
    ending at V - 1, each with ``per_group`` faces inside it.  A few hundred faces: the sequential union-find of the oracle takes them
    in no time, the kernels' vertex scans run over all V."""
    rng = np.random.default_rng(seed)
    los = np.linspace(0, V - block, groups).astype(np.int64)
    faces = np.concatenate([lo + np.stack([rng.permutation(block)[:3] for _ in range(per_group)]) for lo in los])
    faces[-1] = [V - 1, V - 3, V - 2]
    return make_mesh(rng.uniform(-1, 1, (V, 3)), rng.permutation(faces), seed=seed)


def fan(rim, closed, seed=5):
    """A centre (vertex 0) with ``rim`` vertices around it, slightly out of plane; closed: the last triangle joins the first."""
    rng = np.random.default_rng(seed)
    a = 2 * np.pi * np.arange(rim) / rim
    verts = np.concatenate([[[0.0, 0.0, 0.3]], np.stack([np.cos(a), np.sin(a), 0.05 * rng.standard_normal(rim)], 1)])
    k = np.arange(rim if closed else rim - 1)
    faces = np.stack([np.zeros_like(k), 1 + k, 1 + (k + 1) % rim], 1)
    return make_mesh(verts, faces, seed=seed)


def join(*meshes):
    """The disjoint union, vertex indices shifted."""
    out, off, faces = {k: [] for k in ("vertices", "normals", "colors")}, 0, []
    for m in meshes:
        for k in out:
            out[k].append(m[k])
        faces.append(m["faces"] + off)
        off += len(m["vertices"])
    res = {k: np.concatenate(v) for k, v in out.items()}
    res["faces"] = np.concatenate(faces).astype(np.int32)
    return res


def grid(nx, ny, s=0.1):
    """A flat regular grid in the plane z = 0.25, every cell split along the same diagonal."""
    j, i = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    verts = np.stack([s * i.ravel(), s * j.ravel(), np.full(nx * ny, 0.25)], 1)
    v = (j[:-1, :-1] * nx + i[:-1, :-1]).ravel()
    faces = np.stack([np.stack([v, v + 1, v + nx + 1], 1), np.stack([v, v + nx + 1, v + nx], 1)], 1).reshape(-1, 3)
    return make_mesh(verts, faces, seed=nx)


def with_absent(mesh, seed=3, every=7):
    """``mesh`` with absent faces mixed in (one after every ``every`` faces): indices -1, V and 2^30 in any corner."""
    rng = np.random.default_rng(seed)
    V, faces, out = len(mesh["vertices"]), mesh["faces"], []
    for n, f in enumerate(faces.tolist()):
        out.append(f)
        if n % every == 0:
            bad = list(rng.integers(0, max(V, 1), 3))
            code = ABSENT[(n // every) % 3]
            bad[(n // every) % 3] = V if code is None else code
            if (n // every) % 5 == 0:
                bad = [V if c is None else c for c in ABSENT]          # all three out of range
            out.append(bad)
    return dict(mesh, faces=np.asarray(out, np.int64).astype(np.int32).reshape(-1, 3))


@functools.lru_cache(maxsize=None)
def extracted(kind):
    """The float32 mesh surface nets give for surface_cases.extract_case(kind, (17, 9, 33))."""
    m = sc.extract_refs(kind, EXTRACT_DIMS)[1]
    return {k: np.ascontiguousarray(m[k], np.float32 if k != "faces" else np.int32) for k in ("vertices", "normals", "colors", "faces")}


def floater():
    """A closed shell of 12 faces: a hexagonal bipyramid."""
    a = 2 * np.pi * np.arange(6) / 6
    verts = np.concatenate([np.stack([0.02 * np.cos(a), 0.02 * np.sin(a), np.zeros(6)], 1), [[0, 0, 0.02], [0, 0, -0.02]]]) + 0.4
    k = np.arange(6)
    faces = np.concatenate([np.stack([k, (k + 1) % 6, np.full(6, 6)], 1), np.stack([(k + 1) % 6, k, np.full(6, 7)], 1)])
    return make_mesh(verts, faces, seed=12)


def noisy_sphere(amplitude=0.15, seed=21):
    """The extracted sphere with seeded radial noise of ``amplitude`` voxels; returns (mesh, centre)."""
    vol, _ = sc.extract_case("sphere", EXTRACT_DIMS)
    m, c = extracted("sphere"), np.asarray(sc.sphere_centre(vol))
    d = m["vertices"].astype(np.float64) - c
    r = np.linalg.norm(d, axis=1, keepdims=True)
    noise = amplitude * vol["s"] * np.random.default_rng(seed).standard_normal((len(d), 1))
    return dict(m, vertices=(c + d / r * (r + noise)).astype(np.float32)), c


@functools.lru_cache(maxsize=None)
def topology_case(name):
    """The meshes the component and compaction tests run on."""
    if name in ("sphere", "random", "min_weight"):
        return extracted(name)
    if name == "empty":
        return make_mesh(np.zeros((0, 3)), np.zeros((0, 3)))
    if name == "no_faces":
        return make_mesh(np.random.default_rng(1).uniform(-1, 1, (300, 3)), np.zeros((0, 3)))
    if name == "triangle":
        return make_mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]])
    if name == "v257":
        return blocks(257, seed=257)
    if name == "v1025":
        return blocks(1025, seed=1025)
    if name == "v262145":
        return islands(SCAN_CHUNK + 1, seed=262145)
    if name == "strip_permuted":
        return strip(5000, permute_seed=11)
    if name == "strip_natural":
        return strip(5000)
    if name == "equal_pair":
        return join(fan(6, False), fan(6, False, seed=6))
    if name == "absent":
        return with_absent(blocks(257, seed=258))
    if name == "absent_random":
        return with_absent(extracted("random"))
    raise KeyError(name)


TOPOLOGY_CASES = ("sphere", "random", "min_weight", "empty", "no_faces", "triangle", "v257", "v1025", "strip_permuted", "strip_natural",
                  "equal_pair", "absent", "absent_random")
CHUNK_CASES = ("v262145",)           # past a scan chunk: V = 1025 workgroups of vertices, F = 2 workgroups of faces (GPU tests only)
CLEAN_CHOICES = ({}, {"keep_largest": 1}, {"keep_largest": 3, "min_faces": 5}, {"min_faces": 25})


@functools.lru_cache(maxsize=None)
def topology_refs(name):
    m = topology_case(name)
    return mo.components(len(m["vertices"]), m["faces"])


@functools.lru_cache(maxsize=None)
def smooth_case(name):
    """The meshes the smoothing tests run on.  "mixed": a closed fan of valence 80, an open fan (boundary; its rim ends have
    valence 1), a lone triangle (valence 1 everywhere), two vertices in no face and some absent faces."""
    if name == "sphere":
        return noisy_sphere()[0]
    if name == "random":
        return extracted("random")
    if name == "grid":
        return grid(9, 7)
    if name == "mixed":
        lone = make_mesh(np.random.default_rng(2).uniform(2, 3, (2, 3)), np.zeros((0, 3)))
        tri = make_mesh([[3, 0, 0], [4, 0.1, 0], [3, 1, 0.2]], [[0, 1, 2]])
        return with_absent(join(fan(80, True), lone, fan(9, False, seed=8), tri), every=20)
    raise KeyError(name)


SMOOTH_CASES = ("sphere", "random", "grid", "mixed")
SMOOTH_RUNS = ((0, True), (1, True), (1, False), (10, True), (10, False))      # (iterations, pin_boundary)
LAMBDA, MU = 0.5, -0.53


@functools.lru_cache(maxsize=None)
def smooth_refs(name, iterations, pin):
    """The float64 truth and the float32 statement; computed once, shared, read-only."""
    m = smooth_case(name)
    return (mo.smooth(m["vertices"], m["faces"], iterations, LAMBDA, MU, pin, np.float64),
            mo.smooth(m["vertices"], m["faces"], iterations, LAMBDA, MU, pin, np.float32))
