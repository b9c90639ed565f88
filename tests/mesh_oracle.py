"""numpy statement of the mesh calls of fdgs.surface (csrc/mesh.hip), written from their definition in include/fdgs.h: connected
components (a sequential union-find), component filtering with order-preserving compaction, Taubin smoothing with recomputed normals.

A mesh is a dict: ``vertices``, ``normals``, ``colors`` [V, 3] float32 and ``faces`` [F, 3] int32.  A face with an index outside
[0, V) is absent.  ``smooth`` takes a ``dtype``: float64 is the truth, float32 is "the float32 statement" -- the same operations in the
same order on float32 values, whose distance from the truth is the error bar of the kernels (tests/test_gpu_mesh.py).
"""
import numpy as np


def present(faces, V):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < V)).all(1)


def components(V, faces):
    """{"vertex_component" [V] int32, "n", "vertex_counts" [n], "face_counts" [n]}: dense ids in ascending order of each
    component's smallest vertex index; a face counts for the component of its first index."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[present(f, V)]
    parent = list(range(V))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b, c in f.tolist():
        for u, w in ((a, b), (a, c)):
            ru, rw = find(u), find(w)
            if ru != rw:
                parent[max(ru, rw)] = min(ru, rw)
    root = np.array([find(v) for v in range(V)], np.int64).reshape(V)
    is_root = root == np.arange(V)
    dense = np.cumsum(is_root) - 1
    vc = dense[root].astype(np.int32) if V else np.zeros(0, np.int32)
    n = int(is_root.sum())
    return {"vertex_component": vc, "n": n, "vertex_counts": np.bincount(vc, minlength=n).astype(np.int32),
            "face_counts": np.bincount(vc[f[:, 0]], minlength=n).astype(np.int32)}


def compact(mesh, vertex_component, keep):
    """The mesh of the kept components and the old-to-new vertex map (-1: dropped)."""
    V = len(mesh["vertices"])
    vc, keep = np.asarray(vertex_component, np.int64), np.asarray(keep).astype(bool)
    kv = np.zeros(V, bool)
    ok = (vc >= 0) & (vc < len(keep))
    kv[ok] = keep[vc[ok]]
    f = np.asarray(mesh["faces"], np.int64).reshape(-1, 3)
    kf = present(f, V)
    kf[kf] = kv[f[kf, 0]]
    vmap = np.where(kv, np.cumsum(kv) - 1, -1)
    out = {k: mesh[k][kv] for k in ("vertices", "normals", "colors")}
    out["faces"] = vmap[f[kf]].astype(np.int32).reshape(-1, 3)
    return out, vmap


def keep_mask(face_counts, keep_largest=None, min_faces=None):
    fc = np.asarray(face_counts, np.int64)
    keep = fc > 0
    if min_faces is not None:
        keep &= fc >= min_faces
    if keep_largest is not None:
        largest = np.zeros(len(fc), bool)
        largest[np.argsort(-fc, kind="stable")[:keep_largest]] = True      # ties: the smaller id first
        keep &= largest
    return keep


def clean(mesh, keep_largest=None, min_faces=None):
    c = components(len(mesh["vertices"]), mesh["faces"])
    return compact(mesh, c["vertex_component"], keep_mask(c["face_counts"], keep_largest, min_faces))[0]


def incidences(V, faces):
    """The rows of the vertex-to-face incidence structure: (row_start [V + 1], face [n], o1 [n], o2 [n]) with the incidences
    (vertex, 3 face + corner) of the present faces in ascending order; o1, o2 are the face's other corners in ascending corner index."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ids = np.nonzero(present(f, V))[0]
    key = f[ids].reshape(-1)
    val = (3 * ids[:, None] + np.arange(3)[None, :]).reshape(-1)
    order = np.argsort(key, kind="stable")
    key, val = key[order], val[order]
    face, k = val // 3, val % 3
    o1 = f[face, np.where(k == 0, 1, 0)]
    o2 = f[face, np.where(k == 2, 1, 2)]
    return np.searchsorted(key, np.arange(V + 1)), face, o1, o2


def boundary(V, faces):
    """[V] uint8: 1 where some index occurs among the other corners of exactly one incidence of the vertex's row."""
    rs, _, o1, o2 = incidences(V, faces)
    out = np.zeros(V, np.uint8)
    for v in range(V):
        a, b = o1[rs[v]:rs[v + 1]], o2[rs[v]:rs[v + 1]]
        for u in np.unique(np.concatenate([a, b])):
            if int(((a == u) | (b == u)).sum()) == 1:
                out[v] = 1
                break
    return out


def _row_sums(rs, terms, dtype):
    """Per row the sum of ``terms`` [n, 3] in row order: S = S + term, one row position at a time."""
    deg = np.diff(rs)
    S = np.zeros((len(deg), 3), dtype)
    for j in range(int(deg.max()) if len(deg) else 0):
        has = deg > j
        S[has] = S[has] + terms[rs[:-1][has] + j]
    return S, deg


def smooth(vertices, faces, iterations, lam, mu, pin_boundary, dtype):
    """{"vertices", "normals" [V, 3] of ``dtype``, "boundary" [V] uint8, "flag" [V] bool}: flag marks the vertices whose normal is a
    near-cancelling sum (its length before normalisation is below 1e-6 of the largest incident face's area; dtype float64)."""
    dt = np.dtype(dtype).type
    V = len(vertices)
    p = np.asarray(vertices, np.float32).astype(dtype).reshape(V, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    rs, face, o1, o2 = incidences(V, f)
    bnd = boundary(V, f)
    deg = np.diff(rs)
    move = (deg > 0) & ~((bnd > 0) & bool(pin_boundary))
    for it in range(2 * iterations):
        t = dt(np.float32(mu if it & 1 else lam))
        S, _ = _row_sums(rs, p[o1] + p[o2], dtype)
        with np.errstate(all="ignore"):
            m = S / (2 * deg).astype(dtype)[:, None]
            q = p + t * (m - p)
        p = np.where(move[:, None], q, p)
    a, b, c = (p[f[face, k]] for k in range(3))
    u, w = b - a, c - a
    cr = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
    N, _ = _row_sums(rs, cr, dtype)
    len2 = (N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2]
    ok = len2 > 0
    ln = np.sqrt(np.where(ok, len2, dt(1)))
    nrm = np.where(ok[:, None], N / ln[:, None], dt(0))
    area = 0.5 * np.sqrt((cr.astype(np.float64) ** 2).sum(1))
    largest = np.zeros(V)
    if len(face):
        np.maximum.at(largest, np.repeat(np.arange(V), deg), area)
    flag = (deg > 0) & (np.sqrt(len2.astype(np.float64)) < 1e-6 * largest)
    return {"vertices": p, "normals": nrm, "boundary": bnd, "flag": flag}


def volume(vertices, faces):
    """The signed volume a closed, outward-wound mesh encloses."""
    v, f = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)
    return float((v[f[:, 0]] * np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)
