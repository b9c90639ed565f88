"""numpy statement of fdgs.surface (csrc/tsdf.hip), written from its definition: TSDF integration of depth views and surface nets.

Both functions take a ``dtype``: float64 is the truth, float32 is "the float32 statement" -- the same operations in the same order
on float32 values, whose distance from the truth is the error bar of the kernels (tests/test_gpu_surface.py).  Inputs are float32
either way (they are what the kernels receive).

A volume is a dict: ``dims`` (nx, ny, nz), ``origin``, ``s``, ``trunc`` and the arrays ``tsdf``, ``weight`` [nz, ny, nx], ``color``
[3, nz, ny, nx] or None, ``cweight``.  A view is a dict: ``depth`` [H, W], ``alpha`` / ``mask`` [H, W] or None, ``image`` [3, H, W] or
None, ``vm`` (the 4 x 4 world_view_transform as the rasterizer takes it: view = (p, 1) @ vm), ``intr`` = (fl_x, fl_y, cx, cy),
``alpha_min``, ``weight``.
"""
import numpy as np

NEAR = 0.2     # the rasterizer's near plane


def _near_int(x, eps):
    return np.abs(x - np.round(x)) < eps


def integrate(vol, views, dtype):
    """The volume's four arrays after ``views`` (in order), and the per-voxel cliff flag: some view's decision for that voxel sits
    within a hair of one of its thresholds, so a float32 evaluation may decide otherwise (meaningful for dtype float64)."""
    dt = np.dtype(dtype).type
    nx, ny, nz = vol["dims"]
    s, trunc = dt(np.float32(vol["s"])), dt(np.float32(vol["trunc"]))
    o = [dt(np.float32(v)) for v in vol["origin"]]
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    px = o[0] + (i.astype(dtype) + dt(0.5)) * s
    py = o[1] + (j.astype(dtype) + dt(0.5)) * s
    pz = o[2] + (k.astype(dtype) + dt(0.5)) * s
    t, wt = vol["tsdf"].astype(dtype), vol["weight"].astype(dtype)
    has_color = vol.get("color") is not None
    col = vol["color"].astype(dtype) if has_color else None
    cw = vol["cweight"].astype(dtype) if has_color else None
    flag = np.zeros((nz, ny, nx), bool)
    with np.errstate(all="ignore"):
        for V in views:
            m = np.asarray(V["vm"], np.float32).astype(dtype)
            fl_x, fl_y, cx, cy = (dt(np.float32(v)) for v in V["intr"])
            w, amin = dt(np.float32(V["weight"])), dt(np.float32(V["alpha_min"]))
            H, W = V["depth"].shape
            z = ((m[0, 2] * px + m[1, 2] * py) + m[2, 2] * pz) + m[3, 2]
            x = ((m[0, 0] * px + m[1, 0] * py) + m[2, 0] * pz) + m[3, 0]
            y = ((m[0, 1] * px + m[1, 1] * py) + m[2, 1] * pz) + m[3, 1]
            flag |= np.abs(z - dt(NEAR)) < 1e-5
            live = z > dt(np.float32(NEAR))
            zs = np.where(live, z, dt(1))
            u, v = (fl_x * x) / zs + cx, (fl_y * y) / zs + cy
            flag |= live & (_near_int(u, 1e-3) | _near_int(v, 1e-3))         # (the image border is at integers)
            fu, fv = np.floor(u), np.floor(v)
            live &= (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
            iu, iv = np.where(live, fu, 0).astype(np.int64), np.where(live, fv, 0).astype(np.int64)
            zp = V["depth"].astype(dtype)[iv, iu]
            if V.get("alpha") is not None:
                a = V["alpha"].astype(dtype)[iv, iu]
                flag |= live & (np.abs(a - amin) < 1e-5)
                live &= a >= amin
                zp = zp / np.where(live, a, dt(1))
            if V.get("mask") is not None:
                live &= V["mask"][iv, iu] > 0
            live &= (zp > 0) & (zp < np.inf)
            sdf = zp - z
            flag |= live & ((np.abs(sdf + trunc) < 1e-4 * trunc) | (np.abs(sdf - trunc) < 1e-4 * trunc))
            live &= ~(sdf < -trunc)
            d = np.minimum(dt(1), sdf / trunc)
            wn = wt + w
            t = np.where(live, (wt * t + w * d) / wn, t)
            wt = np.where(live, wn, wt)
            if has_color and V.get("image") is not None:
                lc = live & (d < 1)
                cn = cw + w
                img = V["image"].astype(dtype)
                for c in range(3):
                    col[c] = np.where(lc, (cw * col[c] + w * img[c][iv, iu]) / cn, col[c])
                cw = np.where(lc, cn, cw)
    return {"tsdf": t, "weight": wt, "color": col, "cweight": cw, "flag": flag}


# the 12 edges of a cell, axis by axis: corner m0 (bit 0: +x, bit 1: +y, bit 2: +z) to m0 | (1 << axis)
EDGES = [(0, 0), (0, 2), (0, 4), (0, 6), (1, 0), (1, 1), (1, 4), (1, 5), (2, 0), (2, 1), (2, 2), (2, 3)]


def extract(vol, min_weight, dtype):
    """Surface nets: {"vertices" [V, 3], "normals", "colors", "faces" [F, 3] int32}."""
    dt = np.dtype(dtype).type
    nx, ny, nz = vol["dims"]
    empty = {"vertices": np.zeros((0, 3), dtype), "normals": np.zeros((0, 3), dtype), "colors": np.zeros((0, 3), dtype),
             "faces": np.zeros((0, 3), np.int32)}
    if min(nx, ny, nz) < 2:
        return empty
    s = dt(np.float32(vol["s"]))
    o = [dt(np.float32(v)) for v in vol["origin"]]
    T = vol["tsdf"].astype(dtype)
    known = (vol["weight"] >= np.float32(min_weight)) & (vol["weight"] > 0)
    inside = vol["tsdf"] < 0
    cell = lambda A, m: A[..., (m >> 2):nz - 1 + (m >> 2), ((m >> 1) & 1):ny - 1 + ((m >> 1) & 1), (m & 1):nx - 1 + (m & 1)]  # noqa: E731
    allk = np.ones((nz - 1, ny - 1, nx - 1), bool)
    cnt = np.zeros((nz - 1, ny - 1, nx - 1), int)
    for m in range(8):
        allk &= cell(known, m)
        cnt += cell(inside, m)
    active = allk & (cnt > 0) & (cnt < 8)
    nv = int(active.sum())
    cmap = np.full((nz, ny, nx), -1, np.int64)          # per voxel = per cell whose lowest corner it is
    sub = cmap[:nz - 1, :ny - 1, :nx - 1]
    sub[active] = np.arange(nv)                          # C order of [k, j, i]: x fastest
    k, j, i = (a[active] for a in np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij"))
    tv = [cell(T, m)[active] for m in range(8)]
    has_color = vol.get("color") is not None
    cv = [cell(vol["color"].astype(dtype), m)[:, active] for m in range(8)] if has_color else None
    ssum = [np.zeros(nv, dtype) for _ in range(3)]
    csum = [np.zeros(nv, dtype) for _ in range(3)]
    n = np.zeros(nv, dtype)
    with np.errstate(all="ignore"):
        for ax, m0 in EDGES:
            m1 = m0 | (1 << ax)
            fa, fb = tv[m0], tv[m1]
            cross = (fa < 0) != (fb < 0)
            tt = fa / np.where(cross, fa - fb, dt(1))
            for c in range(3):
                comp = tt if c == ax else np.full(nv, dt((m0 >> c) & 1))
                ssum[c] = np.where(cross, ssum[c] + comp, ssum[c])
                if has_color:
                    c0, c1 = cv[m0][c], cv[m1][c]
                    csum[c] = np.where(cross, csum[c] + (c0 + tt * (c1 - c0)), csum[c])
            n = n + cross.astype(dtype)
        verts = np.stack([o[c] + ((idx.astype(dtype) + dt(0.5)) + ssum[c] / n) * s for c, idx in enumerate((i, j, k))], 1)
        cols = np.stack([csum[c] / n for c in range(3)], 1)
        q = dt(0.25)
        gx = (((tv[1] - tv[0]) + (tv[3] - tv[2])) + ((tv[5] - tv[4]) + (tv[7] - tv[6]))) * q
        gy = (((tv[2] - tv[0]) + (tv[3] - tv[1])) + ((tv[6] - tv[4]) + (tv[7] - tv[5]))) * q
        gz = (((tv[4] - tv[0]) + (tv[5] - tv[1])) + ((tv[6] - tv[2]) + (tv[7] - tv[3]))) * q
        len2 = (gx * gx + gy * gy) + gz * gz
        ok = len2 > dt(np.float32(1e-20))
        ln = np.sqrt(np.where(ok, len2, dt(1)))
        nrm = np.stack([np.where(ok, g / ln, dt(0)) for g in (gx, gy, gz)], 1)
    # faces: every grid edge from voxel e along axis a, ascending 3 e + a
    K, J, I = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    dims = (nx, ny, nz)
    lin = lambda c: (c[2] * ny + c[1]) * nx + c[0]  # noqa: E731
    kn, ins, cm = known.ravel(), inside.ravel(), cmap.ravel()
    keys, quads = [], []
    for ax in range(3):
        b, e = (ax + 1) % 3, (ax + 2) % 3
        c = [I.ravel(), J.ravel(), K.ravel()]
        okv = (c[ax] < dims[ax] - 1) & (c[b] >= 1) & (c[b] <= dims[b] - 2) & (c[e] >= 1) & (c[e] <= dims[e] - 2)
        c = [a[okv] for a in c]
        v0 = lin(c)

        def moved(db, de, da=0):
            cc = list(c)
            cc[ax], cc[b], cc[e] = cc[ax] + da, cc[b] + db, cc[e] + de
            return lin(cc)
        v1 = moved(0, 0, 1)
        good = kn[v0] & kn[v1] & (ins[v0] != ins[v1])
        q0, q1, q2, q3 = cm[moved(-1, -1)], cm[moved(0, -1)], cm[v0], cm[moved(-1, 0)]    # counter-clockwise seen from +ax
        good &= (q0 >= 0) & (q1 >= 0) & (q2 >= 0) & (q3 >= 0)
        flip = ~ins[v0]                                  # the far end is the inside one: the normal points to -ax
        quads.append(np.stack([q0, np.where(flip, q3, q1), q2, np.where(flip, q1, q3)], 1)[good])
        keys.append(3 * v0[good] + ax)
    keys, quads = np.concatenate(keys), np.concatenate(quads)
    quads = quads[np.argsort(keys, kind="stable")]
    faces = np.stack([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]], 1).reshape(-1, 3).astype(np.int32)
    return {"vertices": verts, "normals": nrm, "colors": cols, "faces": faces}


def mesh_report(vertices, faces, centre=None):
    """Topology of a triangle mesh: {"V", "E", "F", "euler", "edge_uses" (set of how many triangles share an undirected edge),
    "used" (every vertex is in a face) and, with ``centre``, "min_outward": the least dot product of a face's geometric normal with
    the radius from ``centre`` to its centroid}."""
    v, f = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    uniq, uses = np.unique(e, axis=0, return_counts=True)
    r = {"V": len(v), "E": len(uniq), "F": len(f), "euler": len(v) - len(uniq) + len(f), "edge_uses": set(uses.tolist()),
         "used": len(np.unique(f)) == len(v)}
    if centre is not None:
        nrm = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
        r["min_outward"] = float(((v[f].mean(1) - np.asarray(centre, np.float64)) * nrm).sum(1).min())
    return r
