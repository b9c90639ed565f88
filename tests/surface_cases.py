"""The inputs tests/test_surface_host.py and tests/test_gpu_surface.py share: seeded volumes and views for the integration, float32
volumes for the extraction.  Everything is numpy / CPU torch; a case is built once (lru_cache) and never modified.

Integration cases keep the share of cliff voxels (tests/surface_oracle.integrate) at or below 2 % -- checked on the host.  A view
that covers the whole volume flags about 0.4 % of it (u or v within 1e-3 of an integer), so the 17-view case has three such views,
at positions 0, 15 and 16 (either side of the kernel's 16-view chunk), and fourteen that look away from the volume or sit inside it.
"""
import functools
import math

import numpy as np

CHUNK = 16                       # csrc/tsdf.hip TSDF_CHUNK
AWAY = dict(yaw=math.pi)         # at (0, 0, -4) looking down -z: the whole volume is behind it
INSIDE = dict(shift=(0.05, -0.02, 3.6))   # centre (0.05, -0.02, -0.4): inside or just in front of every volume here, part of which is
                                          # behind its near plane

# name -> dims, voxel size, image (W, H), poses, per-view weights, alpha, mask, image, colour volume
INTEGRATE_CASES = {
    "full": dict(dims=(33, 17, 9), s=0.06, image=(40, 24), poses=["rig1", "axis", INSIDE], weights=[1.0, 0.5, 2.0], alpha=True, mask=True,
                 rgb=True, color=True),
    "plain": dict(dims=(16, 16, 16), s=0.08, image=(40, 24), poses=["rig2"], weights=[1.0], alpha=False, mask=False, rgb=False, color=False),
    "chunk": dict(dims=(16, 16, 16), s=0.08, image=(40, 24), poses=["rig0"] + [AWAY] * 6 + [INSIDE] + [AWAY] * 7 + ["rig3", "axis"],
                  weights=[1.0, 1.5] * 8 + [0.5], alpha=True, mask=False, rgb=True, color=True),
    "tiny": dict(dims=(2, 2, 2), s=0.3, image=(1, 1), poses=["axis", "rig0", "axis"], weights=[1.0, 1.0, 3.0], alpha=True, mask=False, rgb=True,
                 color=True),
    "flat": dict(dims=(1, 5, 3), s=0.19, image=(40, 24), poses=["rig3"], weights=[2.0], alpha=False, mask=True, rgb=False, color=True),
    "onepix": dict(dims=(33, 17, 9), s=0.06, image=(1, 1), poses=["axis"], weights=[1.0], alpha=True, mask=True, rgb=True, color=True),
}
assert len(INTEGRATE_CASES["chunk"]["poses"]) == CHUNK + 1


def fresh_volume(dims, s, color=True, trunc=None):
    """An all-zero volume about the world origin, a fraction of a voxel off it: a lattice that is symmetric about a camera's axis puts
    whole planes of voxel centres on pixel borders.  (float32-representable origin, s and trunc: what the kernels receive.)"""
    nx, ny, nz = dims
    s = float(np.float32(s))
    vol = {"dims": tuple(dims), "s": s, "trunc": float(np.float32(4.0 * s if trunc is None else trunc)),
           "origin": tuple(float(np.float32((-0.5 * n + off) * s)) for n, off in zip(dims, (0.37, -0.21, 0.13))),
           "tsdf": np.zeros((nz, ny, nx), np.float32), "weight": np.zeros((nz, ny, nx), np.float32),
           "color": np.zeros((3, nz, ny, nx), np.float32) if color else None, "cweight": np.zeros((nz, ny, nx), np.float32) if color else None}
    return vol


def camera(pose, W, H):
    from fdgs import depth, synth
    cam = synth.camera_for(pose, W, H)
    cam["intr"] = tuple(float(np.float32(v)) for v in depth.intrinsics_of(cam))
    return cam


def make_view(pose, W, H, seed, weight=1.0, alpha=True, mask=True, rgb=True, alpha_min=0.5):
    """A smooth depth surface through the volume's centre as this camera sees it (the centre's view depth, or 0.6 for a camera
    near it), alpha on both sides of alpha_min and the depth premultiplied by it, a mask with holes, a random image."""
    cam = camera(pose, W, H)
    rng = np.random.default_rng(seed)
    vm = cam["world_view_transform"].numpy().astype(np.float32)
    zc = float(vm[3, 2])
    zc = zc if zc > 1.0 else 0.6
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    z = zc + 0.15 * np.sin(0.31 * u + rng.uniform(0, 6)) + 0.1 * np.cos(0.43 * v + rng.uniform(0, 6)) + 0.02 * rng.standard_normal((H, W))
    a = np.clip(rng.uniform(0.3, 1.3, (H, W)), 0.0, 1.0).astype(np.float32) if alpha else None
    d = (z * a if alpha else z).astype(np.float32)
    if H * W > 4:
        d.flat[1], d.flat[2] = 0.0, np.inf                      # a hole and a bad depth: zp is not positive and finite
    return {"depth": d, "alpha": a, "mask": (rng.uniform(0, 1, (H, W)) > 0.1).astype(np.float32) if mask else None,
            "image": rng.uniform(0, 1, (3, H, W)).astype(np.float32) if rgb else None, "vm": vm, "intr": cam["intr"],
            "alpha_min": alpha_min, "weight": weight, "camera": cam}


@functools.lru_cache(maxsize=None)
def integrate_case(name):
    """(fresh volume, views) of INTEGRATE_CASES[name]."""
    c = INTEGRATE_CASES[name]
    W, H = c["image"]
    seed0 = 1000 * (1 + sorted(INTEGRATE_CASES).index(name))
    views = [make_view(p, W, H, seed0 + n, c["weights"][n], c["alpha"], c["mask"], c["rgb"]) for n, p in enumerate(c["poses"])]
    return fresh_volume(c["dims"], c["s"], c["color"]), views


@functools.lru_cache(maxsize=None)
def integrate_refs(name):
    """The float64 truth and the float32 statement of a case; computed once, shared, read-only."""
    import surface_oracle as so
    vol, views = integrate_case(name)
    return so.integrate(vol, views, np.float64), so.integrate(vol, views, np.float32)


# ---- the analytic plane z = PLANE_Z seen by three unrotated cameras in front of it: every depth map is a constant, so the projective
# distance of a seen voxel is its exact signed distance to the plane
PLANE_Z, PLANE_DIMS, PLANE_S = 0.013, (16, 16, 16), 0.08
PLANE_SHIFTS = [(0.0, 0.0, 0.0), (0.3, -0.2, 0.5), (-0.25, 0.15, -0.4)]


@functools.lru_cache(maxsize=None)
def plane_case():
    W, H = 40, 24
    views = []
    for n, shift in enumerate(PLANE_SHIFTS):
        cam = camera(dict(shift=shift), W, H)
        depth = np.full((H, W), PLANE_Z - (-4.0 + shift[2]), np.float32)
        views.append({"depth": depth, "alpha": None, "mask": None, "image": np.full((3, H, W), 0.25 * (n + 1), np.float32),
                      "vm": cam["world_view_transform"].numpy().astype(np.float32), "intr": cam["intr"], "alpha_min": 0.5, "weight": 1.0,
                      "camera": cam})
    return fresh_volume(PLANE_DIMS, PLANE_S), views


# ---- float32 volumes for the extraction ----
EXTRACT_SHAPES = [(17, 9, 33), (2, 2, 2), (5, 1, 4)]
EXTRACT_KINDS = ["sphere", "plane_slab", "random", "min_weight"]
# past a scan chunk (1024 workgroup counts = 262 144 voxels; the shapes above are a few thousand voxels, a few workgroups): GPU tests only
CHUNK_SHAPE, CHUNK_KINDS = (65, 64, 64), ["sphere", "random"]
SPHERE_CENTRE, SPHERE_RADIUS = (0.37, 0.22, 0.41), 3.1       # offset from the volume's centre and radius, in voxels


def _centres(vol):
    nx, ny, nz = vol["dims"]
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return [vol["origin"][c] + (idx + 0.5) * vol["s"] for c, idx in enumerate((i, j, k))]


def sphere_centre(vol):
    return tuple(SPHERE_CENTRE[c] * vol["s"] for c in range(3))


@functools.lru_cache(maxsize=None)
def extract_case(kind, dims):
    """(volume, min_weight): every array float32, exactly what the kernels and both runs of the statement receive."""
    s = 0.05
    vol = fresh_volume(dims, s)
    rng = np.random.default_rng(7 + 13 * EXTRACT_KINDS.index(kind) + sum(dims))
    x, y, z = _centres(vol)
    shape = vol["tsdf"].shape
    vol["color"] = rng.uniform(0, 1, (3,) + shape).astype(np.float32)
    vol["cweight"] = np.ones(shape, np.float32)
    vol["weight"] = np.ones(shape, np.float32)
    min_weight = 1.0
    if kind == "sphere":
        c = sphere_centre(vol)
        vol["tsdf"] = ((np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - SPHERE_RADIUS * s) / vol["trunc"]).astype(np.float32)
    elif kind == "plane_slab":
        vol["tsdf"] = np.clip((0.35 * x - 0.2 * y + 0.9 * z - 0.011) / vol["trunc"], -1, 1).astype(np.float32)
        vol["weight"][:, :, shape[2] // 2] = 0.0            # an unknown slab through the plane
        vol["weight"][shape[0] // 3] = 0.0
    else:
        f = np.sin(9.0 * x + 1.0) + np.cos(7.0 * y - 0.5) * np.sin(8.0 * z + 0.3) + 0.2 * rng.standard_normal(shape)
        vol["tsdf"] = np.clip(0.5 * f, -1, 1).astype(np.float32)
        if kind == "random":
            vol["weight"] = (rng.uniform(0, 1, shape) > 0.03).astype(np.float32) * rng.choice([1.0, 2.5], shape).astype(np.float32)
        else:
            vol["weight"] = rng.choice([0.5, 1.0, 2.0, 3.0], shape, p=[0.02, 0.02, 0.48, 0.48]).astype(np.float32)
            min_weight = 1.5
    return vol, min_weight


@functools.lru_cache(maxsize=None)
def extract_refs(kind, dims):
    import surface_oracle as so
    vol, mw = extract_case(kind, dims)
    return so.extract(vol, mw, np.float64), so.extract(vol, mw, np.float32)
