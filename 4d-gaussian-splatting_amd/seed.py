"""Point clouds a run starts from (csrc/seed.hip, include/fdgs_seed.h): thinning, random clouds, the initial model.

What the reference does on the host between reading ``points3d.ply`` and iteration 0 -- ``np.random.randint`` over the cloud (it
draws with replacement: duplicates, and another cloud every run; scene/dataset_readers.py:339-355), ``np.random`` clouds (:329-331,
:357-371) and ``GaussianModel.create_from_pcd`` (scene/gaussian_model.py:259-300) -- as three HIP entry points whose results are pure
functions of their inputs, bit for bit:

* ``thin(cloud, cell, cell_t)``  -- one point per occupied cell of a grid in (x, y, z, t): the float32 mean of the cell's members.
* ``thin_to(cloud, num_pts)``    -- the finest grid of a fixed ladder of 65536 cell sizes that leaves at most ``num_pts`` points.
* ``random_cloud`` / ``sphere_shell`` -- Philox4x32-10 draws: the reference's random initial cloud and its ``num_extra_pts`` shell.
* ``create_from_pcd(cloud, ...)`` -- the ``GaussianParams`` a run starts from, written into the flat bucket by one launch.
* ``load_ply`` / ``save_ply``    -- point-cloud PLY files (x y z, red green blue, optional normals, optional ``time``), host code.

There is no CPU path for the first four."""
import math
from collections import namedtuple
from typing import Optional, Sequence

import numpy as np
import torch

from . import _capi, _seed_capi, layout
from .checkpoint import reference_sh_channels
from .knn import distCUDA2
from .train_host import GaussianParams

C0 = 0.28209479177387814                      # utils/sh_utils.py:24
AXIS_CELLS = _seed_capi.SEED_AXIS_CELLS       # cells a cloud may span along one axis: 16 bits of the sort key each
LADDER = 65536                                # thin_to's cell sizes: 2 * extent * k / LADDER, k = 1 .. LADDER (16 bisection steps)
_ONE_CELL = 2.0 ** -100                       # the inverse cell size of an axis that is not cut


class PointCloud:
    """``xyz`` float32 [N, 3], ``rgb`` float32 [N, 3] in [0, 1], ``t`` float32 [N] or None (the reference's BasicPointCloud without
    its normals, as tensors)."""

    def __init__(self, xyz: torch.Tensor, rgb: torch.Tensor, t: Optional[torch.Tensor] = None):
        xyz, rgb = torch.as_tensor(xyz), torch.as_tensor(rgb)
        if xyz.dim() != 2 or xyz.shape[1] != 3 or tuple(rgb.shape) != tuple(xyz.shape):
            raise ValueError("fdgs.seed: xyz and rgb must both be [N, 3], got %s and %s" % (tuple(xyz.shape), tuple(rgb.shape)))
        self.xyz, self.rgb = xyz.detach().float().contiguous(), rgb.detach().float().contiguous()
        self.t = None
        if t is not None:
            t = torch.as_tensor(t).detach().float().reshape(-1).contiguous()
            if t.shape[0] != xyz.shape[0]:
                raise ValueError("fdgs.seed: t must hold one time per point (%d), got %d" % (xyz.shape[0], t.shape[0]))
            if t.device != self.xyz.device:
                raise ValueError("fdgs.seed: t lives on %s, xyz on %s" % (t.device, self.xyz.device))
            self.t = t
        if self.rgb.device != self.xyz.device:
            raise ValueError("fdgs.seed: rgb lives on %s, xyz on %s" % (self.rgb.device, self.xyz.device))

    def __len__(self):
        return int(self.xyz.shape[0])

    device = property(lambda s: s.xyz.device)

    def to(self, device) -> "PointCloud":
        return PointCloud(self.xyz.to(device), self.rgb.to(device), None if self.t is None else self.t.to(device))

    def select(self, mask) -> "PointCloud":
        return PointCloud(self.xyz[mask], self.rgb[mask], None if self.t is None else self.t[mask])

    @staticmethod
    def cat(clouds: Sequence["PointCloud"]) -> "PointCloud":
        timed = [c.t is not None for c in clouds]
        if any(timed) and not all(timed):
            raise ValueError("fdgs.seed: clouds with and without times cannot be joined")
        return PointCloud(torch.cat([c.xyz for c in clouds]), torch.cat([c.rgb for c in clouds]),
                          torch.cat([c.t for c in clouds]) if all(timed) and clouds else None)


# cloud: the thinned PointCloud.  key: int64 [M] the cells' sort keys (the bit pattern of (ix << 48) | (iy << 32) | (iz << 16) | it),
# ascending as unsigned numbers.  count: int32 [M] members.  first: int32 [M] the smallest index of a member.  cell, cell_t: the grid.
Thinned = namedtuple("Thinned", "cloud key count first cell cell_t")


def _extent(cloud):
    """(origin [4], maxima [4]) of the cloud as float32 numpy; the time entries are 0 without times."""
    lo, hi = np.zeros(4, np.float32), np.zeros(4, np.float32)
    if len(cloud):
        lo[:3], hi[:3] = cloud.xyz.amin(0).cpu().numpy(), cloud.xyz.amax(0).cpu().numpy()
        if cloud.t is not None:
            lo[3], hi[3] = float(cloud.t.amin()), float(cloud.t.amax())
    return lo, hi


def _grid(cloud, cell, cell_t):
    """The float32 grid ``fdgs_seed_thin`` takes -- origin = the cloud's minimum, inv_cell = 1 / cell rounded once -- after the checks
    that need no GPU: the sizes, finite coordinates, at most AXIS_CELLS cells along every axis."""
    cell = float(cell)
    if not (cell > 0.0 and math.isfinite(cell)):
        raise ValueError("fdgs.seed: cell must be positive and finite, got %r" % (cell,))
    if cell_t is not None and not (float(cell_t) > 0.0 and math.isfinite(float(cell_t))):
        raise ValueError("fdgs.seed: cell_t must be positive and finite, got %r" % (cell_t,))
    lo, hi = _extent(cloud)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError("fdgs.seed: the cloud has coordinates that are not finite")
    with np.errstate(over="ignore", divide="ignore"):
        inv_s = np.float32(1.0) / np.float32(cell)
        inv_t = np.float32(_ONE_CELL) if cell_t is None or cloud.t is None else np.float32(1.0) / np.float32(cell_t)
        inv = np.array([inv_s, inv_s, inv_s, inv_t], np.float32)
        top = np.floor((hi - lo) * inv)                    # float32, the kernel's own expression: the largest index of every axis
    if not (np.isfinite(inv).all() and (inv > 0).all()):
        raise ValueError("fdgs.seed: cell sizes %r / %r have no float32 inverse" % (cell, cell_t))
    if not (top < AXIS_CELLS).all():
        raise ValueError("fdgs.seed: the cloud spans %s cells along (x, y, z, t); the sort key holds %d per axis -- use a larger cell"
                         % ([int(min(v, 2.0 ** 62)) if math.isfinite(v) else v for v in top.tolist()], AXIS_CELLS))
    return lo, inv


def _launch_thin(cloud, lo, inv, count_only, scratch, n_cells):
    N, dev = len(cloud), cloud.device
    ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    outs = [None] * 6
    if not count_only:
        outs = [torch.empty(N, dtype=torch.int64, device=dev), torch.empty((N, 3), dtype=torch.float32, device=dev),
                torch.empty((N, 3), dtype=torch.float32, device=dev), None if cloud.t is None else torch.empty(N, dtype=torch.float32, device=dev),
                torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)]
    _seed_capi.call("fdgs_seed_thin", dev, N, ptr(cloud.xyz) if N else None, ptr(cloud.rgb) if N else None, ptr(cloud.t) if N else None,
                    _seed_capi.host_floats(lo, 4), _seed_capi.host_floats(inv, 4), int(count_only), 0 if count_only else N,
                    *[ptr(o) if N else None for o in outs], n_cells.data_ptr(), scratch.data_ptr(), arg_error=ValueError)
    return outs


def _thin_scratch(cloud):
    dev = cloud.device
    return _capi.scratch(_seed_capi.lib.fdgs_seed_thin_scratch_bytes(len(cloud)), dev, floor=256), torch.zeros(1, dtype=torch.int32, device=dev)


def thin(cloud: PointCloud, cell: float, cell_t: Optional[float] = None) -> Thinned:
    """One point per occupied cell of the grid with spatial cell size ``cell`` and time cell size ``cell_t`` (None, or a cloud
    without times: time is not cut), anchored at the cloud's minimum.  A coordinate v falls into cell
    ``floor((v - origin) * inv_cell)`` with ``inv_cell = float32(1) / float32(cell)``, every operation in float32.  The result is
    ordered by cell key; position, colour and time are the float32 means of the cell's members, summed in ascending point index
    and divided by the count.  Deterministic: two calls give the same bits.  ``ValueError``: a cloud that spans more than
    ``AXIS_CELLS`` = 65536 cells along an axis (the sort key holds 16 bits per axis), non-finite coordinates, a cell size that is
    not positive and finite."""
    lo, inv = _grid(cloud, cell, cell_t)
    _capi.need_gpu(cloud.xyz, "cloud.xyz")
    scratch, n_cells = _thin_scratch(cloud)
    key, xyz, rgb, t, count, first = _launch_thin(cloud, lo, inv, False, scratch, n_cells)
    M = int(n_cells.item())
    return Thinned(PointCloud(xyz[:M], rgb[:M], None if t is None else t[:M]), key[:M], count[:M], first[:M], float(cell),
                   None if cell_t is None or cloud.t is None else float(cell_t))


def count_cells(cloud: PointCloud, cell: float, cell_t: Optional[float] = None) -> int:
    """``len(thin(cloud, cell, cell_t).cloud)`` without building it (the ``count_only`` mode)."""
    lo, inv = _grid(cloud, cell, cell_t)
    _capi.need_gpu(cloud.xyz, "cloud.xyz")
    scratch, n_cells = _thin_scratch(cloud)
    _launch_thin(cloud, lo, inv, True, scratch, n_cells)
    return int(n_cells.item())


def ladder_cell(cloud: PointCloud, k: int):
    """Rung ``k`` (1 .. LADDER) of ``thin_to``'s ladder for this cloud: ``(cell, cell_t)`` = 2 * extent * k / LADDER with the largest
    spatial extent and the time extent (``cell_t`` None without times or with one time only).  Rung LADDER puts the whole cloud into
    one cell; rung 1 cuts the longest axis into 32768."""
    lo, hi = _extent(cloud)
    ext = float((hi[:3].astype(np.float64) - lo[:3]).max()) or 1.0
    ext_t = float(hi[3]) - float(lo[3])
    return 2.0 * ext * k / LADDER, (2.0 * ext_t * k / LADDER if ext_t > 0.0 else None)


def thin_to(cloud: PointCloud, num_pts: int) -> Thinned:
    """The cloud thinned to at most ``num_pts`` points: bisection over the LADDER rungs of ``ladder_cell`` with 16 ``count_only``
    launches, then ``thin`` at the finest rung found whose count is <= ``num_pts`` (the rung below it was counted and exceeds it).
    Space and time are cut in proportion to their extents.  A cloud that already has at most ``num_pts`` points comes back
    unchanged (key None, count 1, first = the index).  ``ValueError``: ``num_pts`` < 1."""
    num_pts = int(num_pts)
    if num_pts < 1:
        raise ValueError("fdgs.seed: num_pts must be at least 1, got %d" % num_pts)
    _grid(cloud, *ladder_cell(cloud, LADDER))           # the finite-coordinates check
    _capi.need_gpu(cloud.xyz, "cloud.xyz")
    N, dev = len(cloud), cloud.device
    if N <= num_pts:
        return Thinned(cloud, None, torch.ones(N, dtype=torch.int32, device=dev), torch.arange(N, dtype=torch.int32, device=dev), None, None)
    scratch, n_cells = _thin_scratch(cloud)
    lo_k, hi_k = 0, LADDER                             # rung LADDER: one cell
    while hi_k - lo_k > 1:
        mid = (lo_k + hi_k) // 2
        lo, inv = _grid(cloud, *ladder_cell(cloud, mid))
        _launch_thin(cloud, lo, inv, True, scratch, n_cells)
        if int(n_cells.item()) <= num_pts:
            hi_k = mid
        else:
            lo_k = mid
    return thin(cloud, *ladder_cell(cloud, hi_k))


def ladder_rung(cloud: PointCloud, cell: float) -> int:
    """The rung of ``ladder_cell`` whose spatial cell is ``cell`` (what ``thin_to`` returned in ``Thinned.cell``)."""
    return int(round(cell / ladder_cell(cloud, 1)[0]))


def _random(N, seed, stream_id, shape, params, device, width, debug=False):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("fdgs.seed: random clouds are drawn on the GPU; there is no CPU path (got %s)" % dev)
    N = int(N)
    if N < 0:
        raise ValueError("fdgs.seed: the number of points must not be negative, got %d" % N)
    out = torch.empty((N, 3) if width == 3 else (N,), dtype=torch.float32, device=dev)
    words = torch.empty((N, 4), dtype=torch.int32, device=dev) if debug else None
    uniforms = torch.empty((N, 4), dtype=torch.float32, device=dev) if debug else None
    ptr = lambda x: None if x is None or N == 0 else x.data_ptr()  # noqa: E731
    _seed_capi.call("fdgs_seed_random", dev, N, int(seed) & (2 ** 64 - 1), int(stream_id), shape, _seed_capi.host_floats(params, 6), ptr(out),
                    ptr(words), ptr(uniforms), arg_error=ValueError)
    return (out, words, uniforms) if debug else out


def random_box(N, seed, lo, extent, device, stream_id=0, debug=False):
    """float32 [N, 3]: ``u * extent + lo`` per axis with Philox4x32-10 uniforms (key = the 64-bit ``seed``, counter = (point index,
    ``stream_id``, 0, 0), u = (word >> 8) * 2^-24).  ``debug``: also the raw words (int32 bit patterns [N, 4]) and uniforms [N, 4]."""
    lo3, ext3 = (np.broadcast_to(np.asarray(v, np.float32), (3,)).tolist() for v in (lo, extent))
    return _random(N, seed, stream_id, _seed_capi.SEED_BOX, lo3 + ext3, device, 3, debug)


def random_sphere(N, seed, radius, device, stream_id=0, debug=False):
    """float32 [N, 3] uniform on the sphere of ``radius`` around the origin (same generator)."""
    return _random(N, seed, stream_id, _seed_capi.SEED_SPHERE, [radius], device, 3, debug)


def random_times(N, seed, time_duration, device, stream_id=2):
    """float32 [N]: ``(u * 1.2 - 0.1) * (t1 - t0) + t0``, the times ``create_from_pcd`` gives a cloud that has none
    (scene/gaussian_model.py:268); t1 - t0 is taken in float32."""
    t0, t1 = np.float32(time_duration[0]), np.float32(time_duration[1])
    return _random(N, seed, stream_id, _seed_capi.SEED_TIME, [t0, t1 - t0], device, 1)


def random_cloud(num_pts: int, seed: int = 0, lo: float = -1.3, extent: float = 2.6, device="cuda") -> PointCloud:
    """The reference's cloud for a scene without one (scene/dataset_readers.py:329-331): ``num_pts`` positions uniform in the box
    [lo, lo + extent)^3 and colours ``SH2RGB(u / 255)`` = u * (C0 / 255) + 0.5, from streams 0 and 1 of ``seed``."""
    return PointCloud(random_box(num_pts, seed, lo, extent, device, stream_id=0),
                      random_box(num_pts, seed, 0.5, float(np.float32(C0) / np.float32(255.0)), device, stream_id=1))


def sphere_shell(num_pts: int, radius: float = 60.0, seed: int = 0, device="cuda", time: Optional[float] = None) -> PointCloud:
    """The reference's ``num_extra_pts`` shell (scene/dataset_readers.py:357-384): ``num_pts`` grey points uniform on the sphere of
    ``radius``, all at ``time`` if given (the middle of the time span there)."""
    xyz = random_sphere(num_pts, seed, radius, device, stream_id=3)
    return PointCloud(xyz, torch.full_like(xyz, 0.5), None if time is None else torch.full((int(num_pts),), float(time), device=xyz.device))


def init_constants(time_duration):
    """(inverse_sigmoid(0.1), log(sqrt((t1 - t0) / 5))) in float32, one rounding per operation, as the reference's PyTorch lines
    compute them (scene/gaussian_model.py:280-286)."""
    x = np.float32(0.1)
    with np.errstate(divide="ignore", invalid="ignore"):
        opacity = np.log(x / (np.float32(1.0) - x))
        span = (np.float32(time_duration[1]) - np.float32(time_duration[0])) / np.float32(5.0)
        scaling_t = np.log(np.sqrt(span))
    return float(np.float32(opacity)), float(np.float32(scaling_t))


def create_from_pcd(cloud: PointCloud, *, sh_degree: int, sh_degree_t: int = 0, gaussian_dim: int = 3, rot_4d: bool = False,
                    force_sh_3d: bool = False, time_duration=(0.0, 1.0), seed: int = 0, dist2: Optional[torch.Tensor] = None,
                    M: Optional[int] = None, prefilter_var: float = -1.0) -> GaussianParams:
    """``GaussianModel.create_from_pcd`` (scene/gaussian_model.py:259-300) in one launch: the model a run starts from, active degrees
    (0, 0).  ``dist2``: ``distCUDA2(cloud.xyz)`` (computed here if None).  A 4D model of a cloud without times draws them with
    ``random_times(seed)``.  ``M``: the coefficients per Gaussian (default: the reference's ``get_max_sh_channels``).  Segments the
    mode does not read hold ``layout.placeholder_``'s values."""
    _capi.need_gpu(cloud.xyz, "cloud.xyz")
    P, dev = len(cloud), cloud.device
    gaussian_dim = int(gaussian_dim)
    if gaussian_dim not in (3, 4):
        raise ValueError("fdgs.seed: gaussian_dim must be 3 or 4, got %r" % (gaussian_dim,))
    M = reference_sh_channels(int(sh_degree), int(sh_degree_t), gaussian_dim, bool(force_sh_3d)) if M is None else int(M)
    if dist2 is None:
        dist2 = distCUDA2(cloud.xyz)
    dist2 = _capi._dev_f32(dist2, "dist2") if P else dist2
    if P and (dist2.dim() != 1 or dist2.shape[0] != P or dist2.device != dev):
        raise ValueError("fdgs.seed: dist2 must be [%d] on %s, got %s on %s" % (P, dev, tuple(dist2.shape), dist2.device))
    t = cloud.t
    if gaussian_dim == 4 and t is None:
        t = random_times(P, seed, time_duration, dev)
    opacity_raw, scaling_t_raw = init_constants(time_duration)
    model = GaussianParams.empty(P, M, dev)
    assert [s.kernel for s in layout.SEGMENTS] == ["means3D", "opacities", "scales", "rotations", "ts", "scales_t", "rotations_r", "shs"] \
        and layout.row_floats(M) == [3, 1, 3, 4, 1, 1, 4, 3 * M]   # the order fdgs_seed_init writes
    ptr = lambda x: None if x is None or P == 0 else x.data_ptr()  # noqa: E731
    _seed_capi.call("fdgs_seed_init", dev, P, M, gaussian_dim, ptr(cloud.xyz), ptr(cloud.rgb), ptr(t) if gaussian_dim == 4 else None, ptr(dist2),
                    opacity_raw, scaling_t_raw, ptr(model.flat), arg_error=ValueError)
    return model.apply_settings(max_sh_degree=int(sh_degree), max_sh_degree_t=int(sh_degree_t), active_sh_degree=0, active_sh_degree_t=0,
                                time_duration=(float(time_duration[0]), float(time_duration[1])), rot_4d=bool(rot_4d), gaussian_dim=gaussian_dim,
                                force_sh_3d=bool(force_sh_3d), prefilter_var=prefilter_var)


# ---- PLY ------------------------------------------------------------------------------------------------------------------------------
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply_vertices(path: str) -> dict:
    """The vertex element of a PLY file (ascii or binary_little_endian) as {property: numpy array}; list properties and elements in
    front of the vertices are not supported (point clouds have neither)."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError("fdgs.seed: %s is not a PLY file" % path)
        fmt, count, props, in_vertex, first = None, None, [], False, None
        while True:
            line = f.readline()
            if not line:
                raise ValueError("fdgs.seed: %s: the header does not end" % path)
            w = line.decode("ascii", "replace").split()
            if not w or w[0] in ("comment", "obj_info"):
                continue
            if w[0] == "format":
                fmt = w[1]
            elif w[0] == "element":
                first = w[1] if first is None else first
                in_vertex = w[1] == "vertex"
                if in_vertex:
                    if first != "vertex":
                        raise ValueError("fdgs.seed: %s: the vertex element must come first" % path)
                    count = int(w[2])
            elif w[0] == "property" and in_vertex:
                if w[1] == "list" or w[1] not in _PLY_TYPES:
                    raise ValueError("fdgs.seed: %s: unsupported vertex property %r" % (path, " ".join(w[1:])))
                props.append((w[2], _PLY_TYPES[w[1]]))
            elif w[0] == "end_header":
                break
        if count is None or fmt not in ("ascii", "binary_little_endian"):
            raise ValueError("fdgs.seed: %s: need a vertex element in ascii or binary_little_endian format (format: %r)" % (path, fmt))
        if fmt == "ascii":
            rows = np.loadtxt(f, dtype=np.float64, max_rows=count, ndmin=2) if count else np.zeros((0, len(props)))
            if rows.shape != (count, len(props)):
                raise ValueError("fdgs.seed: %s: expected %d rows of %d numbers, got %s" % (path, count, len(props), rows.shape))
            return {name: rows[:, k].astype(np.dtype(ty)) for k, (name, ty) in enumerate(props)}
        dt = np.dtype([(name, "<" + ty) for name, ty in props])
        data = np.frombuffer(f.read(count * dt.itemsize), dtype=dt)
        if data.shape[0] != count:
            raise ValueError("fdgs.seed: %s: the file ends after %d of %d vertices" % (path, data.shape[0], count))
        return {name: np.ascontiguousarray(data[name]) for name, _ in props}


def load_ply(path: str, device="cpu") -> PointCloud:
    """``fetchPly`` (scene/dataset_readers.py:118-131): positions ``x y z``, colours ``red green blue`` / 255, the ``time`` column if
    there is one; normals are skipped.  Read by this module's own parser (no plyfile)."""
    v = read_ply_vertices(path)
    for name in ("x", "y", "z", "red", "green", "blue"):
        if name not in v:
            raise ValueError("fdgs.seed: %s has no vertex property %r" % (path, name))
    xyz = np.stack([v["x"], v["y"], v["z"]], axis=1).astype(np.float32)
    rgb = (np.stack([v["red"], v["green"], v["blue"]], axis=1) / 255.0).astype(np.float32)
    t = torch.from_numpy(v["time"].astype(np.float32)) if "time" in v else None
    return PointCloud(torch.from_numpy(xyz), torch.from_numpy(rgb), t).to(device)


def save_ply(path: str, cloud: PointCloud, binary: bool = True, normals: bool = True):
    """``storePly`` (scene/dataset_readers.py:133-148) plus the ``time`` column of a timed cloud: float32 positions, zero normals
    (``normals``), uint8 colours (``rgb * 255`` cut to [0, 255] and truncated, as a cast to uint8 does), float32 ``time``."""
    xyz = cloud.xyz.detach().cpu().numpy().astype(np.float32)
    rgb = np.clip(cloud.rgb.detach().cpu().numpy().astype(np.float64) * 255.0, 0.0, 255.0).astype(np.uint8)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")] if normals else []) + \
             [("red", "u1"), ("green", "u1"), ("blue", "u1")] + ([("time", "<f4")] if cloud.t is not None else [])
    rows = np.zeros(len(cloud), dtype=np.dtype(fields))
    rows["x"], rows["y"], rows["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    rows["red"], rows["green"], rows["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    if cloud.t is not None:
        rows["time"] = cloud.t.detach().cpu().numpy().astype(np.float32)
    names = {"<f4": "float", "u1": "uchar"}
    header = ["ply", "format %s 1.0" % ("binary_little_endian" if binary else "ascii"), "element vertex %d" % len(cloud)]
    header += ["property %s %s" % (names[ty], name) for name, ty in fields] + ["end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        if binary:
            f.write(rows.tobytes())
        else:
            for r in rows:
                f.write((" ".join(repr(float(r[name])) if ty == "<f4" else str(int(r[name])) for name, ty in fields) + "\n").encode("ascii"))
