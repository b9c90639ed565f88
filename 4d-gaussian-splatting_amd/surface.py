"""A coloured surface from a trained model, on the GPU (csrc/tsdf.hip): TSDF fusion of rendered depth maps and surface nets.

* ``TSDFVolume(origin, voxel_size, dims)`` -- ``nx x ny x nz`` voxels of edge ``s``; voxel (i, j, k) has its centre at
  ``origin + (i + .5, j + .5, k + .5) s``.  float32 tensors, x fastest: ``tsdf`` and ``weight`` [nz, ny, nx], optionally ``color``
  [3, nz, ny, nx] and ``cweight`` [nz, ny, nx].  All zeros when fresh (``weight = 0``: never seen); ``reset()`` zeroes it.
* ``integrate(volume, views)`` -- every view (``depth``, ``alpha``, ``image``, ``mask``, ``camera``, ``weight``) is applied to every
  voxel centre in order: project with ``fdgs.depth.intrinsics_of(camera)``, keep the pixel under ``fdgs.depth``'s validity rule
  (``alpha >= alpha_min``, ``mask > 0``, ``zp = depth / alpha`` finite and positive), ``sdf = zp - z``, skip below ``-trunc``,
  ``d = min(1, sdf / trunc)``, a running weighted mean of ``d`` -- and of the pixel's colour where ``d < 1``.  One launch per 16 views
  with the voxel in registers; bit-identical to one call per view.  ``tsdf`` is in units of ``trunc``.
* ``fuse(model, cameras, pipe, bg, volume)`` renders the cameras with ``render()`` and integrates them; ``extract(volume)`` is the
  mesh: one vertex per cell the surface crosses (surface nets: no case tables, quads between the four cells around every
  sign-changing grid edge, vertices shared by construction), with normals from the distance gradient and colours from the volume.
* ``prepare_views`` does the host side of ``integrate`` once (tensor checks, view matrices on the device, intrinsics) for callers that
  integrate the same buffers repeatedly.  ``fuse_sequence`` yields one mesh per timestamp; ``save_mesh_ply`` / ``load_mesh_ply`` write and read it.
* ``components(mesh)``, ``clean(mesh, keep_largest=, min_faces=)`` and ``smooth(mesh)`` (csrc/mesh.hip) finish a raw mesh on the
  device: connected components, dropping floaters with order-preserving compaction, Taubin smoothing with recomputed normals.  A face
  with an index outside ``[0, V)`` is absent to all three.
* ``simplify(mesh, cell)`` (csrc/mesh_simplify.hip) makes the mesh small enough to use: vertex clustering on a grid of edge ``cell``
  with quadric placement; ``cell_for_target(mesh, faces)`` finds a cell size for a face budget.

Everything runs on the current stream; ``extract`` reads two counters from the device once, to size its outputs.  No atomics: two
runs are bit-identical.  There is no CPU path.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _capi
from .depth import intrinsics_of


class TSDFVolume:
    def __init__(self, origin, voxel_size, dims, trunc=None, color=True, device="cuda"):
        self.origin = tuple(float(v) for v in origin)
        self.voxel_size = float(voxel_size)
        self.dims = tuple(int(v) for v in dims)          # (nx, ny, nz)
        self.trunc = 4.0 * self.voxel_size if trunc is None else float(trunc)
        if torch.device(device).type != "cuda":
            raise RuntimeError("fdgs: a TSDFVolume lives on the GPU (got %s); there is no CPU path" % (device,))
        if len(self.origin) != 3 or len(self.dims) != 3 or min(self.dims) < 0:
            raise ValueError("fdgs: TSDFVolume needs origin (x, y, z) and dims (nx, ny, nz) >= 0; got %s, %s" % (origin, dims))
        nx, ny, nz = self.dims
        self.tsdf = torch.zeros((nz, ny, nx), dtype=torch.float32, device=device)
        self.device = self.tsdf.device                   # with its index ("cuda" -> the current device), as every tensor reports it
        self.weight = torch.zeros_like(self.tsdf)
        self.color = torch.zeros((3, nz, ny, nx), dtype=torch.float32, device=self.device) if color else None
        self.cweight = torch.zeros_like(self.tsdf) if color else None

    def reset(self):
        for t in (self.tsdf, self.weight, self.color, self.cweight):
            if t is not None:
                t.zero_()

    def arrays(self):
        return {"tsdf": self.tsdf, "weight": self.weight, "color": self.color, "cweight": self.cweight}

    @property
    def voxels(self) -> int:
        return self.dims[0] * self.dims[1] * self.dims[2]

    def _struct(self):
        return _capi.FdgsTsdfVolume(*self.dims, *self.origin, self.voxel_size, self.trunc, _capi._ptr(self.tsdf), _capi._ptr(self.weight),
                                    _capi._ptr(self.color), _capi._ptr(self.cweight))


def _field(view, key, default=None):
    v = view.get(key, default) if isinstance(view, dict) else getattr(view, key, default)
    return default if v is None else v


def _image(t, name, dev, shape=None):
    if t is None:
        return None
    _capi.need_gpu(t, name)
    if t.device != dev:
        raise RuntimeError("fdgs: '%s' lives on %s, the volume on %s" % (name, t.device, dev))
    t = t.detach().contiguous().float()
    if shape is not None and (t.numel() != shape[0] * shape[1] or tuple(t.shape[-2:]) != shape):
        raise ValueError("fdgs: '%s' must have the depth's [1, H, W] shape %s; got %s" % (name, shape, tuple(t.shape)))
    return t


class PreparedViews:
    """Views as ``fdgs_tsdf_integrate`` takes them: the array of structs and the tensors its pointers refer to."""

    def __init__(self, structs, count, device, tensors):
        self.structs, self.count, self.device, self.tensors = structs, count, device, tensors

    def __len__(self):
        return self.count


def prepare_views(views, device) -> PreparedViews:
    """The host side of ``integrate``, once: checks the tensors, puts every view matrix on ``device`` and reads the intrinsics --
    a view's own ``intrinsics`` = (fl_x, fl_y, cx, cy) where it carries them, else ``fdgs.depth.intrinsics_of(camera)`` (a host read
    of two matrices).  ``integrate(volume, prepared)`` is then the C call alone; the views' tensors may be rewritten in place between
    calls (a render into the same buffers)."""
    views = list(views)
    dev = torch.device(device)
    keep, structs = [], (_capi.FdgsTsdfView * max(len(views), 1))()
    for n, view in enumerate(views):
        d = _field(view, "depth")
        if d is None:
            raise ValueError("fdgs: view %d has no depth" % n)
        d = _image(d, "depth", dev)
        if d.dim() < 2 or d.numel() != d.shape[-2] * d.shape[-1]:
            raise ValueError("fdgs: depth must be one [1, H, W] image; got %s" % (tuple(d.shape),))
        shape = (int(d.shape[-2]), int(d.shape[-1]))
        a, m = _image(_field(view, "alpha"), "alpha", dev, shape), _image(_field(view, "mask"), "mask", dev, shape)
        img = _image(_field(view, "image"), "image", dev)
        if img is not None and tuple(img.shape) != (3,) + shape:
            raise ValueError("fdgs: image must be [3, H, W] = %s; got %s" % ((3,) + shape, tuple(img.shape)))
        cam = _field(view, "camera")
        if cam is None:
            raise ValueError("fdgs: view %d has no camera" % n)
        get = (lambda k: cam.get(k)) if isinstance(cam, dict) else (lambda k: getattr(cam, k, None))
        vm = get("world_view_transform")
        if vm is None:
            raise ValueError("fdgs: the camera of view %d has no world_view_transform" % n)
        vm = vm.detach().to(dev, torch.float32).contiguous()
        intr = _field(view, "intrinsics")
        fx, fy, cx, cy = (float(v) for v in intr) if intr is not None else intrinsics_of(cam)
        keep.append((d, a, m, img, vm))
        structs[n] = _capi.FdgsTsdfView(shape[0], shape[1], d.data_ptr(), _capi._ptr(a), _capi._ptr(m), _capi._ptr(img), vm.data_ptr(),
                                        float(_field(view, "alpha_min", 0.5)), fx, fy, cx, cy, float(_field(view, "weight", 1.0)))
    return PreparedViews(structs, len(views), dev, keep)


def integrate(volume: TSDFVolume, views) -> None:
    """Fuses ``views`` -- dicts or objects with ``depth`` [1, H, W], ``camera`` and optionally ``alpha``, ``mask`` (both [1, H, W]),
    ``image`` [3, H, W], ``weight`` (1.0), ``alpha_min`` (0.5) and ``intrinsics``, or a ``PreparedViews`` -- into ``volume``, in
    order, in one call."""
    dev = volume.device
    if not isinstance(views, PreparedViews):
        views = prepare_views(views, dev)
    elif views.device != dev:
        raise RuntimeError("fdgs: the views were prepared for %s, the volume lives on %s" % (views.device, dev))
    if volume.voxels == 0 or len(views) == 0:
        return
    vol = volume._struct()
    _capi.call("fdgs_tsdf_integrate", dev, C.byref(vol), len(views), views.structs)


@torch.no_grad()
def fuse(model, cameras, pipe, bg, volume: TSDFVolume, *, alpha_min: float = 0.5, masks=None, intrinsics=None) -> TSDFVolume:
    """Renders every camera with ``render()`` and integrates depth, alpha and colour of all of them into ``volume`` in one call.
    ``masks``: one [1, H, W] tensor (or None) per camera.  ``intrinsics``: one ``intrinsics_of(camera)`` per camera, for callers that
    fuse the same rig again and again (``fuse_sequence``); default: read from the cameras here."""
    from .gaussian_renderer import render
    cameras = list(cameras)
    if masks is not None and len(masks) != len(cameras):
        raise ValueError("fdgs: fuse needs one mask (or None) per camera")
    if intrinsics is not None and len(intrinsics) != len(cameras):
        raise ValueError("fdgs: fuse needs one intrinsics tuple per camera")
    views = []
    for n, cam in enumerate(cameras):
        pkg = render(cam, model, pipe, bg)
        views.append({"depth": pkg["depth"], "alpha": pkg["alpha"], "image": pkg["render"], "mask": None if masks is None else masks[n],
                      "camera": cam, "alpha_min": alpha_min, "intrinsics": None if intrinsics is None else intrinsics[n]})
    integrate(volume, views)
    return volume


@dataclass
class Mesh:
    vertices: torch.Tensor   # [V, 3] float32
    normals: torch.Tensor    # [V, 3] float32, unit (towards growing distance: out of the surface) or 0
    colors: torch.Tensor     # [V, 3] float32
    faces: torch.Tensor      # [F, 3] int32


def _empty_mesh(V, F, dev) -> Mesh:
    return Mesh(*[torch.empty((V, 3), dtype=torch.float32, device=dev) for _ in range(3)], torch.empty((F, 3), dtype=torch.int32, device=dev))


def _surface_out(counts, vcap=0, fcap=0, vertices=None, normals=None, colors=None, faces=None):
    """fdgs_surface_out: the two counters in ``counts`` and, for an emitting pass, the four arrays with their capacities."""
    return _capi.FdgsSurfaceOut(int(vcap), int(fcap), _capi._ptr(vertices), _capi._ptr(normals), _capi._ptr(colors), _capi._ptr(faces),
                                counts.data_ptr(), counts.data_ptr() + 4)


def _two_pass(call, counts, dev) -> Mesh:
    """What every mesh-producing entry point asks for: ``call()`` counts, one read of the two counters, exact allocation,
    ``call(vcap, fcap, vertices, normals, colors, faces)`` emits."""
    call()
    V, F = (int(v) for v in counts.cpu())
    mesh = _empty_mesh(V, F, dev)
    if V > 0:
        call(V, F, mesh.vertices, mesh.normals, mesh.colors, mesh.faces)
    return mesh


def _extract_call(volume, min_weight, counts, scratch, vcap=0, fcap=0, vertices=None, normals=None, colors=None, faces=None):
    vol, sout = volume._struct(), _surface_out(counts, vcap, fcap, vertices, normals, colors, faces)
    _capi.call("fdgs_surface_extract", volume.device, C.byref(vol), float(min_weight), C.byref(sout), scratch.data_ptr())


def extract(volume: TSDFVolume, min_weight: float = 1.0) -> Mesh:
    """The surface-nets mesh of the voxels with ``weight >= min_weight``: a count pass, one read of the two counters, exact
    allocation, the emitting pass."""
    dev = volume.device
    if volume.voxels == 0:
        return _empty_mesh(0, 0, dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    scratch = _capi.scratch(_capi.lib.fdgs_surface_extract_scratch_bytes(*volume.dims), dev, floor=256)
    return _two_pass(lambda *out: _extract_call(volume, min_weight, counts, scratch, *out), counts, dev)


def fuse_sequence(model, cameras, pipe, bg, volume: TSDFVolume, timestamps, *, alpha_min: float = 0.5, min_weight: float = 1.0):
    """Yields one ``Mesh`` per timestamp: the cameras moved to that time (``fdgs.playback.with_timestamp``), fused into the one
    ``volume`` -- reset in between -- and extracted.  The cameras' intrinsics are read once, not per timestamp."""
    from .playback import with_timestamp
    cameras = list(cameras)
    intrinsics = [intrinsics_of(c) for c in cameras]
    for t in timestamps:
        volume.reset()
        fuse(model, [with_timestamp(c, t) for c in cameras], pipe, bg, volume, alpha_min=alpha_min, intrinsics=intrinsics)
        yield extract(volume, min_weight)


# ---- cleaning and smoothing (csrc/mesh.hip) ----
@dataclass
class MeshComponents:
    vertex_component: torch.Tensor   # [V] int32: dense ids, in ascending order of each component's smallest vertex index
    n: int                           # the number of components
    vertex_counts: torch.Tensor      # [n] int32
    face_counts: torch.Tensor        # [n] int32: a face counts for the component of its first index
    rounds: int = 0                  # hook passes the union-find took (the last one is the convergence check)


def _mesh_struct(mesh: Mesh):
    """(fdgs_mesh_in, device, the tensors its pointers refer to) of a mesh on the GPU."""
    named = (("vertices", mesh.vertices), ("normals", mesh.normals), ("colors", mesh.colors), ("faces", mesh.faces))
    for name, t in named:
        _capi.need_gpu(t, name)
        if t.device != mesh.vertices.device:
            raise RuntimeError("fdgs: '%s' lives on %s, the vertices on %s" % (name, t.device, mesh.vertices.device))
    V, F = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    for name, t in named[:3]:
        if tuple(t.shape) != (V, 3):
            raise ValueError("fdgs: '%s' must be [V, 3] = %s; got %s" % (name, (V, 3), tuple(t.shape)))
    if tuple(mesh.faces.shape) != (F, 3):
        raise ValueError("fdgs: faces must be [F, 3]; got %s" % (tuple(mesh.faces.shape),))
    keep = [t.detach().contiguous().float() for _, t in named[:3]] + [mesh.faces.detach().contiguous().to(torch.int32)]
    return _capi.FdgsMeshIn(V, F, *[_capi._ptr(t) for t in keep]), mesh.vertices.device, keep


def _components_call(struct, dev, cap, vertex_component, counter, vertex_counts=None, face_counts=None, labelled=False) -> int:
    """fdgs_mesh_components on the current stream; returns the hook passes it took.  ``labelled``: ``vertex_component`` holds an
    earlier call's ids, only the counts are computed."""
    rounds = C.c_int32(0)
    out = _capi.FdgsMeshComponentsOut(int(cap), int(bool(labelled)), _capi._ptr(vertex_component), counter.data_ptr(), _capi._ptr(vertex_counts),
                                      _capi._ptr(face_counts), C.pointer(rounds))
    scratch = _capi.scratch(_capi.lib.fdgs_mesh_components_scratch_bytes(struct.V, struct.F), dev, floor=256)
    _capi.call("fdgs_mesh_components", dev, C.byref(struct), C.byref(out), scratch.data_ptr())
    return int(rounds.value)


def _compact_call(struct, dev, vertex_component, keep, counts, vcap=0, fcap=0, vertices=None, normals=None, colors=None, faces=None):
    sout = _surface_out(counts, vcap, fcap, vertices, normals, colors, faces)
    scratch = _capi.scratch(_capi.lib.fdgs_mesh_compact_scratch_bytes(struct.V, struct.F), dev, floor=256)
    _capi.call("fdgs_mesh_compact", dev, C.byref(struct), _capi._ptr(vertex_component), _capi._ptr(keep), int(keep.numel()), C.byref(sout),
               scratch.data_ptr())


def _smooth_call(struct, dev, iterations, lam, mu, pin_boundary, vertices=None, normals=None, boundary=None):
    out = _capi.FdgsMeshSmoothOut(int(iterations), float(lam), float(mu), int(bool(pin_boundary)), _capi._ptr(vertices), _capi._ptr(normals),
                                  _capi._ptr(boundary))
    scratch = _capi.scratch(_capi.lib.fdgs_mesh_smooth_scratch_bytes(struct.V, struct.F), dev, floor=256)
    _capi.call("fdgs_mesh_smooth", dev, C.byref(struct), C.byref(out), scratch.data_ptr())


def components(mesh: Mesh) -> MeshComponents:
    """The connected components of the mesh's vertices under its (present) faces: labels first, one read of the one counter, exact
    allocation of the two count arrays, the counts."""
    struct, dev, _held = _mesh_struct(mesh)
    V = struct.V
    vc = torch.empty(V, dtype=torch.int32, device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    rounds = _components_call(struct, dev, 0, vc, counter)
    n = int(counter.cpu())
    vcount, fcount = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    if n > 0:
        _components_call(struct, dev, n, vc, counter, vcount, fcount, labelled=True)
    return MeshComponents(vc, n, vcount, fcount, rounds)


def clean(mesh: Mesh, *, keep_largest=None, min_faces=None) -> Mesh:
    """The mesh without its floaters: the ``keep_largest`` components with the most faces (ties go to the smaller component id) that
    also have at least ``min_faces`` faces -- a component must pass every criterion given.  With neither, only components without a
    face (stray vertices) and absent faces go.  Survivors keep their order; attribute rows are copied bit for bit."""
    struct, dev, _held = _mesh_struct(mesh)
    comp = components(mesh)
    keep = comp.face_counts > 0
    if min_faces is not None:
        keep &= comp.face_counts >= int(min_faces)
    if keep_largest is not None:
        if int(keep_largest) < 0:
            raise ValueError("fdgs: keep_largest must not be negative; got %s" % (keep_largest,))
        order = torch.sort(comp.face_counts.cpu(), descending=True, stable=True).indices[:int(keep_largest)]     # the one small read
        largest = torch.zeros(comp.n, dtype=torch.bool)
        largest[order] = True
        keep &= largest.to(dev)
    keep = keep.to(torch.uint8)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    return _two_pass(lambda *out: _compact_call(struct, dev, comp.vertex_component, keep, counts, *out), counts, dev)


def smooth(mesh: Mesh, iterations: int = 10, lam: float = 0.5, mu: float = -0.53, *, pin_boundary: bool = True,
           recompute_normals: bool = True) -> Mesh:
    """Taubin smoothing: ``iterations`` times a pass with factor ``lam``, then one with ``mu`` (negative: it undoes the shrinking), each
    moving a vertex towards the mean of its incident faces' other corners; boundary vertices stay where they are with
    ``pin_boundary``.  Returns a new mesh -- the normals from the smoothed faces (``recompute_normals``) or copied, the colours and
    faces copied; the input is left untouched."""
    struct, dev, held = _mesh_struct(mesh)
    out = Mesh(torch.empty_like(held[0]), torch.empty_like(held[1]) if recompute_normals else held[1].clone(), held[2].clone(), held[3].clone())
    _smooth_call(struct, dev, iterations, lam, mu, pin_boundary, out.vertices, out.normals if recompute_normals else None)
    return out


# ---- simplification (csrc/mesh_simplify.hip) ----
_PLACEMENTS = {"mean": _capi.FDGS_SIMPLIFY_MEAN, "quadric": _capi.FDGS_SIMPLIFY_QUADRIC}
_MAX_CELLS = 2 ** 30


def _simplify_call(struct, dev, origin, cell, dims, placement, stabilise, counts, scratch=None, vcap=0, fcap=0, vertices=None, normals=None,
                   colors=None, faces=None, vertex_map=None):
    params = _capi.FdgsMeshSimplifyParams(*[int(d) for d in dims], *[float(o) for o in origin], float(cell), int(placement), float(stabilise),
                                          _capi._ptr(vertex_map))
    sout = _surface_out(counts, vcap, fcap, vertices, normals, colors, faces)
    if scratch is None:
        scratch = _capi.scratch(_capi.lib.fdgs_mesh_simplify_scratch_bytes(struct.V, struct.F), dev, floor=256)
    _capi.call("fdgs_mesh_simplify", dev, C.byref(struct), C.byref(params), C.byref(sout), scratch.data_ptr())


def _bounds(vertices):
    """(min [3], max [3]) of the finite vertices as float64 numpy arrays, or None without one: one small reduction, one host read."""
    finite = vertices[torch.isfinite(vertices).all(1)]
    if finite.shape[0] == 0:
        return None
    both = torch.stack([finite.min(0).values, finite.max(0).values]).double().cpu().numpy()
    return both[0], both[1]


def _grid_dims(extent, cell):
    return tuple(int(np.floor(e / cell)) + 1 for e in extent)


def _grid_for(bounds, cell, origin=None):
    """(origin [3], dims) of the grid ``simplify`` uses for vertices within ``bounds`` = (min [3], max [3]) or None; ValueError beyond 2^30 cells."""
    lo = np.zeros(3) if bounds is None else np.asarray(bounds[0], np.float64)
    start = lo if origin is None else np.asarray([float(o) for o in origin], np.float64)
    if start.shape != (3,) or not np.isfinite(start).all():
        raise ValueError("fdgs: origin must be three finite numbers; got %s" % (origin,))
    extent = np.zeros(3) if bounds is None else np.maximum(np.asarray(bounds[1], np.float64) - start, 0.0)
    dims = _grid_dims(extent, cell)
    if dims[0] * dims[1] * dims[2] > _MAX_CELLS:
        fit = cell
        while np.prod([float(d) for d in _grid_dims(extent, fit)]) > _MAX_CELLS:
            fit *= 1.05
        raise ValueError("fdgs: a grid of %d x %d x %d cells of size %g is beyond 2^30 cells; a cell size of %g would fit" % (dims + (cell, fit)))
    return start, dims


def simplify(mesh: Mesh, cell: float, *, origin=None, placement: str = "quadric", stabilise: float = 1e-3, return_map: bool = False):
    """Vertex clustering: all vertices in one cell of a grid of edge ``cell`` become one vertex -- placed where the planes of the faces
    around them meet (``"quadric"``: the minimiser of the summed squared plane distances, pulled towards the members' mean with weight
    ``stabilise`` and kept inside the cell) or at their mean (``"mean"``) -- with the mean colour and the normalised sum of the normals.
    Faces are mapped through the clusters; those with two corners in one cluster and repeats of a face go (two faces of opposite
    winding on the same three clusters are different faces: both stay).  One pass, independent of the order of anything, bit for bit
    reproducible; the price against edge collapse is that the topology may pinch where two sheets pass through one cell.
    With ``origin=None`` the grid starts at the per-axis minimum of the finite vertices (one small device reduction and one host read)
    and has ``floor(extent / cell) + 1`` cells per axis; with an ``origin`` it reaches to the vertices' maximum the same way.  Vertices
    with a non-finite coordinate, and the faces that use them, are dropped; stray vertices are clusters like any other (``clean``
    removes them).  ``return_map``: also the [V] int32 cluster of every input vertex (-1 for none)."""
    struct, dev, _held = _mesh_struct(mesh)
    cell = float(cell)
    if not (cell > 0 and np.isfinite(cell)):
        raise ValueError("fdgs: simplify needs a positive, finite cell size; got %s" % (cell,))
    if placement not in _PLACEMENTS:
        raise ValueError("fdgs: placement must be 'mean' or 'quadric'; got %r" % (placement,))
    start, dims = _grid_for(_bounds(_held[0]) if struct.V > 0 else None, cell, origin)
    V = struct.V
    vmap = torch.empty(V, dtype=torch.int32, device=dev) if return_map else None
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    scratch = _capi.scratch(_capi.lib.fdgs_mesh_simplify_scratch_bytes(struct.V, struct.F), dev, floor=256)
    args = (struct, dev, start, cell, dims, _PLACEMENTS[placement], stabilise, counts, scratch)
    out = _two_pass(lambda *o: _simplify_call(*args, *o, vertex_map=None if o else vmap), counts, dev)   # the counting pass writes the map
    return (out, vmap) if return_map else out


def cell_for_target(mesh: Mesh, target_faces: int, probes: int = 12) -> float:
    """A cell size at which ``simplify(mesh, cell)`` has at most ``target_faces`` faces: ``probes`` count-only calls bisect the cell size
    geometrically between the bounding box's diagonal (one cell: no face) and 1/1024 of it, and the probed size with the most faces not
    above the target is returned.  The face count is not monotone in the cell size, so this is the best probe, not the best cell."""
    struct, dev, _held = _mesh_struct(mesh)
    if int(target_faces) < 0:
        raise ValueError("fdgs: target_faces must not be negative; got %s" % (target_faces,))
    bounds = _bounds(_held[0]) if struct.V > 0 else None
    diagonal = 0.0 if bounds is None else float(np.linalg.norm(bounds[1] - bounds[0]))
    if not (diagonal > 0 and np.isfinite(diagonal)):
        return 1.0                                        # nothing, or one point: every grid gives no face
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    scratch = _capi.scratch(_capi.lib.fdgs_mesh_simplify_scratch_bytes(struct.V, struct.F), dev, floor=256)

    def faces_at(cell):
        _simplify_call(struct, dev, bounds[0], cell, _grid_dims(bounds[1] - bounds[0], cell), _capi.FDGS_SIMPLIFY_MEAN, 0.0, counts, scratch)
        return int(counts.cpu()[1])
    large, small = diagonal * (1.0 + 2.0 ** -20), diagonal / 1024.0      # just above the diagonal: one cell along every axis
    best, best_faces = large, faces_at(large)
    for _ in range(int(probes)):
        cell = float(np.sqrt(large * small))
        n = faces_at(cell)
        if n <= int(target_faces):
            if n >= best_faces:
                best, best_faces = cell, n
            large = cell
        else:
            small = cell
    return best


# ---- PLY: a triangle mesh, binary little-endian as fdgs.slice's files ----
_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                    ("red", "u1"), ("green", "u1"), ("blue", "u1")])
_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def save_mesh_ply(path, mesh: Mesh) -> None:
    """Binary little-endian PLY: vertices x y z nx ny nz + uchar red green blue (the colour clamped to [0, 1], times 255, rounded),
    faces as ``vertex_indices`` lists of three int32."""
    cpu = lambda t: t.detach().cpu().numpy()  # noqa: E731
    V, F = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    vert = np.zeros(V, _VERTEX)
    xyz, nrm = cpu(mesh.vertices), cpu(mesh.normals)
    for k, name in enumerate(("x", "y", "z")):
        vert[name] = xyz[:, k]
        vert["n" + name] = nrm[:, k]
    rgb = np.floor(np.clip(np.nan_to_num(cpu(mesh.colors).astype(np.float64)), 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
    vert["red"], vert["green"], vert["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    face = np.zeros(F, _FACE)
    face["n"] = 3
    face["v"] = cpu(mesh.faces)
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % V
    header += "".join("property float %s\n" % n for n in ("x", "y", "z", "nx", "ny", "nz"))
    header += "".join("property uchar %s\n" % n for n in ("red", "green", "blue"))
    header += "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % F
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(vert.tobytes())
        fh.write(face.tobytes())


def load_mesh_ply(path, device) -> Mesh:
    """The mesh of a PLY in the layout ``save_mesh_ply`` writes; colours come back as ``byte / 255``."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or "format binary_little_endian 1.0" not in lines:
        raise ValueError("load_mesh_ply: %s is not a binary little-endian PLY" % path)
    props = [ln for ln in lines if ln.startswith(("element", "property"))]
    V = next(int(ln.split()[2]) for ln in lines if ln.startswith("element vertex"))
    F = next((int(ln.split()[2]) for ln in lines if ln.startswith("element face")), 0)
    want = (["element vertex %d" % V] + ["property float %s" % n for n in ("x", "y", "z", "nx", "ny", "nz")]
            + ["property uchar %s" % n for n in ("red", "green", "blue")] + ["element face %d" % F, "property list uchar int vertex_indices"])
    if props != want:
        raise ValueError("load_mesh_ply: %s is not in the layout save_mesh_ply writes" % path)
    vert = np.frombuffer(data, _VERTEX, count=V, offset=end)
    face = np.frombuffer(data, _FACE, count=F, offset=end + V * _VERTEX.itemsize)
    if F and not (face["n"] == 3).all():
        raise ValueError("load_mesh_ply: only triangles are supported")
    t = lambda a, dt: torch.from_numpy(np.array(a)).to(dt).to(device)  # noqa: E731
    return Mesh(t(np.stack([vert["x"], vert["y"], vert["z"]], 1), torch.float32), t(np.stack([vert["nx"], vert["ny"], vert["nz"]], 1), torch.float32),
                t(np.stack([vert["red"], vert["green"], vert["blue"]], 1).astype(np.float32) / np.float32(255.0), torch.float32),
                t(face["v"].copy().reshape(F, 3), torch.int32))
