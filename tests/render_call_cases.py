"""What the layer between the user and the native binding hands to ``_C.rasterize_gaussians`` / ``_C.rasterize_gaussians_backward``, and
where the backward's 12 results end up: every render path on CPU tensors with the two entry points replaced by recording stand-ins.
tests/golden/make_golden_render_calls.py records the trace of every case from the commit BEFORE a change to that layer;
tests/test_render_calls_host.py holds the code to it.  No case needs a GPU.

The forward stand-in returns zero tensors; the backward stand-in returns, for slot i of the 12-tuple, a tensor filled with i + 1 (and
writes or adds that value into a ``grad_out`` buffer given for the slot, and 13 + j into camera gradient j), so a parameter's
``.grad`` says which slot reached it and through which activation.  Not reachable this way, and left to the GPU suite: render()'s fast
path (it refuses CPU tensors) and everything below the binding's ``_scene``."""
import torch

PARAMS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation", "_t", "_scaling_t", "_rotation_r")
CAMERA = ("world_view_transform", "full_proj_transform", "camera_center", "timestamp")
SLOTS = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dflows", "dL_dts", "dL_dscales",
         "dL_dscales_t", "dL_drotations", "dL_drotations_r")
# name -> (rot_4d, gaussian_dim, SH degree, temporal SH degree, the model's prefilter_var)
MODELS = {"3d_sh2": (False, 3, 2, 0, 0.25), "4d_sh1": (False, 4, 1, 0, 0.25), "rot4d_sh3_sht2": (True, 4, 3, 2, -1.0)}


def _first(t):
    return None if t is None else float(t.detach().flatten()[0])


class Recorder:
    """The two stand-ins and the log they write."""

    def __init__(self):
        self.log, self.roles = [], []

    def name(self, role, t):
        if isinstance(t, torch.Tensor):
            self.roles.append((role, t))

    def _describe(self, a):
        if isinstance(a, torch.Tensor):
            role = "new"
            if a.numel() == 0:
                role = "empty"
            for name, t in self.roles:
                if t.numel() and t.data_ptr() == a.data_ptr() and t.shape == a.shape:
                    role = name
            return {"role": role, "shape": list(a.shape), "dtype": str(a.dtype)}
        if isinstance(a, dict):
            return {"dict": sorted(a)}
        if callable(a):
            return "callable"
        return a

    def _note(self, fn, a, k):
        self.log.append({"fn": fn, "args": [self._describe(x) for x in a], "kwargs": {n: self._describe(v) for n, v in sorted(k.items())}})

    def forward(self, *a, **k):
        self._note("rasterize_gaussians", a, k)
        P, H, W = a[1].shape[0], a[17], a[18]
        z = torch.zeros
        u8 = torch.zeros(4, dtype=torch.uint8)
        return (7, z(3, H, W), z(2, H, W), z(1, H, W), z(1, H, W), torch.ones(P, dtype=torch.int32), u8, u8.clone(), u8.clone(), z(P, 6),
                z(P, 3))

    def backward(self, *a, **k):
        self._note("rasterize_gaussians_backward", a, k)
        P = a[1].shape[0]
        M = a[23].shape[1] if a[23].numel() else 0
        shapes = ((P, 3), (P, 3), (P, 1), (P, 3), (P, 6), (P, M, 3), (P, 2), (P, 1), (P, 3), (P, 1), (P, 4), (P, 4))
        out = []
        for i, (slot, shape) in enumerate(zip(SLOTS, shapes)):
            t = (k.get("grad_out") or {}).get(slot)
            if t is None:
                t = torch.full(shape, float(i + 1))
            elif k.get("accumulate"):
                t.add_(float(i + 1))
            else:
                t.fill_(float(i + 1))
            out.append(t)
        camera = k.get("camera")
        if camera is not None:
            names, shp = ("viewmatrix", "projmatrix", "campos", "timestamp"), ((4, 4), (4, 4), (3,), (1,))
            camera["grads"] = {n: (torch.full(s, 13.0 + j) if w else None) for j, (n, s, w) in enumerate(zip(names, shp, camera["want"]))}
        return tuple(out)


class _Pipe:
    def __init__(self, **kw):
        self.compute_cov3D_python = self.convert_SHs_python = self.debug = False
        self.env_map_res = 0
        self.__dict__.update(kw)


class _GettersOnly:
    """A model that only has the reference's post-activation getters (no raw ``_xyz`` ... attributes)."""

    def __init__(self, m):
        for n in ("get_xyz", "get_opacity", "get_scaling", "get_rotation", "get_t", "get_scaling_t", "get_rotation_r", "get_features"):
            setattr(self, n, getattr(m, n).detach())
        for n in ("active_sh_degree", "active_sh_degree_t", "time_duration", "rot_4d", "gaussian_dim", "force_sh_3d", "prefilter_var"):
            setattr(self, n, getattr(m, n))


def _sink(model, fill):
    t = {"dL_dmeans3D": model._xyz, "dL_dsh": model.get_features, "dL_dopacity": model._opacity, "dL_dscales": model._scaling,
         "dL_drotations": model._rotation, "dL_dts": model._t, "dL_dscales_t": model._scaling_t, "dL_drotations_r": model._rotation_r}
    return {k: torch.full(tuple(v.shape), float(fill)) for k, v in t.items()}


def _paths():
    """name -> (what to call, given (model, camera, bg, recorder); returns the result dict or None), wants a learnable camera"""
    from fdgs import importance
    from fdgs.fused import render_raw
    from fdgs.gaussian_renderer import render

    def override(m, c, bg, rec):
        colour = torch.full((m._xyz.shape[0], 3), 0.5, requires_grad=True)
        rec.name("override_color", colour)
        return render(c, m, _Pipe(), bg, override_color=colour)

    def sunk(accumulate):
        def run(m, c, bg, rec):
            rec.sink = _sink(m, 100.0 if accumulate else 0.0)
            for k, t in rec.sink.items():
                rec.name("sink." + k, t)
            return render_raw(c, m, _Pipe(), bg, grad_sink=rec.sink, accumulate=accumulate)
        return run

    def contribution(getters):
        def run(m, c, bg, rec):
            model = _GettersOnly(m) if getters else m
            if getters:
                rec.name("get_xyz", model.get_xyz)
                rec.name("get_features", model.get_features)
            assert len(importance._forward(model, c, _Pipe(), bg, False)) == 11
        return run

    return {
        "render": (lambda m, c, bg, rec: render(c, m, _Pipe(), bg), False),
        "render-cov3D_python": (lambda m, c, bg, rec: render(c, m, _Pipe(compute_cov3D_python=True), bg), False),
        "render-SHs_python": (lambda m, c, bg, rec: render(c, m, _Pipe(convert_SHs_python=True), bg), False),
        "render-override_color": (override, False),
        "render_raw": (lambda m, c, bg, rec: render_raw(c, m, _Pipe(), bg), False),
        "render_raw-sink": (sunk(False), False),
        "render_raw-sink-accumulate": (sunk(True), False),
        "render-camera": (lambda m, c, bg, rec: render(c, m, _Pipe(), bg), True),
        "render_raw-camera": (lambda m, c, bg, rec: render_raw(c, m, _Pipe(), bg), True),
        "importance-raw": (contribution(False), False),
        "importance-getters": (contribution(True), False),
    }


_SCENES = {}


def _scene(kind):
    from fdgs import synth
    if kind not in _SCENES:
        rot_4d, dim, deg, deg_t, _pv = MODELS[kind]
        _SCENES[kind] = synth.make_scene(synth.SceneConfig(kind, 40, 32, 16, deg, deg_t, 0.05, 2.0, rot_4d, dim, False), seed=3)
    return _SCENES[kind]


def cases():
    """["<model>/<path>"]"""
    return ["%s/%s" % (m, p) for m in MODELS for p in _paths()]


def run(case, patch):
    """The trace of one case.  ``patch(object, attribute name, value)`` replaces the two entry points (pytest's monkeypatch.setattr, or
    plain setattr in the recording script)."""
    from fdgs import train_host
    from fdgs.gaussian_renderer import diff_gaussian_rasterization as dgr
    kind, path = case.split("/")
    fn, learnable_camera = _paths()[path]
    rec = Recorder()
    rec.sink = None
    patch(dgr._C, "rasterize_gaussians", rec.forward)
    patch(dgr._C, "rasterize_gaussians_backward", rec.backward)
    sc = _scene(kind)
    model = train_host.ReferenceStyleModel(sc, "cpu")
    model.prefilter_var = MODELS[kind][4]
    cam = train_host.SyntheticCamera(sc, "cpu")
    if learnable_camera:
        for n in CAMERA[:3]:
            setattr(cam, n, getattr(cam, n).clone().requires_grad_(True))
        cam.timestamp = torch.tensor(float(cam.timestamp), requires_grad=True)
    bg = torch.tensor([0.1, 0.2, 0.3])
    rec.name("bg", bg)
    for n in PARAMS:
        rec.name(n, getattr(model, n))
    for n in CAMERA:
        rec.name("camera." + n, getattr(cam, n))
    out = {}
    try:
        pkg = fn(model, cam, bg, rec)
        if pkg is not None:
            (pkg["render"].sum() + pkg["depth"].sum()).backward()
            out["grads"] = {n: _first(getattr(model, n).grad) for n in PARAMS}
            out["grads"]["viewspace_points"] = _first(pkg["viewspace_points"].grad)
            for n in CAMERA:
                t = getattr(cam, n)
                out["grads"]["camera." + n] = _first(t.grad) if isinstance(t, torch.Tensor) else None
            if rec.sink is not None:
                out["sink"] = {k: _first(t) for k, t in sorted(rec.sink.items())}
    except Exception as e:  # noqa: BLE001 -- a path that refuses a model is recorded as that
        out["raised"] = [type(e).__name__, str(e)]
    out["calls"] = rec.log
    return out
